"""wgrad dW[N,K] = dy^T[N,M] @ x[M,K] at the four flagship shapes
(gpt2-345m, batch 64 x seq 1024 -> M = 65536 tokens), three ways:

  a  transposes + canonical hand GEMM: transpose_dy(dy), transpose2d(x),
     then the 256 kernel on two k-contiguous operands (the hand path before
     the kernel read k-outer operands)
  b  the 256 kernel on dy and x as they lie (both k-outer)
  c  torch.matmul(dy.t(), x) (hipBLASLt)

One window = one call on each of SETS distinct operand sets (so no input
sits in the Infinity Cache from the previous call), timed with device
events; the windows of a, b, c are interleaved in one process. Reports the
per-call median and min..max over the windows in microseconds.

Run on the GPU: python benchmarks/wgrad_tn.py [--out profiles/wgrad_tn.json]

--colsum times the bias gradient instead, same shapes and method:

  d  b, then the streaming bias sum over dy (hip._bias_sum: workspace
     fill, bias_sum kernel, cast), what a biased site ran before
  e  one hand call that also returns the column sums of dy (colsum_out)
  b  the in-place wgrad alone, to show what the column sums add to it

python benchmarks/wgrad_tn.py --colsum [--out profiles/wgrad_colsum.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd.ops import hip

BF16 = torch.bfloat16
M = 65536
SHAPES = [("proj", 1024, 1024), ("qkv", 3072, 1024), ("fc", 4096, 1024),
          ("out", 1024, 4096)]       # (name, N, K) of y[M,N] = x[M,K] @ w^T
SETS = 8
WINDOWS = 9


def with_transposes(dy, x, N, K):
    dyT = torch.empty(N, M, dtype=BF16, device=dy.device)
    hip.ext.transpose_dy(dy.data_ptr(), 0, dyT.data_ptr(), 0, 0, M, N,
                         hip._stream())
    xT = hip.transpose2d(x)
    return hip._gemm_raw(dyT, xT, True, True, N, K, M, M, M, 0, 0, 1)[0]


def in_place(dy, x, N, K):
    return hip._gemm_raw(dy, x, False, False, N, K, M, N, K, 0, 0, 1)[0]


def library(dy, x, N, K):
    return torch.matmul(dy.t(), x)


def in_place_plus_bias_sum(dy, x, N, K):
    return in_place(dy, x, N, K), hip._bias_sum(dy)


def fused_colsum(dy, x, N, K):
    db = torch.empty(N, dtype=BF16, device=dy.device)
    dw = hip._gemm_raw(dy, x, False, False, N, K, M, N, K, 0, 0, 1,
                       colsum_out=db)[0]
    return dw, db


def window(fn, sets, N, K):
    """Microseconds per call over one pass through the operand sets."""
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    beg.record()
    for dy, x in sets:
        fn(dy, x, N, K)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / len(sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--colsum", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    ways = [("a_transposes_plus_kc_gemm", with_transposes),
            ("b_in_place", in_place), ("c_torch_matmul", library)]
    if args.colsum:
        ways = [("d_in_place_plus_bias_sum", in_place_plus_bias_sum),
                ("e_fused_colsum", fused_colsum), ("b_in_place", in_place)]
    rows = []
    for name, N, K in SHAPES:
        plan = hip.ext.gemm_plan(N, K, M, N, K, False, False, 0, 1)[:3]
        assert plan[0] == 256, (name, plan)
        sets = [(torch.randn(M, N, device="cuda", dtype=BF16),
                 torch.randn(M, K, device="cuda", dtype=BF16))
                for _ in range(SETS)]
        # the three agree before anything is timed
        ref = library(*sets[0], N, K).float()
        if args.colsum:
            dw_d, db_d = in_place_plus_bias_sum(*sets[0], N, K)
            dw_e, db_e = fused_colsum(*sets[0], N, K)
            assert torch.equal(dw_d, dw_e), name
            s32 = sets[0][0].float().sum(0)
            for db in (db_d, db_e):
                err = (db.float() - s32).abs().max().item()
                assert err < 3e-2 * M ** 0.5, (name, err)
        for _, fn in ([] if args.colsum else ways[:2]):
            err = (fn(*sets[0], N, K).float() - ref).abs().max().item()
            assert err < 3e-2 * M ** 0.5, (name, err)
        times = {w: [] for w, _ in ways}
        for w, fn in ways:                       # warm-up pass each
            window(fn, sets, N, K)
        for _ in range(WINDOWS):
            for w, fn in ways:
                times[w].append(window(fn, sets, N, K))
        row = {"shape": name, "N": N, "K": K, "M": M, "plan": list(plan),
               "sets": SETS, "windows": WINDOWS, "unit": "us per call"}
        for w, _ in ways:
            t = times[w]
            row[w] = {"median": round(statistics.median(t), 1),
                      "min": round(min(t), 1), "max": round(max(t), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0),
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
