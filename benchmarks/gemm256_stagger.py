"""The 256-tile GEMM of this tree against another build of it (the parent
commit's, before the wave halves were staggered) and against hipBLASLt, at
the flagship shapes (gpt2-345m, batch 64 x seq 1024 -> 65536 tokens):

  wgrad   four in-place wgrads with column sums (k-outer operands)
  fwd     four forwards with the bias epilogue, fc also with bias+gelu
  dgelu   fc dgrad with the dgelu epilogue
  square  4096^3 and 8192^3, plain

The method is benchmarks/wgrad_tn.py's: one window = one call on each of SETS
distinct random operand sets (no input sits in the Infinity Cache from the
previous call), timed with device events; the windows of all contenders are
interleaved in one process; per-call median and min..max over the windows in
microseconds. Both builds' extensions are loaded side by side and their
outputs compared bit for bit before anything is timed. A shape counts as
faster only if this build's slowest window beats the other's fastest.

python benchmarks/gemm256_stagger.py --parent /path/to/other/_tepdist_hip.so \
    [--out profiles/gemm256_stagger.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd.ops import hip

BF16 = torch.bfloat16
T = 65536
SETS = 8
WINDOWS = 9
NEW_EXT = hip.ext


def load_ext(path):
    # a qualified name of its own: the import system caches extension
    # modules by name, the init symbol comes from the last component
    spec = importlib.util.spec_from_file_location(
        "gemm256_parent._tepdist_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rnd(*shape):
    return torch.randn(*shape, device="cuda", dtype=BF16)


# each case: (name, M, N, K of the GEMM, make(set) -> operands,
#             hand(ops) -> tensors, lib(ops) -> tensors)
def wgrad_case(name, N, K):
    def make():
        return rnd(T, N), rnd(T, K)

    def hand(o):
        dy, x = o
        db = torch.empty(N, dtype=BF16, device="cuda")
        dw = hip._gemm_raw(dy, x, False, False, N, K, T, N, K, 0, 0, 1,
                           colsum_out=db)[0]
        return dw, db

    def lib(o):
        dy, x = o
        return torch.matmul(dy.t(), x), hip._bias_sum(dy)

    plan = NEW_EXT.gemm_plan(N, K, T, N, K, False, False, 0, 1)
    return dict(name=f"wgrad_{name}_colsum", mnk=(N, K, T), plan=plan,
                make=make, hand=hand, lib=lib)


def fwd_case(name, N, K, epi):
    def make():
        return rnd(T, K), rnd(N, K) * 0.03, rnd(N)

    def hand(o):
        x, w, b = o
        return hip._gemm_raw(x, w, True, True, T, N, K, K, K, 0, 0, 1,
                             bias=b, epi=epi)

    def lib(o):
        x, w, b = o
        pre = torch.nn.functional.linear(x, w, b)
        if epi == 1:
            return pre, None
        return hip.gelu_fwd(pre), pre

    plan = NEW_EXT.gemm_plan(T, N, K, K, K, True, True, epi, 1)
    tag = "bias" if epi == 1 else "bias_gelu"
    return dict(name=f"fwd_{name}_{tag}", mnk=(T, N, K), plan=plan, make=make,
                hand=hand, lib=lib)


def dgelu_case():
    N, K = 4096, 1024        # dh[T, 4d] = dy[T, d] @ w2[d, 4d], * gelu'(pre)

    def make():
        return rnd(T, K), rnd(N, K) * 0.03, rnd(T, N)

    def hand(o):
        dy, w2T, pre = o
        return hip._gemm_raw(dy, w2T, True, True, T, N, K, K, K, 0, 0, 1,
                             epi=4, out_pre=pre)[0]

    def lib(o):
        dy, w2T, pre = o
        return hip.gelu_bwd(torch.matmul(dy, w2T.t()), pre)

    plan = NEW_EXT.gemm_plan(T, N, K, K, K, True, True, 4, 1)
    return dict(name="dgrad_fc_dgelu", mnk=(T, N, K), plan=plan, make=make,
                hand=hand, lib=lib)


def square_case(n):
    def make():
        return rnd(n, n), rnd(n, n)

    def hand(o):
        a, b = o
        return hip._gemm_raw(a, b, True, True, n, n, n, n, n, 0, 0, 1)[0]

    def lib(o):
        a, b = o
        return torch.matmul(a, b.t())

    plan = NEW_EXT.gemm_plan(n, n, n, n, n, True, True, 0, 1)
    return dict(name=f"square_{n}", mnk=(n, n, n), plan=plan, make=make,
                hand=hand, lib=lib)


def cases():
    shapes = [("proj", 1024, 1024), ("qkv", 3072, 1024), ("fc", 4096, 1024),
              ("out", 1024, 4096)]   # (name, N, K) of y[T,N] = x[T,K] @ w^T
    out = [wgrad_case(*s) for s in shapes]
    out += [fwd_case(*s, 1) for s in shapes]
    out += [fwd_case("fc", 4096, 1024, 2), dgelu_case(),
            square_case(4096), square_case(8192)]
    return out


def flat(r):
    r = r if isinstance(r, (tuple, list)) else (r,)
    return [t for t in r if t is not None]


def window(fn, sets):
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    beg.record()
    for o in sets:
        fn(o)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / len(sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None,
                    help="another build's _tepdist_hip.so to compare with")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of case names")
    args = ap.parse_args()
    torch.manual_seed(0)
    parent_ext = load_ext(args.parent) if args.parent else None

    def using(ext, fn):
        def run(o):
            hip.ext = ext
            try:
                return fn(o)
            finally:
                hip.ext = NEW_EXT
        return run

    rows = []
    for c in cases():
        if args.only and args.only not in c["name"]:
            continue
        assert c["plan"][0] == 256, (c["name"], c["plan"])
        sets = [c["make"]() for _ in range(SETS)]
        ways = [("new", using(NEW_EXT, c["hand"]))]
        if parent_ext is not None:
            ways.insert(0, ("parent", using(parent_ext, c["hand"])))
        ways.append(("hipblaslt", c["lib"]))
        bit_equal = None
        if parent_ext is not None:
            got = [flat(fn(sets[0])) for _, fn in ways[:2]]
            torch.cuda.synchronize()
            bit_equal = all(torch.equal(p, n) for p, n in zip(*got))
            del got
        times = {w: [] for w, _ in ways}
        for _, fn in ways:                       # warm-up pass each
            window(fn, sets)
        for _ in range(WINDOWS):
            for w, fn in ways:
                times[w].append(window(fn, sets))
        M, N, K = c["mnk"]
        row = {"case": c["name"], "M": M, "N": N, "K": K,
               "plan": list(c["plan"][:3]), "sets": SETS, "windows": WINDOWS,
               "unit": "us per call", "new_bit_equal_to_parent": bit_equal}
        for w, _ in ways:
            t = times[w]
            row[w] = {"median": round(statistics.median(t), 1),
                      "min": round(min(t), 1), "max": round(max(t), 1),
                      "tflops_median": round(
                          2.0 * M * N * K / statistics.median(t) * 1e-6, 1)}
        if parent_ext is not None:
            row["new_faster"] = row["new"]["max"] < row["parent"]["min"]
            row["new_slower"] = row["new"]["min"] > row["parent"]["max"]
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
