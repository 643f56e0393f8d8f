"""Decode-attention microbenchmark: the fused KV-cache kernel
(ops.decode_attention, append mode) against the composed sequence the
engine's decode step used before it (index_copy_ x2, two batched matmuls
over the whole S_max cache, scale, mask, fp32 softmax, casts, transpose
copy), alternating in one process.

Each variant is captured into a hipGraph holding CALLS back-to-back calls,
call i on its own K/V cache pair — the way the engine's decode step walks
the caches of a 24-layer model, and so that the working set (CALLS x one
layer's cache) does not sit in the 256 MiB Infinity Cache at the default
shape — and timed with device events over REPLAYS replays per window,
WINDOWS windows per variant, fused and composed windows interleaved.
Prints one JSON line per (shape, position) and one per splits-sweep
point.

The achieved-bandwidth figure divides the bytes the algorithm needs — the
valid K and V rows, (p + 1) * D * 2 B each per (b, h); q/out/new rows are
noise next to them — by the fused call time. The bound for this kernel
is HBM bandwidth (about 2 flop per byte streamed, no reuse), so the
figure is to be read against the 8 TB/s HBM3E peak of the MI355X."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd import ops
from tepdist_amd.ops import hip

BF16 = torch.bfloat16
CALLS, REPLAYS, WINDOWS = 24, 10, 5
HBM_PEAK = 8.0e12


def needed_bytes(B, H, D, p):
    return 2 * B * H * (p + 1) * D * 2


def make_case(B, H, D, S_max, p):
    torch.manual_seed(0)
    d = H * D
    kc = [torch.randn(B, H, S_max, D, dtype=BF16, device="cuda")
          for _ in range(CALLS)]
    vc = [torch.randn(B, H, S_max, D, dtype=BF16, device="cuda")
          for _ in range(CALLS)]
    qkv = torch.randn(B, 1, 3 * d, dtype=BF16, device="cuda")
    cur_t = torch.full((1,), p, dtype=torch.long, device="cuda")
    kpos = torch.arange(S_max, device="cuda")
    return kc, vc, qkv, cur_t, kpos


def fused_fn(B, H, D, kc, vc, qkv, cur_t, splits=None):
    q3 = qkv.view(B, 3, H, D)

    def f(i):
        return ops.decode_attention(q3[:, 0], kc[i], vc[i], cur_t,
                                    k_new=q3[:, 1], v_new=q3[:, 2],
                                    splits=splits).reshape(B, 1, H * D)
    return f


def composed_fn(B, H, D, kc, vc, qkv, cur_t, kpos):
    d = H * D
    scale = 1.0 / math.sqrt(D)

    mask = (kpos > cur_t)       # once per step in the engine, not per layer

    def f(i):
        q, k, v = qkv.split(d, dim=-1)
        qh = q.reshape(B, 1, H, D).transpose(1, 2)
        kc[i].index_copy_(2, cur_t, k.reshape(B, 1, H, D).transpose(1, 2))
        vc[i].index_copy_(2, cur_t, v.reshape(B, 1, H, D).transpose(1, 2))
        scores = ops.matmul(qh.contiguous(), kc[i].transpose(-1, -2)) * scale
        scores = scores.masked_fill(mask, float("-inf"))
        p = torch.softmax(scores.float(), dim=-1).to(qkv.dtype)
        a = ops.matmul(p, vc[i])
        return a.transpose(1, 2).reshape(B, 1, d)
    return f


def capture(fn):
    """Warm up eagerly (autotune, code objects), then record CALLS calls."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            fn(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        for i in range(CALLS):
            out = fn(i)
    graph.replay()
    torch.cuda.synchronize()
    return graph, out


def window_us(graph):
    """Device time per call (us) over one window of REPLAYS replays."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * CALLS)


def time_alternating(graphs):
    """graphs: {name: graph}. Interleaves one window per variant, WINDOWS
    rounds; returns {name: (median_us, min_us, max_us)}."""
    t = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            t[k].append(window_us(g))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def run_shape(B, H, D, S_max, positions, sweep):
    for p in positions:
        kc, vc, qkv, cur_t, kpos = make_case(B, H, D, S_max, p)
        auto = hip.decode_splits(B * H, S_max)
        gf, of = capture(fused_fn(B, H, D, kc, vc, qkv, cur_t))
        gc, oc = capture(composed_fn(B, H, D, kc, vc, qkv, cur_t, kpos))
        diff = (of.float() - oc.float()).abs().max().item()
        r = time_alternating({"fused": gf, "composed": gc})
        nb = needed_bytes(B, H, D, p)
        bps = nb / (r["fused"][0] * 1e-6)
        print(json.dumps({
            "bench": "decode_attn", "B": B, "H": H, "D": D, "S_max": S_max,
            "pos": p, "splits": auto,
            "fused_us": round(r["fused"][0], 2),
            "fused_us_min_max": [round(x, 2) for x in r["fused"][1:]],
            "composed_us": round(r["composed"][0], 2),
            "composed_us_min_max": [round(x, 2) for x in r["composed"][1:]],
            "speedup": round(r["composed"][0] / r["fused"][0], 2),
            "needed_kv_bytes": nb,
            "fused_bytes_per_s": round(bps, 0),
            "bound": "HBM bandwidth",
            "share_of_hbm_peak": round(bps / HBM_PEAK, 3),
            "max_abs_diff_fused_vs_composed": round(diff, 5),
        }), flush=True)
        if not sweep:
            continue
        graphs = {s: capture(fused_fn(B, H, D, kc, vc, qkv, cur_t, s))[0]
                  for s in (1, 2, 4, 8, 16)}
        rs = time_alternating(graphs)
        print(json.dumps({
            "bench": "decode_attn_splits", "B": B, "H": H, "D": D,
            "S_max": S_max, "pos": p,
            "fused_us_by_splits": {str(s): round(v[0], 2)
                                   for s, v in rs.items()},
        }), flush=True)


# -- grouped-query attention + RoPE (Llama decode) --------------------------
#
# Three contenders on the same packed projection [q (H D) | k | v (Hkv D)]:
#   fused    one ops.decode_attention(..., rope_theta) on [B,Hkv,S_max,D]
#            caches: rope of q and k_new, append, attention, K/V rows read
#            once per group;
#   composed the engine's composed GQA step: rope_at x2, index_copy_ x2,
#            [B,Hkv,G,D] @ K^T over the whole S_max cache, mask, fp32
#            softmax, @ V;
#   mha      what served GQA before this kernel: ops.rope in a launch of
#            its own, K/V new rows and caches expanded to H heads, the
#            G == 1 kernel on them (G times the K/V bytes).
# needed_kv_bytes counts the Hkv-head rows: the bytes GQA needs.

THETA = 10000.0


def make_gqa_case(B, H, Hkv, D, S_max, p, expanded):
    torch.manual_seed(0)
    G = H // Hkv
    kc = [torch.randn(B, Hkv, S_max, D, dtype=BF16, device="cuda")
          for _ in range(CALLS)]
    vc = [torch.randn(B, Hkv, S_max, D, dtype=BF16, device="cuda")
          for _ in range(CALLS)]
    ke = ve = None
    if expanded:
        ke = [t.repeat_interleave(G, dim=1) for t in kc]
        ve = [t.repeat_interleave(G, dim=1) for t in vc]
    qkv = torch.randn(B, (H + 2 * Hkv) * D, dtype=BF16, device="cuda")
    cur_t = torch.full((1,), p, dtype=torch.long, device="cuda")
    kpos = torch.arange(S_max, device="cuda")
    return kc, vc, ke, ve, qkv, cur_t, kpos


def _views(qkv, B, H, Hkv, D):
    return (qkv[:, :H * D].view(B, H, D),
            qkv[:, H * D:(H + Hkv) * D].view(B, Hkv, D),
            qkv[:, (H + Hkv) * D:].view(B, Hkv, D))


def gqa_fused_fn(B, H, Hkv, D, kc, vc, qkv, cur_t, splits=None):
    q, k, v = _views(qkv, B, H, Hkv, D)

    def f(i):
        return ops.decode_attention(q, kc[i], vc[i], cur_t, k_new=k,
                                    v_new=v, splits=splits,
                                    rope_theta=THETA).reshape(B, H * D)
    return f


def gqa_composed_fn(B, H, Hkv, D, kc, vc, qkv, cur_t, kpos):
    from tepdist_amd.ops import reference as ref
    G = H // Hkv
    scale = 1.0 / math.sqrt(D)
    dead = (kpos > cur_t)
    q, k, v = _views(qkv, B, H, Hkv, D)

    def f(i):
        qr = ref.rope_at(q, cur_t, THETA).view(B, Hkv, G, D)
        kc[i].index_copy_(2, cur_t, ref.rope_at(k, cur_t, THETA)[:, :, None])
        vc[i].index_copy_(2, cur_t, v[:, :, None])
        scores = ops.matmul(qr.contiguous(), kc[i].transpose(-1, -2)) * scale
        scores = scores.masked_fill(dead, float("-inf"))
        p = torch.softmax(scores.float(), dim=-1).to(qkv.dtype)
        return ops.matmul(p, vc[i]).reshape(B, H * D)
    return f


def gqa_mha_fn(B, H, Hkv, D, ke, ve, qkv, cur_t):
    G = H // Hkv
    _, _, v = _views(qkv, B, H, Hkv, D)

    def expand(t):      # [B, Hkv, D] -> [B, H, D], head h <- h // G
        return t[:, :, None].expand(B, Hkv, G, D).reshape(B, H, D)

    def f(i):
        # ops.rope rotates by token % seq_len, not by the device position:
        # the same work and launch as a decode step's rope, other angles
        qk = ops.rope(qkv[:, :(H + Hkv) * D].reshape(B, H + Hkv, D), B,
                      THETA)
        return ops.decode_attention(
            qk[:, :H], ke[i], ve[i], cur_t,
            k_new=expand(qk[:, H:]), v_new=expand(v)).reshape(B, H * D)
    return f


def run_gqa_shape(B, H, Hkv, D, S_max, positions, sweep=False, mha=True):
    for p in positions:
        kc, vc, ke, ve, qkv, cur_t, kpos = make_gqa_case(B, H, Hkv, D,
                                                         S_max, p, mha)
        auto = hip.decode_splits(B * Hkv, S_max, H // Hkv)
        graphs = {}
        graphs["fused"], of = capture(
            gqa_fused_fn(B, H, Hkv, D, kc, vc, qkv, cur_t))
        graphs["composed"], oc = capture(
            gqa_composed_fn(B, H, Hkv, D, kc, vc, qkv, cur_t, kpos))
        if mha:
            graphs["mha"], _ = capture(
                gqa_mha_fn(B, H, Hkv, D, ke, ve, qkv, cur_t))
        diff = (of.float() - oc.float()).abs().max().item()
        r = time_alternating(graphs)
        nb = needed_bytes(B, Hkv, D, p)
        bps = nb / (r["fused"][0] * 1e-6)
        row = {
            "bench": "decode_attn_gqa", "B": B, "H": H, "Hkv": Hkv,
            "G": H // Hkv, "D": D, "S_max": S_max, "pos": p,
            "splits": auto, "needed_kv_bytes": nb,
            "fused_bytes_per_s": round(bps, 0),
            "share_of_hbm_peak": round(bps / HBM_PEAK, 3),
            "max_abs_diff_fused_vs_composed": round(diff, 5),
        }
        for k, v in r.items():
            row[k + "_us"] = round(v[0], 2)
            row[k + "_us_min_max"] = [round(x, 2) for x in v[1:]]
        spread = max(r["fused"][2] - r["fused"][1],
                     r["composed"][2] - r["composed"][1])
        row["fused_beats_composed_by_more_than_spread"] = \
            r["composed"][0] - r["fused"][0] > spread
        print(json.dumps(row), flush=True)
        if not sweep:
            continue
        gs = {s: capture(gqa_fused_fn(B, H, Hkv, D, kc, vc, qkv, cur_t,
                                      s))[0] for s in (1, 2, 4, 8, 16)}
        rs = time_alternating(gs)
        print(json.dumps({
            "bench": "decode_attn_gqa_splits", "B": B, "H": H, "Hkv": Hkv,
            "D": D, "S_max": S_max, "pos": p,
            "fused_us_by_splits": {str(s): round(v[0], 2)
                                   for s, v in rs.items()},
        }), flush=True)


def main_gqa():
    run_gqa_shape(32, 32, 8, 64, 640, (512, 639), sweep=True)  # llama-1b-gqa
    run_gqa_shape(32, 32, 4, 64, 640, (639,), sweep=True)      # G = 8
    run_gqa_shape(32, 16, 4, 128, 640, (639,), sweep=True)
    run_gqa_shape(4, 32, 8, 64, 640, (639,), sweep=True)
    run_gqa_shape(1, 32, 8, 64, 2048, (2047,), sweep=True)
    # the remaining (D, G) the kernel covers, fused against composed only
    run_gqa_shape(32, 16, 16, 64, 640, (639,), mha=False)  # G = 1 + rope
    run_gqa_shape(32, 32, 16, 64, 640, (639,), mha=False)  # G = 2
    run_gqa_shape(32, 16, 16, 128, 640, (639,), mha=False)
    run_gqa_shape(32, 16, 8, 128, 640, (639,), mha=False)
    run_gqa_shape(32, 32, 4, 128, 640, (639,), sweep=True, mha=False)


def main():
    assert torch.cuda.is_available(), "bench_decode_attn needs a GPU"
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "mha"):
        run_shape(32, 16, 64, 640, (512, 639), sweep=True)
        run_shape(32, 8, 128, 640, (639,), sweep=True)
        # smaller batches: where the split over KV has to fill the chip
        run_shape(4, 16, 64, 640, (639,), sweep=True)
        run_shape(1, 16, 64, 2048, (2047,), sweep=True)
    if which in ("all", "gqa"):
        main_gqa()


if __name__ == "__main__":
    main()
