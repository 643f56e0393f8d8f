"""MoE routing microbenchmark: route + dispatch + combine, forward and
backward, with the expert replaced by identity. The fused path
(ops.moe_route / moe_dispatch / moe_combine, ops/csrc/moe_route.hip) against
the composed torch-op sequence of MoELayer.forward, alternating in one
process.

Each variant is captured into a hipGraph holding LAYERS forward+backward
passes, pass i on its own x / gates / dout (the way a model walks its MoE
layers, and so that the working set does not sit in the 256 MiB Infinity
Cache at the bench shape), and timed with device events over REPLAYS
replays per window, WINDOWS windows per variant, fused and composed windows
interleaved; medians and min/max are reported. An eager (uncaptured) host
clock figure per pass is reported as well: it contains the launch overhead
of the composed path's many small ops.

Usage: bench_moe_route.py [bench|small] — one shape per process, so that
the caller can put every timed step under its own time limit. Prints one
JSON line.

The bytes figure is what the fused algorithm needs: with n kept entries,
rows of d bf16, 2*d*(5n + 2*E*C + 3T) bytes over the five row passes (maps
and weights are noise next to it). Row gathers are bound by memory
bandwidth; the figure is to be read against the ~6.3 TB/s a plain copy
reaches on the MI355X."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd import ops

BF16 = torch.bfloat16
LAYERS, REPLAYS, WINDOWS = 8, 10, 7
COPY_BW = 6.3e12
SHAPES = {"bench": (8192, 8, 2, 768, 2560), "small": (2048, 8, 2, 256, 640)}


def composed(x, gates, k, C):
    """The routing of MoELayer.forward (route="composed"), expert = identity."""
    T, d = x.shape
    E = gates.shape[1]
    topv, topi = torch.topk(gates.float(), k, dim=-1)
    topv = topv / topv.sum(-1, keepdim=True).clamp_min(1e-9)
    with torch.no_grad():
        f = torch.zeros(E, device=x.device)
        f.scatter_add_(0, topi.reshape(-1),
                       torch.ones_like(topi.reshape(-1), dtype=torch.float32))
    flat_e = topi.reshape(-1)
    flat_w = topv.reshape(-1)
    flat_t = torch.arange(T, device=x.device).repeat_interleave(k)
    order = torch.argsort(flat_e, stable=True)
    counts = torch.zeros(E, dtype=torch.long, device=x.device).scatter_add_(
        0, flat_e, torch.ones_like(flat_e))
    offs = torch.cumsum(counts, 0) - counts
    r = torch.arange(flat_e.numel(), device=x.device)
    pos = torch.empty_like(r)
    pos[order] = r - offs[flat_e[order]]
    keep = pos < C
    slot = flat_e * C + pos
    slot_safe = torch.where(keep, slot, torch.zeros_like(slot))
    contrib = x[flat_t] * keep.unsqueeze(-1).to(x.dtype)
    D = torch.zeros(E * C, d, dtype=x.dtype, device=x.device)
    D = D.index_put((slot_safe,), contrib, accumulate=True)
    back = D
    gathered = back[slot_safe] * \
        (flat_w * keep.to(flat_w.dtype)).unsqueeze(-1).to(back.dtype)
    return torch.zeros_like(x).index_add(0, flat_t, gathered.to(x.dtype)), f


def fused(x, gates, k, C):
    route = ops.moe_route(gates, k, C)
    w = gates.float().gather(1, route.topi.long())
    w = w / w.sum(-1, keepdim=True).clamp_min(1e-9)
    f = route.counts.float()
    return ops.moe_combine(ops.moe_dispatch(x, route), w, route), f


def make_inputs(T, E, k, d):
    gen = torch.Generator().manual_seed(0)
    sets = []
    for _ in range(LAYERS):
        x = torch.randn(T, d, generator=gen).to(BF16).cuda().requires_grad_()
        logits = torch.randn(T, E, generator=gen).cuda().requires_grad_()
        dout = torch.randn(T, d, generator=gen).to(BF16).cuda()
        sets.append((x, logits, dout))
    return sets


def make_step(fn, sets, k, C):
    def step():
        outs = []
        for x, logits, dout in sets:
            x.grad = None
            logits.grad = None
            gates = torch.softmax(logits, -1).to(BF16)
            out, f = fn(x, gates, k, C)
            out.backward(dout)
            outs.append((out.detach(), x.grad, logits.grad, f))
        return outs
    return step


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    return graph, outs


def window_us(graph):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * LAYERS)


def eager_us(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPLAYS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (REPLAYS * LAYERS)


def stats(v):
    return {"median": round(statistics.median(v), 2),
            "min": round(min(v), 2), "max": round(max(v), 2)}


def main():
    assert torch.cuda.is_available(), "bench_moe_route needs a GPU"
    name = sys.argv[1] if len(sys.argv) > 1 else "bench"
    T, E, k, d, C = SHAPES[name]
    sets = make_inputs(T, E, k, d)
    steps = {"fused": make_step(fused, sets, k, C),
             "composed": make_step(composed, sets, k, C)}
    graphs, outs = {}, {}
    for n, s in steps.items():
        graphs[n], o = capture(s)
        outs[n] = [[t.float().clone() for t in layer] for layer in o]
    diffs = {nm: max((a[i] - b[i]).abs().max().item()
                     for a, b in zip(outs["fused"], outs["composed"]))
             for i, nm in enumerate(("out", "dx", "dlogits", "counts"))}

    t_graph = {n: [] for n in steps}
    t_eager = {n: [] for n in steps}
    for _ in range(WINDOWS):
        for n in steps:
            t_graph[n].append(window_us(graphs[n]))
    for _ in range(WINDOWS):
        for n in steps:
            t_eager[n].append(eager_us(steps[n]))

    with torch.no_grad():
        x, logits, _ = sets[0]
        route = ops.moe_route(torch.softmax(logits, -1).to(BF16), k, C)
        n_kept = int((route.slot >= 0).sum().item())
    nbytes = 2 * d * (5 * n_kept + 2 * E * C + 3 * T)
    fg = statistics.median(t_graph["fused"])
    cg = statistics.median(t_graph["composed"])
    print(json.dumps({
        "bench": "moe_route", "shape": name, "T": T, "E": E, "k": k, "d": d,
        "C": C, "kept_entries": n_kept, "layers_per_graph": LAYERS,
        "graph_us_per_pass": {n: stats(v) for n, v in t_graph.items()},
        "eager_us_per_pass": {n: stats(v) for n, v in t_eager.items()},
        "speedup_graph": round(cg / fg, 2),
        "speedup_eager": round(statistics.median(t_eager["composed"]) /
                               statistics.median(t_eager["fused"]), 2),
        "fused_needed_bytes": nbytes,
        "fused_bytes_per_s": round(nbytes / (fg * 1e-6), 0),
        "share_of_copy_bandwidth": round(nbytes / (fg * 1e-6) / COPY_BW, 3),
        "note": "fused time includes the softmax, gate-weight and autograd "
                "glue ops, not only the kernels",
        "max_abs_diff_fused_vs_composed": diffs,
    }), flush=True)


if __name__ == "__main__":
    main()
