"""Decode-step linear microbenchmark: the skinny weight-streaming kernel
(ops.linear_decode / ops.swiglu_linear_decode) against what a site runs
without it, alternating in one process, by the method of
bench_decode_attn.py.

Contenders per site: "skinny" (one launch, epilogue fused), "lib" (F.linear
= hipBLASLt, plus the separate residual add / gelu / swiglu launches the
fused epilogue replaces) and "hand" (the 128-tile hand GEMM with its own
bias/gelu epilogue, plus the same separate launches).

Each contender is captured into a hipGraph of `sets` back-to-back calls,
call i on its own copy of the weights, with sets * weight bytes >= 512 MiB
(5 sets for the heads, 256 for gpt2-345m's proj) so the weights do not sit
in the 256 MiB Infinity Cache; timed with device
events over REPLAYS replays per window, WINDOWS windows per contender,
interleaved. One JSON line per (site, M): median and min-max per contender,
the needed weight bytes per skinny call time, and `wins`: whether the
slowest skinny window beats the fastest window of both others.

    bench_linear_decode.py [out.json]

With --mx the contenders are the MX weight formats (ops.linear_decode_mx /
ops.swiglu_linear_decode_mx on "mxfp8" and "mxfp4" weights) against the bf16
skinny kernel and the library, on the same sites, windows and interleaving.
Every contender gets its own number of weight copies by the same rule, sets
* its weight bytes >= 512 MiB, so the smaller formats are not measured out
of the Infinity Cache. `wins[fmt]`: the slowest window of the format beats
the fastest bf16 skinny window. `max_abs_diff_vs_bf16_on_dq[fmt]`: against the
bf16 skinny kernel on the dequantized weight (the same sum in another order).

    bench_linear_decode.py --mx [out.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from tepdist_amd import ops
from tepdist_amd.ops import hip

BF16 = torch.bfloat16
REPLAYS, WINDOWS = 5, 5
COLD_BYTES = 512 << 20
MS = (1, 8, 32, 64)

# (model, site, N, K, form)
SITES = [
    ("llama-1b-gqa", "qkv", 3072, 2048, "plain"),
    ("llama-1b-gqa", "o", 2048, 2048, "res"),
    ("llama-1b-gqa", "gate_up", 6144, 2048, "swiglu"),
    ("llama-1b-gqa", "down", 2048, 6144, "res"),
    ("llama-1b-gqa", "head", 32000, 2048, "plain"),
    ("gpt2-345m", "qkv", 3072, 1024, "bias"),
    ("gpt2-345m", "proj", 1024, 1024, "bias_res"),
    ("gpt2-345m", "fc", 4096, 1024, "bias_gelu"),
    ("gpt2-345m", "out", 1024, 4096, "bias_res"),
    ("gpt2-345m", "head", 50304, 1024, "plain"),
]


def contenders(form, x, ws, ws2, b, r):
    """{name: fn(i)} for one site; ws/ws2: per-call weight copies."""
    M, K = x.shape
    N = ws[0].shape[0]
    bias = b if "bias" in form else None
    res = r if "res" in form else None
    act = "gelu" if form == "bias_gelu" else "none"

    def hand_mm(w, bias=None, epi=0):
        return hip._gemm_raw(x, w, True, True, M, N, K, K, K, 0, 0, 1,
                             bias=bias, epi=epi)[0]

    if form == "swiglu":
        return {
            "skinny": lambda i: ops.swiglu_linear_decode(x, ws[i], ws2[i]),
            "lib": lambda i: ops.swiglu(F.linear(x, ws[i]),
                                        F.linear(x, ws2[i])),
            "hand": lambda i: ops.swiglu(hand_mm(ws[i]), hand_mm(ws2[i])),
        }

    def tail(y):
        return y if res is None else res + y

    def lib(i):
        y = F.linear(x, ws[i], bias)
        return tail(ops.gelu(y) if act == "gelu" else y)

    epi = 2 if act == "gelu" else 1 if bias is not None else 0
    return {
        "skinny": lambda i: ops.linear_decode(x, ws[i], bias, act, res),
        "lib": lib,
        "hand": lambda i: tail(hand_mm(ws[i], bias, epi)),
    }


def capture(fn, sets):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            fn(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        for i in range(sets):
            out = fn(i)
    graph.replay()
    torch.cuda.synchronize()
    return graph, out


def window_us(graph, sets):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * sets)


def run_site(model, site, N, K, form):
    torch.manual_seed(0)
    nmat = 2 if form == "swiglu" else 1
    wbytes = nmat * N * K * 2
    sets = max(4, -(-COLD_BYTES // wbytes))
    ws = [torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
          for _ in range(sets)]
    ws2 = [torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
           for _ in range(sets)] if nmat == 2 else None
    b = torch.randn(N, dtype=BF16, device="cuda")
    rows = []
    for M in MS:
        x = torch.randn(M, K, dtype=BF16, device="cuda")
        r = torch.randn(M, N, dtype=BF16, device="cuda")
        fns = contenders(form, x, ws, ws2, b, r)
        graphs, outs = {}, {}
        for name, fn in fns.items():
            graphs[name], outs[name] = capture(fn, sets)
        t = {k: [] for k in graphs}
        for _ in range(WINDOWS):
            for k, g in graphs.items():
                t[k].append(window_us(g, sets))
        row = {"bench": "linear_decode", "model": model, "site": site,
               "form": form, "M": M, "N": N, "K": K, "sets": sets,
               "plan": list(hip.ext.skinny_plan(M, N, K, K, K, 0,
                                                nmat == 2)[:4])}
        for k, v in t.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        row["weight_bytes"] = wbytes
        row["skinny_weight_bytes_per_s"] = round(
            wbytes / (row["skinny_us"] * 1e-6))
        row["wins"] = max(t["skinny"]) < min(min(t["lib"]), min(t["hand"]))
        row["max_abs_diff_vs_lib"] = round(
            (outs["skinny"].float() - outs["lib"].float()).abs().max().item(),
            4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def run_site_mx(model, site, N, K, form):
    from tepdist_amd.ops import mx
    torch.manual_seed(0)
    nmat = 2 if form == "swiglu" else 1
    w = torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
    w2 = torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
    q = {f: (ops.mx_quantize(w, f), ops.mx_quantize(w2, f))
         for f in mx.FORMATS}
    wbytes = {"bf16": nmat * N * K * 2}
    wbytes.update({f: nmat * q[f][0].nbytes for f in mx.FORMATS})
    sets = {f: max(4, -(-COLD_BYTES // nb)) for f, nb in wbytes.items()}

    def copies(m, n):
        return [mx.MXWeight(m.codes.clone(), m.scales.clone(), m.fmt, m.shape)
                for _ in range(n)]

    ws = [w.clone() for _ in range(sets["bf16"])]
    ws2 = [w2.clone() for _ in range(sets["bf16"])] if nmat == 2 else None
    qs = {f: (copies(q[f][0], sets[f]),
              copies(q[f][1], sets[f]) if nmat == 2 else None)
          for f in mx.FORMATS}
    b = torch.randn(N, dtype=BF16, device="cuda")
    rows = []
    for M in MS:
        x = torch.randn(M, K, dtype=BF16, device="cuda")
        r = torch.randn(M, N, dtype=BF16, device="cuda")
        bias = b if "bias" in form else None
        res = r if "res" in form else None
        act = "gelu" if form == "bias_gelu" else "none"
        base = contenders(form, x, ws, ws2, b, r)
        fns = {"skinny": (base["skinny"], sets["bf16"])}
        for f in mx.FORMATS:
            a, a2 = qs[f]
            if nmat == 2:
                fns[f] = (lambda i, a=a, a2=a2:
                          ops.swiglu_linear_decode_mx(x, a[i], a2[i]), sets[f])
            else:
                fns[f] = (lambda i, a=a:
                          ops.linear_decode_mx(x, a[i], bias, act, res),
                          sets[f])
        fns["lib"] = (base["lib"], sets["bf16"])
        graphs, outs = {}, {}
        for name, (fn, n) in fns.items():
            graphs[name], outs[name] = capture(fn, n)
        t = {k: [] for k in graphs}
        for _ in range(WINDOWS):
            for k, g in graphs.items():
                t[k].append(window_us(g, fns[k][1]))
        row = {"bench": "linear_decode_mx", "model": model, "site": site,
               "form": form, "M": M, "N": N, "K": K, "sets": sets,
               "weight_bytes": wbytes, "wins": {}, "max_abs_diff_vs_bf16_on_dq": {},
               "weight_bytes_per_s": {}}
        for k, v in t.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        for f in mx.FORMATS:
            row["wins"][f] = max(t[f]) < min(t["skinny"])
            row["weight_bytes_per_s"][f] = round(
                wbytes[f] / (row[f"{f}_us"] * 1e-6))
            with torch.no_grad():
                dq = [ops.mx_dequantize(m) for m in q[f]]
                want = ops.swiglu_linear_decode(x, dq[0], dq[1]) \
                    if nmat == 2 else \
                    ops.linear_decode(x, dq[0], bias, act, res)
            row["max_abs_diff_vs_bf16_on_dq"][f] = round(
                (outs[f].float() - want.float()).abs().max().item(), 4)
        row["weight_bytes_per_s"]["bf16"] = round(
            wbytes["bf16"] / (row["skinny_us"] * 1e-6))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main(*argv):
    use_mx = "--mx" in argv
    out = next((a for a in argv if not a.startswith("--")), None)
    rows = []
    for s in SITES:
        rows += run_site_mx(*s) if use_mx else run_site(*s)
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:])
