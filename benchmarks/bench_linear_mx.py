"""Tiled MX linear microbenchmark: ops.linear_mx (csrc/mx_gemm.hip) against
the dequantize-then-GEMM path the engine runs without it, at the flagship
sites and M = 128 .. 4096, by the method of bench_linear_decode.py --mx
(whose capture / window helpers it uses).

Contenders per (site, M, format):
  "dequant"  ops.mx_dequantize into one scratch buffer + ops.linear, plus
             the residual add / swiglu launches the engine issues: the
             yardstick (mx_linear="dequant");
  "fused"    ops.linear_mx with the tile the plan picks (for the SwiGLU site
             two calls + ops.swiglu, as the engine does);
  "other"    the same with the other tile, at M <= 512 only, so that the
             plan's tile rule is measured;
  "floor"    ops.linear on a weight dequantized beforehand: what "dequant"
             cannot go below. For information.
Each contender is a hipGraph of `sets` back-to-back calls, call i on its own
copy of the weight, sets * its weight bytes >= 512 MiB; median (min-max) of
WINDOWS interleaved windows of REPLAYS replays. `wins`: the slowest "fused"
window beats the fastest "dequant" window.

    bench_linear_mx.py [out.json] [--sites qkv,o] [--ms 128,512]

--act mxfp8: the MXFP8-activation model instead (ops.linear_mx_a8, csrc/
mx_gemm_a8.hip), same sites, M and method. Contenders:
  "quant_a8" ops.mx_quantize_act + ops.linear_mx_a8 (the SwiGLU site: one
             quantization, two calls, ops.swiglu), as the engine runs it;
  "a8"       ops.linear_mx_a8 on x quantized beforehand: the GEMM alone;
  "library"  the same model on the library: ops.mx_quantize_act(roundtrip) +
             ops.mx_dequantize + ops.linear and the engine's tail launches;
  "w_fused", "w_dequant"  from M = 2048, for information: the weight-only
             paths on bf16 x (ops.linear_mx; dequantize + ops.linear), a
             different model.
`wins`: the slowest "quant_a8" window beats the fastest "library" window.

--act mxfp4: the W4A4 model (mxfp4 weights only; ops.linear_mx_a8 on mxfp4
activations, the e2m1 x e2m1 instantiations), same sites, M and method, to
profiles/linear_mx_a4.json. Contenders, all in the same windows:
  "quant_a4" ops.mx_quantize_act(fmt="mxfp4") + ops.linear_mx_a8, as the
             engine runs it;  "a4": the GEMM alone on x quantized beforehand;
  "quant_a8", "a8"  the W4A8 pair above on the same weights (another model,
             for speed only);
  "library"  the W4A4 model on the library: the mxfp4 round trip +
             ops.mx_dequantize + ops.linear and the engine's tail launches.
`wins`: the slowest "quant_a4" window beats the fastest "library" window;
`beats_a8`: it beats the fastest "quant_a8" window.

--mlp: Llama's whole MLP under MX activations (llama-1b-gqa: I 6144, d 2048),
M as above, the three (weight, activation) format pairs, to
profiles/mlp_mx_a8.json. Contenders, all in the same windows:
  "composed" ops.mx_quantize_act + two ops.linear_mx_a8 + ops.swiglu + the
             down call with its own quantizer and the residual, as the engine
             runs it under mx_mlp="composed";
  "fused"    ops.mx_quantize_act + ops.linear_mx_a8(act="swiglu", up=,
             out_format=) (csrc/mx_swiglu_a8.hip) writing MX + the down GEMM
             on those codes: mx_mlp="fused";
  "gate_up_composed", "gate_up_fused"  the part between the first quantizer
             and the down GEMM alone, on x quantized beforehand: two GEMMs +
             ops.swiglu + the quantizer of h, against the one fused launch.
`wins`: the slowest "fused" window beats the fastest "composed" window;
`gate_up_wins`: the same for the gate/up part."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from bench_linear_decode import BF16, COLD_BYTES, SITES, WINDOWS, capture, \
    window_us
from tepdist_amd import ops
from tepdist_amd.ops import hip, mx

MS = (128, 256, 512, 1024, 2048, 4096)


def run_site(model, site, N, K, form, ms):
    torch.manual_seed(0)
    nmat = 2 if form == "swiglu" else 1
    w = [torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
         for _ in range(nmat)]
    b = torch.randn(N, dtype=BF16, device="cuda")
    scratch = torch.empty(N, K, dtype=BF16, device="cuda")
    rows = []
    for fmt in mx.FORMATS:
        q = [ops.mx_quantize(t, fmt) for t in w]
        dq = [ops.mx_dequantize(m) for m in q]
        nbytes = {"mx": nmat * q[0].nbytes, "bf16": nmat * N * K * 2}
        sets = {k: max(4, -(-COLD_BYTES // v)) for k, v in nbytes.items()}
        qs = [[mx.MXWeight(m.codes.clone(), m.scales.clone(), m.fmt, m.shape)
               for _ in range(sets["mx"])] for m in q]
        ds = [[t.clone() for _ in range(sets["bf16"])] for t in dq]
        for M in ms:
            x = torch.randn(M, K, dtype=BF16, device="cuda")
            r = torch.randn(M, N, dtype=BF16, device="cuda")
            bias = b if "bias" in form else None
            res = r if "res" in form else None
            act = "gelu" if form == "bias_gelu" else "none"
            epi = hip.skinny_epi(bias, act, res)

            def tail(ys):
                if nmat == 2:
                    return ops.swiglu(ys[0], ys[1])
                return ys[0] if res is None else res + ys[0]

            def dequant(i):
                return tail([ops.linear(x, ops.mx_dequantize(a[i],
                                                             out=scratch),
                                        bias, act) for a in qs])

            def floor(i):
                return tail([ops.linear(x, a[i], bias, act) for a in ds])

            def fused(tile):
                if nmat == 2:
                    return lambda i: ops.swiglu(*(hip._mx_gemm_raw(
                        x, a[i], None, None, 0, tile) for a in qs))
                return lambda i: hip._mx_gemm_raw(x, qs[0][i], bias, res,
                                                  epi, tile)

            tile = hip.ext.mx_gemm_plan(
                M, N, K, mx.bits(fmt), q[0].codes.stride(0),
                q[0].scales.stride(0))[0]
            fns = {"dequant": (dequant, sets["mx"]),
                   "fused": (fused(tile), sets["mx"]),
                   "floor": (floor, sets["bf16"])}
            if M <= 512:
                fns["other"] = (fused(64 if tile == 128 else 128), sets["mx"])
            graphs, outs = {}, {}
            for name, (fn, n) in fns.items():
                graphs[name], outs[name] = capture(fn, n)
            t = {k: [] for k in graphs}
            for _ in range(WINDOWS):
                for k, g in graphs.items():
                    t[k].append(window_us(g, fns[k][1]))
            row = {"bench": "linear_mx", "model": model, "site": site,
                   "form": form, "fmt": fmt, "M": M, "N": N, "K": K,
                   "tile": tile, "sets": sets, "weight_bytes": nbytes}
            for k, v in t.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            row["wins"] = max(t["fused"]) < min(t["dequant"])
            if "other" in t:
                row["other_tile_wins"] = max(t["other"]) < min(t["fused"])
            row["fused_tflops"] = round(
                nmat * 2.0 * M * N * K / (row["fused_us"] * 1e-6) / 1e12, 1)
            row["max_abs_diff_vs_dequant"] = round(
                (outs["fused"].float() - outs["dequant"].float())
                .abs().max().item(), 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del graphs, outs
        del qs, ds
        torch.cuda.empty_cache()
    return rows


def run_site_a8(model, site, N, K, form, ms):
    torch.manual_seed(0)
    nmat = 2 if form == "swiglu" else 1
    w = [torch.randn(N, K, dtype=BF16, device="cuda") * K ** -0.5
         for _ in range(nmat)]
    b = torch.randn(N, dtype=BF16, device="cuda")
    scratch = torch.empty(N, K, dtype=BF16, device="cuda")
    rows = []
    for fmt in mx.FORMATS:
        q = [ops.mx_quantize(t, fmt) for t in w]
        nbytes = nmat * q[0].nbytes
        sets = max(4, -(-COLD_BYTES // nbytes))
        qs = [[mx.MXWeight(m.codes.clone(), m.scales.clone(), m.fmt, m.shape)
               for _ in range(sets)] for m in q]
        for M in ms:
            x = torch.randn(M, K, dtype=BF16, device="cuda")
            r = torch.randn(M, N, dtype=BF16, device="cuda")
            xq, xr = ops.mx_quantize_act(x), torch.empty_like(x)
            bias = b if "bias" in form else None
            res = r if "res" in form else None
            act = "gelu" if form == "bias_gelu" else "none"
            epi = hip.skinny_epi(bias, act, res)

            def tail(ys):
                if nmat == 2:
                    return ops.swiglu(ys[0], ys[1])
                return ys[0] if res is None else res + ys[0]

            def a8(xin, i):
                if nmat == 2:
                    return ops.swiglu(*(hip._mx_gemm_a8_raw(
                        xin, a[i], None, None, 0) for a in qs))
                return hip._mx_gemm_a8_raw(xin, qs[0][i], bias, res, epi)

            fns = {
                "quant_a8": lambda i: a8(ops.mx_quantize_act(x, out=xq), i),
                "a8": lambda i: a8(xq, i),
                "library": lambda i: tail([ops.linear(
                    ops.mx_quantize_act(x, roundtrip=True, out=xr),
                    ops.mx_dequantize(a[i], out=scratch), bias, act)
                    for a in qs]),
            }
            if M >= 2048:
                fns["w_fused"] = lambda i: ops.swiglu(*(hip._mx_gemm_raw(
                    x, a[i], None, None, 0) for a in qs)) if nmat == 2 \
                    else hip._mx_gemm_raw(x, qs[0][i], bias, res, epi)
                fns["w_dequant"] = lambda i: tail([ops.linear(
                    x, ops.mx_dequantize(a[i], out=scratch), bias, act)
                    for a in qs])
            graphs, outs = {}, {}
            for name, fn in fns.items():
                graphs[name], outs[name] = capture(fn, sets)
            t = {k: [] for k in graphs}
            for _ in range(WINDOWS):
                for k, g in graphs.items():
                    t[k].append(window_us(g, sets))
            tile = hip.ext.mx_gemm_a8_plan(
                M, N, K, mx.bits(fmt), q[0].codes.stride(0),
                q[0].scales.stride(0), K, K // 32)[0]
            row = {"bench": "linear_mx_a8", "model": model, "site": site,
                   "form": form, "fmt": fmt, "M": M, "N": N, "K": K,
                   "tile": tile, "sets": sets, "weight_bytes": nbytes}
            for k, v in t.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            row["wins"] = max(t["quant_a8"]) < min(t["library"])
            row["a8_tflops"] = round(
                nmat * 2.0 * M * N * K / (row["a8_us"] * 1e-6) / 1e12, 1)
            row["max_abs_diff_vs_library"] = round(
                (outs["quant_a8"].float() - outs["library"].float())
                .abs().max().item(), 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del graphs, outs
        del qs
        torch.cuda.empty_cache()
    return rows


def run_site_a4(model, site, N, K, form, ms):
    torch.manual_seed(0)
    nmat = 2 if form == "swiglu" else 1
    q = [ops.mx_quantize(torch.randn(N, K, dtype=BF16, device="cuda")
                         * K ** -0.5, "mxfp4") for _ in range(nmat)]
    b = torch.randn(N, dtype=BF16, device="cuda")
    scratch = torch.empty(N, K, dtype=BF16, device="cuda")
    nbytes = nmat * q[0].nbytes
    sets = max(4, -(-COLD_BYTES // nbytes))
    qs = [[mx.MXWeight(m.codes.clone(), m.scales.clone(), m.fmt, m.shape)
           for _ in range(sets)] for m in q]
    rows = []
    for M in ms:
        x = torch.randn(M, K, dtype=BF16, device="cuda")
        r = torch.randn(M, N, dtype=BF16, device="cuda")
        xq = {f: ops.mx_quantize_act(x, fmt=f) for f in mx.FORMATS}
        xr = torch.empty_like(x)
        bias = b if "bias" in form else None
        res = r if "res" in form else None
        act = "gelu" if form == "bias_gelu" else "none"
        epi = hip.skinny_epi(bias, act, res)

        def tail(ys):
            if nmat == 2:
                return ops.swiglu(ys[0], ys[1])
            return ys[0] if res is None else res + ys[0]

        def gemm(xin, i):
            if nmat == 2:
                return ops.swiglu(*(hip._mx_gemm_a8_raw(
                    xin, a[i], None, None, 0) for a in qs))
            return hip._mx_gemm_a8_raw(xin, qs[0][i], bias, res, epi)

        def quant(f):
            return lambda i: gemm(ops.mx_quantize_act(x, out=xq[f], fmt=f), i)

        fns = {
            "quant_a4": quant("mxfp4"), "a4": lambda i: gemm(xq["mxfp4"], i),
            "quant_a8": quant("mxfp8"), "a8": lambda i: gemm(xq["mxfp8"], i),
            "library": lambda i: tail([ops.linear(
                ops.mx_quantize_act(x, roundtrip=True, out=xr, fmt="mxfp4"),
                ops.mx_dequantize(a[i], out=scratch), bias, act)
                for a in qs]),
        }
        graphs, outs = {}, {}
        for name, fn in fns.items():
            graphs[name], outs[name] = capture(fn, sets)
        t = {k: [] for k in graphs}
        for _ in range(WINDOWS):
            for k, g in graphs.items():
                t[k].append(window_us(g, sets))
        tile = hip.ext.mx_gemm_a8_plan(M, N, K, 4, K // 2, K // 32, K // 2,
                                       K // 32, 0, 0, 4)[0]
        row = {"bench": "linear_mx_a4", "model": model, "site": site,
               "form": form, "fmt": "mxfp4", "M": M, "N": N, "K": K,
               "tile": tile, "sets": sets, "weight_bytes": nbytes}
        for k, v in t.items():
            row[f"{k}_us"] = round(statistics.median(v), 2)
            row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        row["wins"] = max(t["quant_a4"]) < min(t["library"])
        row["beats_a8"] = max(t["quant_a4"]) < min(t["quant_a8"])
        for k in ("a4", "a8"):
            row[f"{k}_tflops"] = round(
                nmat * 2.0 * M * N * K / (row[f"{k}_us"] * 1e-6) / 1e12, 1)
        row["max_abs_diff_vs_library"] = round(
            (outs["quant_a4"].float() - outs["library"].float())
            .abs().max().item(), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del graphs, outs
    return rows


def run_mlp(ms, model="llama-1b-gqa", I=6144, d=2048):
    torch.manual_seed(0)
    wg, wu = (torch.randn(I, d, dtype=BF16, device="cuda") * d ** -0.5
              for _ in range(2))
    wd = torch.randn(d, I, dtype=BF16, device="cuda") * I ** -0.5
    rows = []
    for wfmt, xfmt in (("mxfp4", "mxfp8"), ("mxfp8", "mxfp8"),
                       ("mxfp4", "mxfp4")):
        q = [ops.mx_quantize(t, wfmt) for t in (wg, wu, wd)]
        nbytes = sum(m.nbytes for m in q)
        sets = max(4, -(-COLD_BYTES // nbytes))
        g, u, dn = ([mx.MXWeight(m.codes.clone(), m.scales.clone(), m.fmt,
                                 m.shape) for _ in range(sets)] for m in q)
        for M in ms:
            x = torch.randn(M, d, dtype=BF16, device="cuda")
            xq = ops.mx_quantize_act(x, fmt=xfmt)

            def gate_up(xin, i):
                return ops.swiglu(ops.linear_mx_a8(xin, g[i]),
                                  ops.linear_mx_a8(xin, u[i]))

            def fused_gate_up(xin, i):
                return ops.linear_mx_a8(xin, g[i], act="swiglu", up=u[i],
                                        out_format=xfmt)

            def quant():
                return ops.mx_quantize_act(x, out=xq, fmt=xfmt)

            fns = {
                "composed": lambda i: ops.linear_mx_a8(
                    gate_up(quant(), i), dn[i], residual=x, act_format=xfmt),
                "fused": lambda i: ops.linear_mx_a8(
                    fused_gate_up(quant(), i), dn[i], residual=x),
                "gate_up_composed": lambda i: ops.mx_quantize_act(
                    gate_up(xq, i), fmt=xfmt).codes,
                "gate_up_fused": lambda i: fused_gate_up(xq, i).codes,
            }
            graphs, outs = {}, {}
            for name, fn in fns.items():
                graphs[name], outs[name] = capture(fn, sets)
            t = {k: [] for k in graphs}
            for _ in range(WINDOWS):
                for k, gr in graphs.items():
                    t[k].append(window_us(gr, sets))
            wb, ldc, lds = mx.bits(wfmt), q[0].codes.stride(0), d // 32
            tile = hip.ext.mx_swiglu_a8_plan(
                M, I, d, wb, ldc, lds, I, d, wb, ldc, lds, xq.codes.stride(0),
                d // 32, 0, 0, mx.bits(xfmt), mx.bits(xfmt),
                I * mx.bits(xfmt) // 8, I // 32)[0]
            row = {"bench": "mlp_mx_a8", "model": model, "fmt": wfmt,
                   "act": xfmt, "M": M, "I": I, "d": d, "tile": tile,
                   "sets": sets, "weight_bytes": nbytes}
            for k, v in t.items():
                row[f"{k}_us"] = round(statistics.median(v), 2)
                row[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            row["wins"] = max(t["fused"]) < min(t["composed"])
            row["gate_up_wins"] = \
                max(t["gate_up_fused"]) < min(t["gate_up_composed"])
            row["gate_up_fused_tflops"] = round(
                4.0 * M * I * d / (row["gate_up_fused_us"] * 1e-6) / 1e12, 1)
            row["max_abs_diff_vs_composed"] = round(
                (outs["fused"].float() - outs["composed"].float())
                .abs().max().item(), 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del graphs, outs
        del g, u, dn
        torch.cuda.empty_cache()
    return rows


def main(*argv):
    def opt(name, default):
        return argv[argv.index(name) + 1].split(",") if name in argv \
            else default

    sites = opt("--sites", None)
    ms = tuple(int(m) for m in opt("--ms", MS))
    act = opt("--act", ["bf16"])[0]
    if act not in ("bf16", "mxfp8", "mxfp4"):
        raise SystemExit(f"--act must be bf16, mxfp8 or mxfp4, got {act!r}")
    run = {"bf16": run_site, "mxfp8": run_site_a8, "mxfp4": run_site_a4}[act]
    skip = {a for n in ("--sites", "--ms", "--act") if n in argv
            for a in (n, argv[argv.index(n) + 1])} | {"--mlp"}
    out = next((a for a in argv if a not in skip), None)
    rows = run_mlp(ms) if "--mlp" in argv else []
    for s in SITES:
        if "--mlp" not in argv and (sites is None or s[1] in sites):
            rows += run(*s, ms)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:])
