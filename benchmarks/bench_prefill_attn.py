"""Prefill-attention benchmark: ops.prefill_attention (one fused call: rope
of q and the chunk's K rows, cache append, attention over the cache at Hkv
heads) against what the engine's composed path runs for the same chunk,
alternating in one process. Method of bench_decode_attn.py, whose capture
and timing helpers are used as they are: each contender is captured into a
graph of CALLS back-to-back calls, call i on its own K/V cache pair (the
way a prefill walks the layers' caches, and so that nothing sits in the
Infinity Cache), timed with device events over interleaved windows; median
and min-max per contender; outputs compared before anything is timed.

composed, first chunk (p0 == 0): ops.rope x2, two cache slice writes,
repeat_interleave(G).contiguous() of K and V, the training flash forward,
the transpose back. composed, continuation (p0 > 0): ref.rope_at x2, the
slice writes, [B,Hkv,G*T,D] @ K^T over rows 0..p0+T-1, mask, fp32 softmax,
cast, @ V. Without rope (GPT-2) the rope calls drop out.

`python bench_prefill_attn.py calls` prints one JSON line per (shape, p0);
`... whole` runs Generator over a 2048-token prompt of llama-1b-gqa in one
chunk and in chunks of 512, composed and fused alternated. With no argument
both run and the lines are also written to profiles/prefill_attention.json.
`... kv8` compares the fused op on bf16 caches with the same op on MXFP8
caches at the shapes of `calls` and writes profiles/prefill_attention_kv8.json."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench_decode_attn as bd
from tepdist_amd import ops
from tepdist_amd.ops import reference as ref

BF16 = torch.bfloat16
THETA = 10000.0
ROWS = []


def emit(row):
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def make_case(B, T, H, Hkv, D, p0):
    torch.manual_seed(0)
    S = p0 + T
    kc, vc = ([torch.randn(B, Hkv, S, D, dtype=BF16, device="cuda")
               for _ in range(bd.CALLS)] for _ in range(2))
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, dtype=BF16, device="cuda")
    return kc, vc, (qkv[:, :H * D].view(B, T, H, D),
                    qkv[:, H * D:(H + Hkv) * D].view(B, T, Hkv, D),
                    qkv[:, (H + Hkv) * D:].view(B, T, Hkv, D))


def fused_fn(kc, vc, qkv, p0, theta):
    q, k, v = qkv
    pos = torch.full((1,), p0, dtype=torch.long, device="cuda")
    return lambda i: ops.prefill_attention(q, kc[i], vc[i], pos, k_new=k,
                                           v_new=v, rope_theta=theta)


def composed_fn(kc, vc, qkv, p0, theta):
    q, k, v = qkv
    B, T, H, D = q.shape
    Hkv = k.shape[2]
    G = H // Hkv
    qpos = torch.arange(p0, p0 + T, device="cuda")
    dead = torch.arange(p0 + T, device="cuda")[None, :] > qpos[:, None]

    def f(i):
        qr, kr = q, k
        if theta is not None and p0 == 0:
            qr = ops.rope(q.reshape(B * T, H, D), T, theta)
            kr = ops.rope(k.reshape(B * T, Hkv, D), T, theta)
        elif theta is not None:
            qr = ref.rope_at(q, qpos[:, None], theta)
            kr = ref.rope_at(k, qpos[:, None], theta)
        qh = qr.reshape(B, T, H, D).transpose(1, 2)
        kh = kr.reshape(B, T, Hkv, D).transpose(1, 2)
        vh = v.transpose(1, 2)
        kc[i][:, :, p0:p0 + T] = kh
        vc[i][:, :, p0:p0 + T] = vh
        if p0 == 0:
            a = ops.attention(qh.contiguous(),
                              kh.repeat_interleave(G, dim=1).contiguous(),
                              vh.repeat_interleave(G, dim=1).contiguous(),
                              causal=True)
        else:
            q4 = qh.reshape(B, Hkv, G * T, D)
            s = ops.matmul(q4.contiguous(), kc[i].transpose(-1, -2)) \
                * (1.0 / math.sqrt(D))
            s = s.view(B, Hkv, G, T, p0 + T).masked_fill(
                dead, float("-inf")).view(B, Hkv, G * T, p0 + T)
            p = torch.softmax(s.float(), dim=-1).to(BF16)
            a = ops.matmul(p, vc[i].contiguous()).reshape(B, H, T, D)
        return a.transpose(1, 2).reshape(B, T, H * D)
    return f


def run_shape(role, B, T, H, Hkv, D, p0s, theta=THETA):
    G = H // Hkv
    for p0 in p0s:
        kc, vc, qkv = make_case(B, T, H, Hkv, D, p0)
        gf, of = bd.capture(fused_fn(kc, vc, qkv, p0, theta))
        gc, oc = bd.capture(composed_fn(kc, vc, qkv, p0, theta))
        diff = (of.reshape(oc.shape).float() - oc.float()).abs().max().item()
        r = bd.time_alternating({"fused": gf, "composed": gc})
        # causal flops of the two products over the visible keys
        flops = 4.0 * B * H * D * (T * p0 + T * (T + 1) / 2)
        emit({
            "bench": "prefill_attn", "role": role, "B": B, "T": T, "H": H,
            "Hkv": Hkv, "G": G, "D": D, "p0": p0, "rope": theta is not None,
            "blocks": B * Hkv * ((T * G + 127) // 128),
            "fused_us": round(r["fused"][0], 2),
            "fused_us_min_max": [round(x, 2) for x in r["fused"][1:]],
            "composed_us": round(r["composed"][0], 2),
            "composed_us_min_max": [round(x, 2) for x in r["composed"][1:]],
            "speedup": round(r["composed"][0] / r["fused"][0], 2),
            "slowest_fused_beats_fastest_composed":
                r["fused"][2] < r["composed"][1],
            "fused_tflops": round(flops / r["fused"][0] * 1e-6, 1),
            "max_abs_diff_fused_vs_composed": round(diff, 5),
        })


def run_kv8_shape(role, B, T, H, Hkv, D, p0s, theta=THETA):
    """The fused op on bf16 caches against the same op on MXFP8 caches
    (mx.MXCache: the KV8 instantiations of both kernels), same shape and
    p0. A win is the slowest MX window beating the fastest bf16 one."""
    from tepdist_amd.ops import mx
    for p0 in p0s:
        kc, vc, qkv = make_case(B, T, H, Hkv, D, p0)
        km, vm = ([mx.MXCache(w.codes.view(t.shape),
                              w.scales.view(*t.shape[:3], D // 32))
                   for t in cs
                   for w in [mx.mx_quantize(t.reshape(-1, D), "mxfp8")]]
                  for cs in (kc, vc))
        r = bd.time_alternating({
            "bf16": bd.capture(fused_fn(kc, vc, qkv, p0, theta))[0],
            "mxfp8": bd.capture(fused_fn(km, vm, qkv, p0, theta))[0]})
        row = {"bench": "prefill_attn_kv8", "role": role, "B": B, "T": T,
               "H": H, "Hkv": Hkv, "G": H // Hkv, "D": D, "p0": p0,
               "rope": theta is not None,
               "blocks": B * Hkv * ((T * (H // Hkv) + 127) // 128),
               "kv_bytes_bf16": 2 * B * Hkv * (p0 + T) * D * 2,
               "kv_bytes_mxfp8": 2 * B * Hkv * (p0 + T) * (D + D // 32),
               "speedup": round(r["bf16"][0] / r["mxfp8"][0], 3),
               "verdict": "win" if r["mxfp8"][2] < r["bf16"][1] else
               "loss" if r["mxfp8"][1] > r["bf16"][2] else "tie"}
        for name, t in r.items():
            row[name + "_us"] = round(t[0], 2)
            row[name + "_us_min_max"] = [round(x, 2) for x in t[1:]]
        emit(row)


def main_calls(run_shape=run_shape):
    run_shape("llama-1b-gqa chunk", 4, 512, 32, 8, 64, (0, 512, 1536))
    run_shape("verify-shaped step", 32, 8, 32, 8, 64, (512,))
    run_shape("llama-1b", 4, 512, 16, 16, 128, (0, 1536))
    run_shape("gpt2-345m", 4, 512, 16, 16, 64, (0, 512), theta=None)
    # the other group sizes, and a grid far below the 256 CUs over a long
    # cache (32 blocks: where a KV split would have to fill the chip)
    run_shape("G = 8", 4, 512, 32, 4, 64, (512,))
    run_shape("G = 2, D = 128", 4, 512, 32, 16, 128, (512,))
    run_shape("small grid", 1, 128, 32, 8, 64, (0, 1920))


def main_whole(B=4, S0=2048, rounds=3):
    from tepdist_amd.inference import Generator
    from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama
    cfg = LLAMA_CONFIGS["llama-1b-gqa"]
    torch.manual_seed(0)
    m = Llama(cfg, dtype=BF16).cuda().eval()
    ids = torch.randint(0, cfg.vocab_size, (B, S0), device="cuda")
    gens = {h: Generator(m, prefill_attn=h) for h in ("composed", "fused")}
    for chunk in (None, 512):
        toks = {h: g.generate(ids, 1, prefill_chunk=chunk)   # also warms up
                for h, g in gens.items()}
        t = {h: [] for h in gens}
        for _ in range(rounds):
            for h, g in gens.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.generate(ids, 1, prefill_chunk=chunk)
                torch.cuda.synchronize()
                t[h].append((time.perf_counter() - t0) * 1e3)
        emit({
            "bench": "prefill_whole", "model": cfg.name, "B": B,
            "prompt": S0, "prefill_chunk": chunk,
            "same_first_token": bool(torch.equal(toks["fused"],
                                                 toks["composed"])),
            **{h + "_ms": round(statistics.median(v), 2)
               for h, v in t.items()},
            **{h + "_ms_min_max": [round(min(v), 2), round(max(v), 2)]
               for h, v in t.items()},
            "slowest_fused_beats_fastest_composed":
                max(t["fused"]) < min(t["composed"]),
        })


def main():
    assert torch.cuda.is_available(), "bench_prefill_attn needs a GPU"
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "calls"):
        main_calls()
    if which in ("all", "whole"):
        main_whole()
    if which == "kv8":
        main_calls(run_kv8_shape)
        with open(os.path.join(ROOT, "profiles",
                               "prefill_attention_kv8.json"), "w") as f:
            json.dump(ROWS, f, indent=1)
    if which == "all":
        with open(os.path.join(ROOT, "profiles", "prefill_attention.json"),
                  "w") as f:
            json.dump(ROWS, f, indent=1)


if __name__ == "__main__":
    main()
