"""Serving-path benchmark: prefill + decode throughput of the KV-cache
generation engine (inference/engine.py) on one GPU. Prints one JSON line
per run: prefill tokens/s and steady-state decode tokens/s, with the
decode-attention mode in use (TEPDIST_DECODE_ATTN=fused|composed|auto).

    bench_decode.py [config] [mode ...]

config is a GPT-2 or Llama config name (e.g. gpt2-345m, llama-1b-gqa).
With modes given (e.g. `fused composed fused composed`) the model is built
once and the modes are measured in that order in this process, which is how
to compare them: alternating, in one GPU visit."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd.inference.engine import Generator
from tepdist_amd.models import GPT2, GPT2_CONFIGS
from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama


def build_model(name):
    torch.manual_seed(0)
    if name in LLAMA_CONFIGS:
        cfg = LLAMA_CONFIGS[name]
        m = Llama(cfg, dtype=torch.bfloat16).cuda()   # initialised by init
    else:
        cfg = GPT2_CONFIGS[name]
        m = GPT2(cfg, dtype=torch.bfloat16).cuda()
        m.reset_parameters()
    return cfg, m.eval()


def measure(cfg, m, name, mode=None, batch=32, prompt=512, new=128):
    g = Generator(m, decode_attn=mode)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (batch, prompt),
                        generator=gen).cuda()
    with torch.no_grad():
        g.generate(ids, 8)                      # warmup (autotune etc.)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = g.generate(ids, new)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # split prefill vs decode: time a prefill-only call (1 new token)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        g.generate(ids, 1)
        torch.cuda.synchronize()
        pre = time.perf_counter() - t1
    n_new = int(out.shape[1] - prompt)
    dec = (batch * (n_new - 1)) / max(dt - pre, 1e-9)
    print(json.dumps({
        "bench": "decode", "config": name, "batch": batch,
        "prompt": prompt, "new_tokens": n_new, "dtype": "bf16",
        "decode_attn": g.decode_attn,
        "decode_attn_fused": g._fused_decode(
            out.new_empty(0, dtype=torch.bfloat16),
            cfg.n_embd // cfg.n_head, cfg.n_head // g.kv_heads),
        "prefill_tokens_per_s": round(batch * prompt / pre, 1),
        "decode_tokens_per_s": round(dec, 1),
        "total_s": round(dt, 3)}), flush=True)
    return out


def main(name="gpt2-345m", *modes):
    cfg, m = build_model(name)
    for mode in modes or (None,):
        measure(cfg, m, name, mode)


if __name__ == "__main__":
    main(*sys.argv[1:])
