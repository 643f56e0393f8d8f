"""Token-sampling benchmark on one GPU.

    bench_sampling.py [op] [e2e [config ...]]

op   ops.sample_logits per call against the composed torch sequence the
     engine's host sampler runs on the device plus a device multinomial
     (scale, topk, masked fill, softmax, torch.multinomial). The composed
     sequence has no top-p step, so for top_p < 1 its figure is that of
     less work than the op does ("composed_does_top_p": false). Method of
     bench_decode_attn.py: each variant is captured into a hipGraph of
     CALLS back-to-back calls, call i on its own logits buffer, timed with device events over REPLAYS replays per
     window, WINDOWS windows per variant, the variants interleaved. The
     logits buffers are not rewritten between calls, so from the second
     replay on a row comes from wherever CALLS buffers of that size stay
     (L2 / Infinity Cache for the shapes here): as in a decode step, where
     the head GEMM has just written it.
e2e  decode tokens/s of Generator.generate at batch 32 x 512 prompt x 128
     new tokens: greedy, host sampler and device sampler interleaved in one
     process, ROUNDS rounds; median and min/max per mode.

One JSON line per measurement."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tepdist_amd import ops

BF16 = torch.bfloat16
CALLS, REPLAYS, WINDOWS = 16, 10, 5
ROUNDS = 3
T = 0.8


def device_fn(bufs, vocab, top_k, top_p):
    B = bufs[0].shape[0]
    step = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    out = torch.zeros(B, 1, dtype=torch.int64, device="cuda")

    def f(i):
        return ops.sample_logits(bufs[i], temperature=T, top_k=top_k,
                                 top_p=top_p, seed=1, step=step, vocab=vocab,
                                 out=out)
    return f


def composed_fn(bufs, vocab, top_k, top_p):
    def f(i):
        logits = bufs[i][:, :vocab].float() / T
        if top_k > 0:
            kth = logits.topk(top_k, dim=-1).values[:, -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        probs = torch.softmax(logits, dim=-1)
        return torch.multinomial(probs, 1)
    return f


def capture(fn):
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
            fn(i)
    graph.replay()
    torch.cuda.synchronize()
    return graph


def window_us(graph):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * CALLS)


def time_alternating(graphs):
    t = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            t[k].append(window_us(g))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def run_op(B, vocab, stride, dtype):
    torch.manual_seed(0)
    bufs = [(torch.randn(B, stride, device="cuda") * 2.5).to(dtype)
            for _ in range(CALLS)]
    for top_k, top_p in ((50, 1.0), (0, 0.9), (50, 0.9)):
        graphs = {"device": capture(device_fn(bufs, vocab, top_k, top_p))}
        try:
            graphs["composed"] = capture(composed_fn(bufs, vocab, top_k,
                                                     top_p))
        except Exception as e:      # a torch op that cannot be captured
            composed_error = f"{type(e).__name__}: {e}"[:200]
        r = time_alternating(graphs)
        row = {"bench": "sample_logits", "B": B, "vocab": vocab,
               "row_stride": stride,
               "dtype": "bf16" if dtype == BF16 else "fp32",
               "temperature": T, "top_k": top_k, "top_p": top_p,
               "composed_does_top_p": False,
               "calls_per_graph": CALLS, "replays_per_window": REPLAYS,
               "windows": WINDOWS}
        for k, v in r.items():
            row[k + "_us"] = round(v[0], 2)
            row[k + "_us_min_max"] = [round(x, 2) for x in v[1:]]
        if "composed" in r:
            row["speedup"] = round(r["composed"][0] / r["device"][0], 2)
        else:
            row["composed_error"] = composed_error
        print(json.dumps(row), flush=True)


def main_op():
    for dtype in (torch.float32, BF16):
        run_op(32, 50257, 50304, dtype)
        run_op(32, 32000, 32000, dtype)
        run_op(1, 128256, 128256, dtype)


def decode_rate(g, ids, new, **kw):
    """Steady-state decode tokens/s: a full run minus a prefill-only run."""
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = g.generate(ids, new, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        t1 = time.perf_counter()
        g.generate(ids, 1, **kw)
        torch.cuda.synchronize()
        pre = time.perf_counter() - t1
    n_new = int(out.shape[1] - ids.shape[1])
    return ids.shape[0] * (n_new - 1) / max(dt - pre, 1e-9)


def main_e2e(name, batch=32, prompt=512, new=128):
    from bench_decode import build_model
    from tepdist_amd.inference.engine import Generator
    cfg, m = build_model(name)
    g = Generator(m)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (batch, prompt),
                        generator=gen).cuda()
    sampled = dict(temperature=T, top_k=50, top_p=0.9, seed=1)
    modes = {"greedy": {},
             "host": dict(sampler="host", **sampled),
             "device": dict(sampler="device", **sampled)}
    with torch.no_grad():
        for kw in modes.values():
            g.generate(ids, 8, **kw)            # warm-up (autotune etc.)
    rates = {k: [] for k in modes}
    for _ in range(ROUNDS):
        for k, kw in modes.items():
            rates[k].append(decode_rate(g, ids, new, **kw))
    row = {"bench": "decode_sampling", "config": name, "batch": batch,
           "prompt": prompt, "new_tokens": new, "dtype": "bf16",
           "temperature": T, "top_k": 50, "top_p": 0.9, "rounds": ROUNDS}
    for k, v in rates.items():
        row[k + "_tokens_per_s"] = round(statistics.median(v), 1)
        row[k + "_tokens_per_s_min_max"] = [round(min(v), 1),
                                            round(max(v), 1)]
    row["device_over_host"] = round(
        statistics.median(rates["device"]) / statistics.median(rates["host"]),
        2)
    row["device_over_greedy"] = round(
        statistics.median(rates["device"])
        / statistics.median(rates["greedy"]), 3)
    print(json.dumps(row), flush=True)


def main():
    assert torch.cuda.is_available(), "bench_sampling needs a GPU"
    args = sys.argv[1:] or ["op", "e2e"]
    if "op" in args:
        main_op()
    if "e2e" in args:
        names = args[args.index("e2e") + 1:] or ["gpt2-345m", "llama-1b-gqa"]
        for name in names:
            main_e2e(name)


if __name__ == "__main__":
    main()
