"""ops.sample_logits through the HIP kernel (csrc/sampling.hip): the checks
of test_sampling_cpu.py against the same float64 oracle and bound
(sampling_checks.py), the sizes at which the kernel's own structure changes,
repeatability, graph replay and the engine's device sampler."""

import pytest
import torch

import sampling_checks as sc
from tepdist_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
THREADS = 1024            # sampling.hip ST: one 1024-thread workgroup per row


def test_topk_thresholds():
    sc.check_topk_thresholds(DEV)


def test_topp_thresholds():
    sc.check_topp_thresholds(DEV)


def test_no_filter_threshold():
    sc.check_no_filter_threshold(DEV)


@pytest.mark.parametrize("top_k,top_p", [(50, 1.0), (0, 0.9), (0, 1.0)])
def test_cdf_sweep(top_k, top_p):
    sc.check_cdf_sweep(DEV, top_k, top_p)


@pytest.mark.parametrize("V", [1, 7, 64, 503, 4097])
@pytest.mark.parametrize("B", [1, 3])
def test_draws(V, B):
    sc.check_draws(DEV, V, B)


def test_u_ends():
    sc.check_u_ends(DEV)


def test_special_rows():
    sc.check_special_rows(DEV)


def test_views():
    sc.check_views(DEV)


def test_philox():
    sc.check_philox(DEV)


# -- where the kernel's structure changes: one 16-byte group per thread is
# THREADS * 4 fp32 or THREADS * 8 bf16 columns, a wave's share of the row
# and the 64-group steps inside it change around those, and a row end one
# column off a group boundary takes the element loads ---------------------

@pytest.mark.parametrize("V", [THREADS * 4 - 1, THREADS * 4, THREADS * 4 + 1,
                               THREADS * 8 - 1, THREADS * 8 + 1])
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_chunk_edges(V, dtype):
    sc.check_draws(DEV, V, 2, dtype=dtype, configs=((0, 1.0), (50, 0.9)))


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_gpt2_vocab_padded_stride(dtype):
    """[B, 50257] as the engine passes it: the padded head's rows, 50304
    apart, columns past the vocabulary never chosen."""
    g = sc.gen(31)
    pad = sc.logits(g, 4, 50304, dtype=dtype)
    pad[:, 50257:] = 50.0
    u = sc.uniforms(g, 4)
    for top_k, top_p in ((50, 1.0), (0, 0.9), (50, 0.9)):
        sc.check_rows(pad, DEV, 0.8, top_k, top_p, u=u, vocab=50257)
        view = pad.to(DEV)[:, :50257]
        assert view.stride(0) == 50304
        sc.check_rows(view, DEV, 0.8, top_k, top_p, u=u)


def test_llama_vocabs():
    sc.check_draws(DEV, 32000, 2, configs=((50, 0.9), (0, 1.0)))
    sc.check_draws(DEV, 128256, 1, configs=((50, 0.9), (0, 0.9), (0, 1.0)))
    sc.check_draws(DEV, 128256, 1, dtype=BF16, configs=((50, 0.9),))


def test_batch_32_distinct_rows():
    sc.check_draws(DEV, 503, 32)
    sc.check_draws(DEV, 5000, 32, dtype=BF16, configs=((50, 0.9),))


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("off", [1, 3, 5])
def test_unaligned_row_start(off, dtype):
    """A view starting `off` elements into a 16-byte-aligned buffer, with
    odd row strides: the rows' head and tail groups take element loads.
    Sentinels around the view must not change the result."""
    g = sc.gen(32 + off)
    B, V = 3, 4099
    x = sc.logits(g, B, V, dtype=dtype)
    u = sc.uniforms(g, B)
    buf = torch.full((B, V + 9), 60.0, dtype=dtype, device=DEV)
    view = buf[:, off:off + V]
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    for top_k, top_p in ((0, 1.0), (50, 0.9)):
        got = sc.check_rows(view, DEV, 0.8, top_k, top_p, u=u)
        want = sc.sample(x, DEV, temperature=0.8, top_k=top_k, top_p=top_p,
                         u=u)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_repeatable():
    g = sc.gen(33)
    x = sc.logits(g, 8, 50257).to(DEV)
    u = sc.uniforms(g, 8)
    first = sc.sample(x, DEV, temperature=0.8, top_k=50, top_p=0.9, u=u)
    for _ in range(19):
        again = sc.sample(x, DEV, temperature=0.8, top_k=50, top_p=0.9, u=u)
        assert torch.equal(first[0], again[0])
        assert torch.equal(first[1], again[1])


def test_out_is_written_in_place():
    x = sc.logits(sc.gen(1), 3, 64).to(DEV)
    u = sc.uniforms(sc.gen(2), 3).to(DEV)
    out = torch.full((3, 1), -1, dtype=torch.int64, device=DEV)
    got = ops.sample_logits(x, temperature=1.0, u=u, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, ops.sample_logits(x, temperature=1.0, u=u))
    assert torch.equal(out.cpu(),
                       ops.sample_logits(x.cpu(), temperature=1.0, u=u.cpu()))


def test_graph_replay_reads_step_on_the_device():
    g = sc.gen(34)
    x = sc.logits(g, 1, 503).repeat(4, 1).to(DEV)
    kw = dict(temperature=1.0, top_k=100, top_p=0.95, seed=11)
    step = torch.tensor([5], dtype=torch.int64, device=DEV)
    out = torch.zeros(4, 1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sample_logits(x, step=step, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sample_logits(x, step=step, out=out, **kw)
    replayed = []
    for _ in range(8):
        graph.replay()
        replayed.append(out.clone())
        step.add_(1)
    eager = [ops.sample_logits(
        x, step=torch.tensor([5 + i], dtype=torch.int64, device=DEV), **kw)
        for i in range(8)]
    replayed, eager = torch.cat(replayed, 1).cpu(), torch.cat(eager, 1).cpu()
    assert torch.equal(replayed, eager), (replayed, eager)
    assert replayed.unique().numel() > 4          # fresh uniforms per step
    for i in range(8):                             # and the CPU draws the same
        cpu = ops.sample_logits(x.cpu(), step=torch.tensor([5 + i]), **kw)
        assert torch.equal(cpu, eager[:, i:i + 1])


def test_refusals(monkeypatch):
    from tepdist_amd.ops import hip
    calls = []
    real = hip.ext.sample_logits
    monkeypatch.setattr(hip.ext, "sample_logits",
                        lambda *a: (calls.append(1), real(*a))[1])
    sc.check_refusals(DEV, launched=lambda: len(calls))
    x = torch.randn(2, 64, device=DEV)
    ops.sample_logits(x, temperature=1.0, u=torch.ones(2, device=DEV))
    assert len(calls) == 1                         # the counter does count


# -- engine ---------------------------------------------------------------

def _gpt2():
    from tepdist_amd.models import GPT2
    from tepdist_amd.models.configs import GPT2Config
    cfg = GPT2Config("sample-test", n_layer=2, n_embd=128, n_head=2,
                     n_ctx=64, vocab_size=503)
    torch.manual_seed(0)
    return cfg, GPT2(cfg, dtype=BF16).cuda().eval()


def _llama():
    from tepdist_amd.models.llama import Llama, LlamaConfig
    cfg = LlamaConfig("llama-test", n_layer=2, n_embd=256, n_head=4,
                      n_ctx=64, vocab_size=503, n_kv_head=2)
    torch.manual_seed(0)
    return cfg, Llama(cfg, dtype=BF16).cuda().eval()


@pytest.mark.parametrize("make", [_gpt2, _llama])
def test_engine_device_sampler_graph_equals_eager(make, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = make()
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device=DEV)
    gen = Generator(model)
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7, sampler="device")

    # the device path never draws on the host and never copies [B, V] there
    def no_multinomial(*a, **k):
        raise AssertionError("torch.multinomial on the device path")
    to_host = []
    real_cpu = torch.Tensor.cpu

    def cpu_spy(self, *a, **k):
        to_host.append(tuple(self.shape))
        return real_cpu(self, *a, **k)
    calls = []
    real_op = ops.sample_logits

    def op_spy(logits, **k):
        calls.append(logits.dtype)
        return real_op(logits, **k)
    replays = []
    real_replay = torch.cuda.CUDAGraph.replay

    def replay_spy(self):
        replays.append(1)
        return real_replay(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay_spy)
    monkeypatch.setattr(torch, "multinomial", no_multinomial)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu_spy)
    monkeypatch.setattr(ops, "sample_logits", op_spy)

    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 12, **kw)
    graph_calls, graph_replays = len(calls), len(replays)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 12, **kw)
    eager_replays = len(replays) - graph_replays
    assert not any(len(s) == 2 and s[1] >= cfg.vocab_size for s in to_host)
    monkeypatch.undo()
    assert a.shape == (2, 24) and torch.equal(a[:, :12], ids)
    assert bool(((a >= 0) & (a < cfg.vocab_size)).all())
    assert torch.equal(a, b), (a, b)
    # eager: one call per new token, on the head's bf16 output; the graph
    # run records its step once (first token, two warm-ups, the capture)
    # and replays it for the other nine tokens
    assert len(calls) - graph_calls == 12 and graph_calls == 4
    assert graph_replays == 9 and eager_replays == 0
    assert all(dt == BF16 for dt in calls)
    c = gen.generate(ids, 12, **{**kw, "seed": 8})
    assert not torch.equal(a, c)
    assert torch.equal(a, gen.generate(ids, 12, **{**kw, "sampler": "auto"}))
