"""ops.sample_logits on the CPU (ops/reference.py) against the float64
oracle, and the generation engine's samplers. The same checks run on the
HIP kernel in test_sampling_gpu.py; the bound is derived in
sampling_checks.py."""

import pytest
import torch

import sampling_checks as sc
from tepdist_amd import ops
from tepdist_amd.inference import Generator
from tepdist_amd.models import GPT2, GPT2_CONFIGS


def test_topk_thresholds():
    sc.check_topk_thresholds("cpu")


def test_topp_thresholds():
    sc.check_topp_thresholds("cpu")


def test_no_filter_threshold():
    sc.check_no_filter_threshold("cpu")


@pytest.mark.parametrize("top_k,top_p", [(50, 1.0), (0, 0.9), (0, 1.0)])
def test_cdf_sweep(top_k, top_p):
    sc.check_cdf_sweep("cpu", top_k, top_p)


@pytest.mark.parametrize("V", [1, 7, 64, 503, 4097])
@pytest.mark.parametrize("B", [1, 3])
def test_draws(V, B):
    sc.check_draws("cpu", V, B)


def test_u_ends():
    sc.check_u_ends("cpu")


def test_special_rows():
    sc.check_special_rows("cpu")


def test_views():
    sc.check_views("cpu")


def test_philox():
    sc.check_philox("cpu")


def test_refusals():
    sc.check_refusals("cpu")


def test_out_is_written_in_place():
    x = sc.logits(sc.gen(1), 3, 64)
    u = sc.uniforms(sc.gen(2), 3)
    out = torch.full((3, 1), -1, dtype=torch.int64)
    got = ops.sample_logits(x, temperature=1.0, u=u, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, ops.sample_logits(x, temperature=1.0, u=u))


# -- engine ---------------------------------------------------------------

def _model(name="gpt2-test"):
    torch.manual_seed(0)
    cfg = GPT2_CONFIGS[name]
    return cfg, GPT2(cfg, dtype=torch.float32).eval()


def _llama():
    from tepdist_amd.models.llama import Llama, LlamaConfig
    cfg = LlamaConfig("sample-test", n_layer=2, n_embd=64, n_head=4,
                      n_ctx=64, vocab_size=503, n_kv_head=2)
    torch.manual_seed(0)
    return cfg, Llama(cfg, dtype=torch.float32).eval()


@pytest.mark.parametrize("make", [_model, _llama])
def test_engine_device_sampler_seeds(make):
    cfg, model = make()
    ids = torch.randint(0, cfg.vocab_size, (2, 8))
    gen = Generator(model)
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, sampler="device")
    a = gen.generate(ids, 16, seed=7, **kw)
    b = gen.generate(ids, 16, seed=7, **kw)
    c = gen.generate(ids, 16, seed=8, **kw)
    assert a.shape == (2, 24) and torch.equal(a[:, :8], ids)
    assert bool(((a >= 0) & (a < cfg.vocab_size)).all())
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


def test_engine_device_sampler_draws_at_written_position(monkeypatch):
    """One op call per new token, with step = the position the token is
    written to, the first one after the prompt included."""
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (2, 8))
    steps = []
    real = ops.sample_logits

    def spy(logits, **kw):
        steps.append(int(kw["step"]))
        assert kw["seed"] == 3 and kw["top_k"] == 20 and kw["top_p"] == 0.9
        return real(logits, **kw)

    monkeypatch.setattr(ops, "sample_logits", spy)
    Generator(model).generate(ids, 5, temperature=0.8, top_k=20, top_p=0.9,
                              seed=3, sampler="device")
    assert steps == [8, 9, 10, 11, 12]


def test_engine_device_sampler_fused_equals_composed():
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (2, 8))
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5, sampler="device")
    a = Generator(model, decode_attn="fused").generate(ids, 12, **kw)
    b = Generator(model, decode_attn="composed").generate(ids, 12, **kw)
    assert torch.equal(a, b)


def test_engine_sampler_choice(monkeypatch):
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (1, 8))
    gen = Generator(model)
    with pytest.raises(ValueError):
        gen.generate(ids, 2, temperature=0.8, sampler="gpu")
    monkeypatch.setenv("TEPDIST_SAMPLER", "nonsense")
    with pytest.raises(ValueError):
        gen.generate(ids, 2, temperature=0.8)
    # the environment selects, the argument wins, "auto" is host on the CPU
    kw = dict(temperature=0.8, top_k=20, seed=7)
    monkeypatch.setenv("TEPDIST_SAMPLER", "device")
    dev = gen.generate(ids, 8, **kw)
    host = gen.generate(ids, 8, sampler="host", **kw)
    assert torch.equal(dev, gen.generate(ids, 8, sampler="device", **kw))
    assert torch.equal(host, gen.generate(ids, 8, sampler="auto", **kw))
    monkeypatch.delenv("TEPDIST_SAMPLER")
    assert torch.equal(host, gen.generate(ids, 8, **kw))
    assert not torch.equal(host, dev)


def _sampled_as_before(gen, ids, n, temperature, top_k, seed):
    """The engine's sampled loop as it stood before the samplers: scaled
    logits, top-k fill, softmax, torch.multinomial on the CPU from
    torch.Generator(seed)."""
    cfg = gen.cfg
    B, S0 = ids.shape
    D = cfg.n_embd // cfg.n_head
    kc = [torch.zeros(B, cfg.n_head, S0 + n, D) for _ in range(cfg.n_layer)]
    vc = [torch.zeros(B, cfg.n_head, S0 + n, D) for _ in range(cfg.n_layer)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = ids
    with torch.no_grad():
        x = gen._stack(gen._embed(ids, torch.arange(S0)), kc, vc, 0)
        for cur in range(S0, S0 + n):
            logits = gen._logits(x).float()[:, -1][:, :cfg.vocab_size]
            logits = logits / temperature
            kth = logits.topk(top_k, dim=-1).values[:, -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
            nxt = torch.multinomial(torch.softmax(logits, dim=-1), 1,
                                    generator=g)
            out = torch.cat([out, nxt], dim=1)
            x = gen._stack(gen._embed(nxt, torch.full((1,), cur)), kc, vc,
                           cur)
    return out


def test_engine_default_sampler_unchanged(monkeypatch):
    """The calls of test_inference_cpu.py give the tokens they gave before:
    the default is the host sampler and top_p = 1.0 changes nothing."""
    monkeypatch.delenv("TEPDIST_SAMPLER", raising=False)
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (1, 8))
    gen = Generator(model)
    a = gen.generate(ids, 5, temperature=0.8, top_k=20, seed=7)
    assert torch.equal(a, _sampled_as_before(gen, ids, 5, 0.8, 20, 7))
    assert torch.equal(a, gen.generate(ids, 5, temperature=0.8, top_k=20,
                                       seed=7, top_p=1.0))
    assert torch.equal(a, gen.generate(ids, 5, temperature=0.8, top_k=20,
                                       seed=7, sampler="host"))
    greedy = gen.generate(ids, 6)
    assert torch.equal(greedy, gen.generate(ids, 6, sampler="device"))


def test_engine_host_top_p():
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (2, 8))
    gen = Generator(model)
    greedy = gen.generate(ids, 8)
    for seed in (0, 1):
        assert torch.equal(greedy, gen.generate(
            ids, 8, temperature=0.8, top_p=1e-6, seed=seed))
    wide = gen.generate(ids, 8, temperature=1.5, seed=3)
    tight = gen.generate(ids, 8, temperature=1.5, seed=3, top_p=0.05)
    assert not torch.equal(wide, tight)
