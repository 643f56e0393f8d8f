"""Decode attention over a KV cache: the pure-torch reference op against a
brute-force loop, its append mode, and the engine wiring of
decode_attn="fused" (reference op on CPU)."""

import math

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.inference import Generator
from tepdist_amd.models import GPT2, GPT2_CONFIGS
from tepdist_amd.ops import reference as ref

B, H, S_MAX, D = 3, 2, 17, 8


def _brute(q, kc, vc, pos):
    """Per-(b, h) softmax over rows 0..pos[b] of the caches."""
    out = torch.empty_like(q)
    for b in range(q.shape[0]):
        n = int(pos[b]) + 1
        for h in range(q.shape[1]):
            s = (kc[b, h, :n] @ q[b, h]) / math.sqrt(q.shape[-1])
            out[b, h] = torch.softmax(s, dim=-1) @ vc[b, h, :n]
    return out


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, D, generator=g)
    kc = torch.randn(B, H, S_MAX, D, generator=g)
    vc = torch.randn(B, H, S_MAX, D, generator=g)
    return q, kc, vc


@pytest.mark.parametrize("pos", [[0], [8], [S_MAX - 1],
                                 [0, 8, S_MAX - 1], [S_MAX - 1, 0, 5]])
def test_reference_matches_brute_force(pos):
    q, kc, vc = _inputs()
    pt = torch.tensor(pos, dtype=torch.long)
    got = ref.decode_attention(q, kc, vc, pt)
    want = _brute(q, kc, vc, pt.expand(B) if len(pos) == 1 else pt)
    assert got.shape == (B, H, D) and got.dtype == q.dtype
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()


def test_reference_ignores_rows_above_position():
    q, kc, vc = _inputs(1)
    pt = torch.tensor([0, 8, S_MAX - 2], dtype=torch.long)
    want = _brute(q, kc, vc, pt)
    for b in range(B):
        kc[b, :, int(pt[b]) + 1:] = float("nan")
        vc[b, :, int(pt[b]) + 1:] = float("inf")
    got = ops.decode_attention(q, kc, vc, pt)
    assert torch.allclose(got, want, atol=1e-5)


@pytest.mark.parametrize("pos", [[0], [S_MAX - 1], [3, 0, S_MAX - 1]])
def test_reference_append_is_write_then_attend(pos):
    q, kc, vc = _inputs(2)
    g = torch.Generator().manual_seed(3)
    kn = torch.randn(B, H, D, generator=g)
    vn = torch.randn(B, H, D, generator=g)
    pt = torch.tensor(pos, dtype=torch.long)
    pb = pt.expand(B) if len(pos) == 1 else pt
    k0, v0 = kc.clone(), vc.clone()
    kw, vw = kc.clone(), vc.clone()
    for b in range(B):
        kw[b, :, int(pb[b])] = kn[b]
        vw[b, :, int(pb[b])] = vn[b]
    want = _brute(q, kw, vw, pb)
    got = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()
    for b in range(B):
        p = int(pb[b])
        assert torch.equal(kc[b, :, p], kn[b])
        assert torch.equal(vc[b, :, p], vn[b])
        keep = torch.arange(S_MAX) != p
        assert torch.equal(kc[b][:, keep], k0[b][:, keep])
        assert torch.equal(vc[b][:, keep], v0[b][:, keep])


def _full_forward_greedy(model, ids, n):
    cfg = model.cfg
    out = ids.clone()
    for _ in range(n):
        logits = model(out)[:, -1, :cfg.vocab_size].float()
        out = torch.cat([out, logits.argmax(-1, keepdim=True)], dim=1)
    return out


def _model():
    torch.manual_seed(0)
    cfg = GPT2_CONFIGS["gpt2-test"]
    return cfg, GPT2(cfg, dtype=torch.float32).eval()


def test_fused_engine_greedy_matches_full_forward():
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (2, 12))
    with torch.no_grad():
        want = _full_forward_greedy(model, ids, 6)
    got = Generator(model, decode_attn="fused").generate(ids, 6)
    assert torch.equal(got, want), (got, want)


def test_fused_engine_sampled_matches_composed():
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (1, 8))
    kw = dict(temperature=0.8, top_k=20, seed=7)
    a = Generator(model, decode_attn="fused").generate(ids, 5, **kw)
    b = Generator(model, decode_attn="composed").generate(ids, 5, **kw)
    assert torch.equal(a, b)
    assert a.shape == (1, 13)


def test_fused_engine_calls_the_op(monkeypatch):
    """"fused" routes every single-token step through ops.decode_attention;
    "auto" on CPU stays composed."""
    cfg, model = _model()
    ids = torch.randint(0, cfg.vocab_size, (1, 8))
    calls = []
    real = ops.decode_attention

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "decode_attention", spy)
    Generator(model, decode_attn="auto").generate(ids, 3)
    assert not calls
    Generator(model, decode_attn="fused").generate(ids, 3)
    # the eager loop runs one single-token stack pass per sampled token
    assert len(calls) == 3 * cfg.n_layer


def test_decode_attn_mode_validation(monkeypatch):
    _, model = _model()
    with pytest.raises(ValueError):
        Generator(model, decode_attn="bogus")
    monkeypatch.setenv("TEPDIST_DECODE_ATTN", "composed")
    assert Generator(model).decode_attn == "composed"
    monkeypatch.delenv("TEPDIST_DECODE_ATTN")
    assert Generator(model).decode_attn == "auto"
