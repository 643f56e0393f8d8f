"""Llama models (MHA and grouped-query) in the KV-cache generation engine,
and the GQA / RoPE semantics of the reference decode-attention op; fp32 on
CPU."""

import dataclasses

import pytest
import torch

from tepdist_amd.inference import Generator
from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama
from tepdist_amd.ops import reference as ref

@pytest.fixture(scope="module", params=["mha", "gqa"])
def model(request):
    cfg = LLAMA_CONFIGS["llama-test"]
    if request.param == "gqa":
        cfg = dataclasses.replace(cfg, n_kv_head=2)
    torch.manual_seed(0)
    return Llama(cfg, dtype=torch.float32).eval()


def _full_forward_greedy(model, ids, n):
    cfg = model.cfg
    out = ids.clone()
    for _ in range(n):
        b, s = out.shape
        logits = model(out).reshape(b, s, -1)[:, -1, :cfg.vocab_size].float()
        out = torch.cat([out, logits.argmax(-1, keepdim=True)], dim=1)
    return out


def _ids(cfg, b, s, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.vocab_size, (b, s), generator=g)


def test_cached_greedy_matches_full_forward(model):
    ids = _ids(model.cfg, 2, 12, 1)
    with torch.no_grad():
        want = _full_forward_greedy(model, ids, 6)
    got = Generator(model).generate(ids, 6)
    assert torch.equal(got, want), (got, want)


def test_chunked_prefill_matches_full_forward(model):
    cfg = model.cfg
    gen = Generator(model)
    ids = _ids(cfg, 2, 12, 2)
    H, D = cfg.n_head, cfg.n_embd // cfg.n_head
    kc = [torch.zeros(2, gen.kv_heads, 16, D) for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    with torch.no_grad():
        gen._stack(gen._embed(ids[:, :8], torch.arange(8)), kc, vc, 0)
        x = gen._stack(gen._embed(ids[:, 8:], torch.arange(8, 12)), kc, vc,
                       8)
        got = gen._logits(x)[:, -1]
        want = model(ids).reshape(2, 12, -1)[:, -1]
    assert kc[0].shape[1] == cfg.kv_heads
    assert torch.allclose(got, want, atol=1e-4), (got - want).abs().max()


def test_fused_on_cpu_equals_composed(model):
    ids = _ids(model.cfg, 2, 9, 3)
    a = Generator(model, decode_attn="fused").generate(ids, 6)
    b = Generator(model, decode_attn="composed").generate(ids, 6)
    assert a.shape == (2, 15)
    assert torch.equal(a, b), (a, b)


# -- reference op -----------------------------------------------------------

B, H, HKV, S_MAX, D = 3, 6, 2, 17, 8
G = H // HKV


def _op_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, D, generator=g)
    kc = torch.randn(B, HKV, S_MAX, D, generator=g)
    vc = torch.randn(B, HKV, S_MAX, D, generator=g)
    kn = torch.randn(B, HKV, D, generator=g)
    vn = torch.randn(B, HKV, D, generator=g)
    return q, kc, vc, kn, vn


@pytest.mark.parametrize("append", [False, True])
def test_reference_gqa_equals_expanded_mha(append):
    q, kc, vc, kn, vn = _op_inputs()
    pos = torch.tensor([0, 7, S_MAX - 1])

    def ex(t):
        return t.repeat_interleave(G, dim=1)
    ke, ve = ex(kc), ex(vc)
    if append:
        got = ref.decode_attention(q, kc, vc, pos, k_new=kn, v_new=vn)
        want = ref.decode_attention(q, ke, ve, pos, k_new=ex(kn),
                                    v_new=ex(vn))
        assert torch.equal(ex(kc), ke) and torch.equal(ex(vc), ve)
    else:
        got = ref.decode_attention(q, kc, vc, pos)
        want = ref.decode_attention(q, ke, ve, pos)
    assert got.shape == (B, H, D)
    assert torch.allclose(got, want, atol=1e-6), (got - want).abs().max()


@pytest.mark.parametrize("append", [False, True])
def test_reference_rope_theta_equals_rope_at_then_plain(append):
    theta = 10000.0
    q, kc, vc, kn, vn = _op_inputs(1)
    pos = torch.tensor([3, 0, S_MAX + 4])            # last one is clamped
    pc = pos.clamp(0, S_MAX - 1)
    qr = ref.rope_at(q, pc[:, None], theta)
    k2, v2 = kc.clone(), vc.clone()
    if append:
        got = ref.decode_attention(q, kc, vc, pos, k_new=kn, v_new=vn,
                                   rope_theta=theta)
        want = ref.decode_attention(
            qr, k2, v2, pos, k_new=ref.rope_at(kn, pc[:, None], theta),
            v_new=vn)
        assert torch.equal(kc, k2) and torch.equal(vc, v2)
        # position 0 rotates by nothing
        assert torch.equal(kc[1, :, 0], kn[1])
    else:
        got = ref.decode_attention(q, kc, vc, pos, rope_theta=theta)
        want = ref.decode_attention(qr, k2, v2, pos)
    assert torch.allclose(got, want, atol=1e-6), (got - want).abs().max()


def test_rope_at_matches_rope_fwd():
    """rope_at at positions t % seq_len is ops.rope's rotation."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2 * 5, 3, D, generator=g)             # [tokens, H, D]
    want = ref.rope_fwd(x, seq_len=5)
    pos = torch.arange(10) % 5
    got = ref.rope_at(x, pos[:, None])
    assert torch.equal(got, want)
