"""Grouped-query attention in models/llama.py (LlamaConfig.n_kv_head), fp32
on CPU: the MHA default is untouched, a GQA model equals the MHA model whose
K/V weights are the GQA rows repeated per group, it trains, and the layers
that do not support it say so."""

import dataclasses

import pytest
import torch

from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama, LlamaConfig
from tepdist_amd.parallel.tp import ParallelEnv


def _batch(cfg, seed=0, b=2, s=33):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (b, s), generator=g)
    return ids[:, :-1], ids[:, 1:]


def test_n_kv_head_equal_to_n_head_changes_nothing():
    base = LlamaConfig()
    same = LlamaConfig(n_kv_head=base.n_head)
    a, b = Llama(base), Llama(same)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(pa) == list(pb)
    for name in pa:
        assert pa[name].shape == pb[name].shape, name
        assert torch.equal(pa[name], pb[name]), name
    x, y = _batch(base)
    assert torch.equal(a(x, labels=y), b(x, labels=y))


def test_config_checks_divisibility():
    with pytest.raises(ValueError):
        LlamaConfig(n_head=4, n_kv_head=3)
    cfg = LLAMA_CONFIGS["llama-1b-gqa"]
    assert (cfg.n_embd, cfg.n_head, cfg.kv_heads, cfg.n_layer, cfg.n_ctx,
            cfg.vocab_size, cfg.ffn_mult) == (2048, 32, 8, 22, 2048, 32000,
                                              3)
    assert LlamaConfig().kv_heads == LlamaConfig().n_head


def _gqa_and_expanded_mha():
    """A GQA model and the MHA model that computes the same function: K/V
    weight rows of K/V head j repeated for the G query heads of group j."""
    gcfg = LlamaConfig(n_embd=256, n_head=4, n_kv_head=2)
    mcfg = dataclasses.replace(gcfg, n_kv_head=None)
    gqa, mha = Llama(gcfg), Llama(mcfg)
    H, Hkv, D, d = 4, 2, 64, 256
    G = H // Hkv
    with torch.no_grad():
        for pg, pm in zip(gqa.parameters(), mha.parameters()):
            if pg.shape == pm.shape:
                pm.copy_(pg)
        for bg, bm in zip(gqa.blocks, mha.blocks):
            assert bg.w_qkv.shape == ((H + 2 * Hkv) * D, d)
            wq, wk, wv = bg.w_qkv.split([H * D, Hkv * D, Hkv * D], dim=0)

            def rep(w):
                return w.reshape(Hkv, D, d).repeat_interleave(
                    G, dim=0).reshape(H * D, d)
            bm.w_qkv.copy_(torch.cat([wq, rep(wk), rep(wv)], dim=0))
    return gqa, mha, (H, Hkv, D, d, G)


def test_gqa_matches_mha_with_repeated_kv_weights():
    gqa, mha, (H, Hkv, D, d, G) = _gqa_and_expanded_mha()
    x, y = _batch(gqa.cfg, seed=1)
    lg, lm = gqa(x, labels=y), mha(x, labels=y)
    assert abs(lg.item() - lm.item()) <= 1e-5, (lg.item(), lm.item())
    lg.backward()
    lm.backward()
    for bg, bm in zip(gqa.blocks, mha.blocks):
        gq, gk, gv = bg.w_qkv.grad.split([H * D, Hkv * D, Hkv * D], dim=0)
        mq, mk, mv = bm.w_qkv.grad.split(H * D, dim=0)
        assert torch.allclose(gq, mq, atol=1e-5)
        for got, full in ((gk, mk), (gv, mv)):
            want = full.reshape(Hkv, G, D, d).sum(1).reshape(Hkv * D, d)
            assert torch.allclose(got, want, atol=1e-5), \
                (got - want).abs().max()
        assert torch.allclose(bg.w_o.grad, bm.w_o.grad, atol=1e-5)


def test_gqa_init_is_order_independent():
    cfg = LlamaConfig(n_embd=256, n_head=4, n_kv_head=2)
    a = Llama(cfg)
    torch.manual_seed(123)
    torch.randn(7)
    b = Llama(cfg)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    assert a.blocks[0].w_qkv.std().item() == pytest.approx(0.02, rel=0.1)


def test_gqa_tiny_trains():
    torch.manual_seed(0)
    cfg = dataclasses.replace(LLAMA_CONFIGS["llama-test"], n_kv_head=2)
    model = Llama(cfg)
    from tepdist_amd.train.optim import AdamW
    opt = AdamW(model.parameters(), lr=3e-3)
    ids = torch.randint(0, cfg.vocab_size, (2, 33))
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = model(ids[:, :-1], labels=ids[:, 1:])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 0.5, losses


def test_gqa_refused_under_tp_and_in_ir():
    cfg = LlamaConfig(n_embd=256, n_head=4, n_kv_head=2)
    env = dataclasses.replace(ParallelEnv.single(), tp_size=2)
    with pytest.raises(NotImplementedError):
        Llama(cfg, env=env)
    from tepdist_amd.ir.capture import llama_ir
    with pytest.raises(NotImplementedError):
        llama_ir(cfg, 2, 16)
    llama_ir(LlamaConfig(), 2, 16)          # MHA still exports
