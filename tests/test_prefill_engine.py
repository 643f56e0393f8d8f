"""Generator(prefill_attn=...) and generate(..., prefill_chunk=...): the
fused prefill path against the composed one. CPU: fp32, where both are the
same math. GPU: bf16 against the fp32 CPU engine on the same weights; the
fused path's error may not exceed 1.5 x the composed path's."""

import dataclasses

import pytest
import torch

from tepdist_amd.inference import Generator
from tepdist_amd.models import GPT2
from tepdist_amd.models.configs import GPT2Config
from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama

GQA = dataclasses.replace(LLAMA_CONFIGS["llama-test"], n_kv_head=2)  # G = 2
GPT = GPT2Config("gpt2-d64", n_layer=2, n_embd=128, n_head=2, n_ctx=128,
                 vocab_size=503)


def _model(kind):
    torch.manual_seed(0)
    return (Llama(GQA, dtype=torch.float32) if kind == "llama"
            else GPT2(GPT, dtype=torch.float32)).eval()


def _ids(cfg, b, s, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.vocab_size, (b, s), generator=g)


@torch.no_grad()
def _hidden(gen, ids, chunks):
    """Last hidden state of the prompt fed in the given chunk lengths."""
    cfg, dev = gen.cfg, ids.device
    p = next(gen.m.parameters())
    D = cfg.n_embd // cfg.n_head
    kc = [torch.zeros(ids.shape[0], gen.kv_heads, ids.shape[1], D,
                      dtype=p.dtype, device=dev) for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    c0 = 0
    for c in chunks:
        x = gen._stack(gen._embed(ids[:, c0:c0 + c],
                                  torch.arange(c0, c0 + c, device=dev)),
                       kc, vc, c0)
        c0 += c
    return x.float().cpu()


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_prefill_chunk_returns_the_same_tokens(kind):
    m = _model(kind)
    ids = _ids(m.cfg, 2, 11, 1)
    gen = Generator(m)
    want = gen.generate(ids, 5)
    for c in (1, 3, 11):
        assert torch.equal(gen.generate(ids, 5, prefill_chunk=c), want), c


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_fused_on_cpu_equals_composed(kind):
    m = _model(kind)
    ids = _ids(m.cfg, 2, 13, 2)
    for chunks in ((13,), (5, 8)):
        a = _hidden(Generator(m, prefill_attn="fused"), ids, chunks)
        b = _hidden(Generator(m, prefill_attn="composed"), ids, chunks)
        assert (a - b).abs().max() <= 1e-5 * b.abs().max(), chunks
    assert torch.equal(
        Generator(m, prefill_attn="fused").generate(ids, 4, prefill_chunk=4),
        Generator(m).generate(ids, 4))


def test_invalid_value():
    with pytest.raises(ValueError):
        Generator(_model("gpt2"), prefill_attn="nonsense")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(96,), (40, 56)], ids=["one", "40+56"])
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_fused_error_within_composed_error_on_gpu(kind, chunks):
    m32 = _model(kind)
    ids = _ids(m32.cfg, 2, 96, 3)
    want = _hidden(Generator(m32), ids, chunks)
    mb = _model(kind).to(torch.bfloat16).cuda()
    err = {how: float((_hidden(Generator(mb, prefill_attn=how), ids.cuda(),
                               chunks) - want).abs().max())
           for how in ("fused", "composed")}
    print(f"prefill engine {kind} {chunks}: {err}")
    assert err["fused"] <= 1.5 * err["composed"], err
