"""Generator(kv_format="mxfp8") and the reference dispatch of the two cache
ops on an mx.MXCache (CPU, unmarked). Engine bound: max(3e-2 max|want|,
2 * yardstick), the rule and reason of test_linear_mx_a8_gpu.py (a flipped
code moves an element by a whole e4m3 step); the yardstick is the CPU engine
against itself on an fp32 copy of the model under the same kv_format."""

import copy

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import mx
from tepdist_amd.ops import reference as ref

BF16 = torch.bfloat16
# "gpt2-d32": head dim 32, which the kernels do not cover: on the GPU the
# engine then runs the reference ops on the GPU-resident MXCache
KINDS = ["llama", "gpt2", "gpt2-d32"]


def _model(kind):
    from test_linear_decode_mx_gpu import _model as covered
    if kind != "gpt2-d32":
        return covered(kind)
    from tepdist_amd.models import GPT2
    from tepdist_amd.models.configs import GPT2Config
    cfg = GPT2Config("kv-d32", n_layer=2, n_embd=128, n_head=4, n_ctx=64,
                     vocab_size=503)
    torch.manual_seed(0)
    return cfg, GPT2(cfg, dtype=BF16).cuda().eval()


@pytest.mark.parametrize("op", ["decode", "prefill"])
@pytest.mark.parametrize("rope", [None, 10000.0], ids=["plain", "rope"])
def test_reference_dispatch(op, rope):
    """ref op on an MXCache == ref op on its dequantized copy, bit for bit;
    the appended bytes equal mx_quantize of the (rotated, bf16) rows."""
    g = torch.Generator().manual_seed(3)
    B, Hkv, G, S, D, T = 2, 2, 2, 24, 64, 1 if op == "decode" else 5
    pos = torch.tensor([3, 11])
    kc, vc = (mx.kv_cache(B, Hkv, S, D) for _ in range(2))
    for c in (kc, vc):
        w = mx.mx_quantize(torch.randn(B * Hkv * S, D, generator=g), "mxfp8")
        c.codes.copy_(w.codes.view(B, Hkv, S, D))
        c.scales.copy_(w.scales.view(B, Hkv, S, D // 32))
    q = torch.randn(B, T, Hkv * G, D, generator=g).to(BF16)
    kn, vn = (torch.randn(B, T, Hkv, D, generator=g).to(BF16)
              for _ in range(2))
    kd, vd = mx.cache_dequantize(kc), mx.cache_dequantize(vc)
    rows = pos[:, None] + torch.arange(T)
    kr = ref._rope_at_f32(kn, rows[:, :, None], rope) if rope else kn.float()
    for b in range(B):      # what the quantized cache must hold afterwards
        for d, x in ((kd, kr), (vd, vn.float())):
            w = mx.mx_quantize(x[b].to(BF16).reshape(-1, D), "mxfp8")
            d[b][:, rows[b]] = mx.dequantize_ref(w).view(T, Hkv, D) \
                .transpose(0, 1)
    if op == "decode":
        got = ops.decode_attention(q[:, 0], kc, vc, pos, k_new=kn[:, 0],
                                   v_new=vn[:, 0], rope_theta=rope)
        want = ref.decode_attention(q[:, 0], kd, vd, pos, rope_theta=rope)
    else:
        got = ops.prefill_attention(q, kc, vc, pos, k_new=kn, v_new=vn,
                                    rope_theta=rope)
        want = ref.prefill_attention(q, kd, vd, pos, rope_theta=rope)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(mx.cache_dequantize(kc).view(torch.int16),
                       kd.view(torch.int16))
    assert torch.equal(mx.cache_dequantize(vc).view(torch.int16),
                       vd.view(torch.int16))
    w = mx.mx_quantize(vn[1].reshape(-1, D), "mxfp8")
    assert torch.equal(vc.codes[1][:, rows[1]].transpose(0, 1).reshape(-1, D),
                       w.codes)
    assert torch.equal(vc.scales[1][:, rows[1]].transpose(0, 1)
                       .reshape(-1, D // 32), w.scales)
    with pytest.raises(ValueError):
        ops.decode_attention(q[:, 0], kc, vd, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_engine_matches_cpu_engine(kind):
    """A 12-token prefill in chunks of 5 + 7, then one step."""
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    cpu = copy.deepcopy(model).cpu()
    gens = [Generator(m, kv_format="mxfp8")
            for m in (model, cpu, copy.deepcopy(cpu).float())]
    S0 = 12
    ids = torch.randint(0, cfg.vocab_size, (2, S0 + 1))
    res = []
    for gen in gens:
        w = gen.m.wte
        kc, vc = gen.new_caches(2, 32, w.device, w.dtype)
        assert isinstance(kc[0], mx.MXCache) and len(vc) == cfg.n_layer
        i = ids.to(w.device)
        ar = torch.arange(S0 + 1, device=w.device)
        with torch.no_grad():
            out = [gen._stack(gen._embed(i[:, a:b], ar[a:b]), kc, vc, a)
                   for a, b in ((0, 5), (5, 12), (12, 13))]
            res.append([t.float().cpu() for t in out[1:]
                        + [gen._logits(out[2])]])
    fails = []
    for got, want, f32, what in zip(*res, ("chunk hidden", "hidden",
                                           "logits")):
        err = (got - want).abs().max().item()
        yard = (want - f32).abs().max().item()
        bound = max(3e-2 * want.abs().max().item(), 2 * yard)
        print(f"{kind} kv mxfp8 {what}: max err {err:.3e}, yardstick "
              f"{yard:.3e}, bound {bound:.3e}")
        if got.shape != want.shape or not err <= bound:
            fails.append((what, err, bound))
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_engine_generate_graph_equals_eager(kind, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, kv_format="mxfp8")
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10, prefill_chunk=5)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10, prefill_chunk=5)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)


@pytest.mark.gpu
def test_engine_default_and_invalid_knob(monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model("gpt2")
    monkeypatch.delenv("TEPDIST_KV_FORMAT", raising=False)
    gen = Generator(model)
    assert gen.kv_format == "bf16"
    assert gen.new_caches(1, 8, "cuda", BF16)[0][0].dtype == BF16
    with pytest.raises(ValueError):
        Generator(model, kv_format="mxfp4")
    monkeypatch.setenv("TEPDIST_KV_FORMAT", "mxfp8")
    assert Generator(model).kv_format == "mxfp8"
