"""Fused KV-cache decode attention (decode_attention.hip) against the fp32
reference op on CPU copies.

Caches are views [:, :, :203] of an all-NaN [B, H, 256, D] buffer and
every row above a batch row's position is NaN too, so any use of an
invalid row shows up as NaN in the output while every access stays inside
the allocation. Criterion: max|out - ref| <= 1e-2 * max(1, max|ref|) — the
output is a convex combination of V rows; bf16 rounding of the output is
at most 2^-9 relative, a design rounding probabilities to bf16 would add
another 2^-9, fp32 summation order is far smaller; 1e-2 is about twice
the sum."""

import math

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, H, S_MAX, S_BUF = 2, 3, 203, 256
NAN = float("nan")


def _randn(*shape, gen):
    return torch.randn(*shape, generator=gen).to(BF16).cuda()


def _nan_caches(D, pos, gen, append=False, batch_buf=B, b0=0):
    """K/V cache views with rows 0..pos[b] valid (0..pos[b]-1 when the
    call appends row pos[b] itself) and NaN everywhere else."""
    out = []
    for _ in range(2):
        buf = torch.full((batch_buf, H, S_BUF, D), NAN, dtype=BF16,
                         device="cuda")
        c = buf[b0:b0 + B, :, :S_MAX]
        for b in range(B):
            n = pos[b] + (0 if append else 1)
            c[b, :, :n] = _randn(H, n, D, gen=gen)
        out.append(c)
    return out


def _cpu(t):
    return None if t is None else t.float().cpu()


def _check(out, want):
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert got.shape == want.shape and out.dtype == BF16
    assert torch.isfinite(got).all(), "an invalid (NaN) row was used"
    err = (got - want).abs().max().item()
    bound = 1e-2 * max(1.0, want.abs().max().item())
    assert err <= bound, f"max err {err} > {bound}"


def _bits(t):
    return t.contiguous().view(torch.int16)


POS_PAIRS = [[0, 202], [7, 8], [63, 64], [127, 128]]


@pytest.mark.parametrize("pos", POS_PAIRS, ids=lambda p: f"p{p[0]}_{p[1]}")
@pytest.mark.parametrize("splits", [1, 2, 3, 7])
@pytest.mark.parametrize("D", [64, 128])
def test_numerics(D, splits, pos):
    gen = torch.Generator().manual_seed(D + splits)
    kc, vc = _nan_caches(D, pos, gen)
    q = _randn(B, H, D, gen=gen)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu())
    out = ops.decode_attention(q, kc, vc, pt, splits=splits)
    _check(out, want)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_broadcast_position(D, splits):
    gen = torch.Generator().manual_seed(5)
    kc, vc = _nan_caches(D, [130, 130], gen)
    q = _randn(B, H, D, gen=gen)
    pt = torch.tensor([130], dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu())
    _check(ops.decode_attention(q, kc, vc, pt, splits=splits), want)


def test_default_splits_heuristic():
    gen = torch.Generator().manual_seed(6)
    kc, vc = _nan_caches(64, [202, 100], gen)
    q = _randn(B, H, 64, gen=gen)
    pt = torch.tensor([202, 100], dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu())
    _check(ops.decode_attention(q, kc, vc, pt), want)


@pytest.mark.parametrize("D", [64, 128])
def test_dominant_key_in_last_split(D):
    """One key aligned with q at 8*sqrt(D)/|q| scale: its logit is 8*|q|
    (~64) against ~N(0,1) for the rest, so the softmax is one-hot on a row
    of the LAST of 3 splits — a wrong max or rescale across splits breaks
    it."""
    gen = torch.Generator().manual_seed(7)
    pos, row = [202, 202], 190
    kc, vc = _nan_caches(D, pos, gen)
    q = _randn(B, H, D, gen=gen)
    qn = q.float()
    kc[:, :, row] = (8.0 * math.sqrt(D) * qn /
                     qn.norm(dim=-1, keepdim=True)).to(BF16)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu())
    out = ops.decode_attention(q, kc, vc, pt, splits=3)
    _check(out, want)
    _check(out, _cpu(vc[:, :, row]))


@pytest.mark.parametrize("pos", [[0, 202], [63, 64], [127, 128]],
                         ids=lambda p: f"p{p[0]}_{p[1]}")
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_append(D, splits, pos):
    """cache[..., p, :] holds NaN before the call: a finite result proves
    row p is never read. Afterwards row p is the new row bit for bit and
    nothing else in the buffer changed."""
    gen = torch.Generator().manual_seed(11 + splits)
    kc, vc = _nan_caches(D, pos, gen, append=True)
    q, kn, vn = (_randn(B, H, D, gen=gen) for _ in range(3))
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    k0, v0 = kc.clone(), vc.clone()
    kr, vr = _cpu(kc), _cpu(vc)
    want = ref.decode_attention(_cpu(q), kr, vr, pt.cpu(), k_new=_cpu(kn),
                                v_new=_cpu(vn))
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                               splits=splits)
    _check(out, want)
    for b in range(B):
        p = pos[b]
        assert torch.equal(_bits(kc[b, :, p]), _bits(kn[b]))
        assert torch.equal(_bits(vc[b, :, p]), _bits(vn[b]))
        keep = torch.arange(S_MAX, device="cuda") != p
        assert torch.equal(_bits(kc[b][:, keep]), _bits(k0[b][:, keep]))
        assert torch.equal(_bits(vc[b][:, keep]), _bits(v0[b][:, keep]))


@pytest.mark.parametrize("D", [64, 128])
def test_strided_operands(D):
    """q/k_new/v_new as views of a packed [B, 1, 3*H*D] projection, caches
    as the [1:3] batch slice of a batch-4 buffer."""
    gen = torch.Generator().manual_seed(13)
    pos = [150, 37]
    kc, vc = _nan_caches(D, pos, gen, append=True, batch_buf=4, b0=1)
    qkv = _randn(B, 1, 3 * H * D, gen=gen)
    q3 = qkv.view(B, 3, H, D)
    q, kn, vn = q3[:, 0], q3[:, 1], q3[:, 2]
    assert not q.is_contiguous() and not kc.is_contiguous()
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    kr, vr = _cpu(kc), _cpu(vc)
    want = ref.decode_attention(_cpu(q), kr, vr, pt.cpu(), k_new=_cpu(kn),
                                v_new=_cpu(vn))
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn, splits=2)
    _check(out, want)
    for b in range(B):
        assert torch.equal(_bits(kc[b, :, pos[b]]), _bits(kn[b]))
        assert torch.equal(_bits(vc[b, :, pos[b]]), _bits(vn[b]))


def test_unsupported_inputs_are_refused():
    gen = torch.Generator().manual_seed(1)
    pt = torch.tensor([3], dtype=torch.long, device="cuda")
    q = _randn(B, H, 32, gen=gen)
    c = _randn(B, H, 16, 32, gen=gen)
    with pytest.raises(ValueError):
        ops.decode_attention(q, c, c.clone(), pt)
    q = _randn(B, H, 64, gen=gen)
    c = _randn(B, H, 16, 64, gen=gen)
    with pytest.raises(RuntimeError):
        ops.decode_attention(q, c, c.clone(), pt, splits=33)


def test_graph_replay():
    """One captured append-mode call replayed while the device position
    advances across a row-group/wave boundary (127 -> 128)."""
    D, p0 = 64, 125
    gen = torch.Generator().manual_seed(17)
    kc, vc = _nan_caches(D, [p0, p0], gen, append=True)
    kr, vr = _cpu(kc), _cpu(vc)
    q, kn, vn = (_randn(B, H, D, gen=gen) for _ in range(3))
    pos = torch.full((1,), p0, dtype=torch.long, device="cuda")

    def refill():
        for t in (q, kn, vn):
            t.copy_(_randn(B, H, D, gen=gen))

    def expect():
        return ref.decode_attention(_cpu(q), kr, vr, pos.cpu(),
                                    k_new=_cpu(kn), v_new=_cpu(vn))

    def call():
        return ops.decode_attention(q, kc, vc, pos, k_new=kn, v_new=vn,
                                    splits=2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            want = expect()
            _check(call(), want)
            pos.add_(1)
            refill()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in range(3):
        if i:
            pos.add_(1)
            refill()
        want = expect()
        graph.replay()
        _check(out, want)
    assert int(pos.item()) == p0 + 4
    torch.cuda.synchronize()
    valid = slice(0, p0 + 5)
    assert torch.equal(kc[:, :, valid].float().cpu(), kr[:, :, valid])
    assert torch.equal(vc[:, :, valid].float().cpu(), vr[:, :, valid])


def _engine_model():
    from tepdist_amd.models import GPT2
    from tepdist_amd.models.configs import GPT2Config
    cfg = GPT2Config("decode-test", n_layer=2, n_embd=128, n_head=2,
                     n_ctx=64, vocab_size=503)          # head dim 64
    torch.manual_seed(0)
    return cfg, GPT2(cfg, dtype=BF16).cuda().eval()


def test_engine_step_fused_matches_composed():
    from tepdist_amd.inference import Generator
    cfg, model = _engine_model()
    gf = Generator(model, decode_attn="fused")
    gc = Generator(model, decode_attn="composed")
    Hh, D, S0 = cfg.n_head, cfg.n_embd // cfg.n_head, 12
    ids = torch.randint(0, cfg.vocab_size, (2, S0 + 1), device="cuda")
    kc = [torch.zeros(2, Hh, 32, D, dtype=BF16, device="cuda")
          for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    with torch.no_grad():
        x = ops.embedding(ids[:, :S0], model.wte) + \
            ops.embedding(torch.arange(S0, device="cuda"), model.wpe)
        gc._stack(x, kc, vc, 0)
        x1 = ops.embedding(ids[:, S0:], model.wte) + \
            ops.embedding(torch.tensor([S0], device="cuda"), model.wpe)
        kf, vf = [t.clone() for t in kc], [t.clone() for t in vc]
        assert gf._fused_decode(x1, D) and not gc._fused_decode(x1, D)
        hf = gf._stack(x1, kf, vf, S0)
        hc = gc._stack(x1, kc, vc, S0)
    torch.cuda.synchronize()
    err = (hf.float() - hc.float()).abs().max().item()
    bound = 3e-2 * hc.float().abs().max().item()
    assert err <= bound, (err, bound)
    # layer 0 sees identical inputs: its appended cache rows are bit-equal
    assert torch.equal(_bits(kf[0]), _bits(kc[0]))
    assert torch.equal(_bits(vf[0]), _bits(vc[0]))


def test_engine_generate_graph_equals_eager(monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _engine_model()
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, decode_attn="fused")
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)
