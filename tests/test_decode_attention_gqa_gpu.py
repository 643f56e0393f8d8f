"""Grouped-query + fused-RoPE decode attention (decode_attn_gqa_kernel in
decode_attention.hip) against the fp32 reference op on CPU copies, and the
Llama path of the generation engine that uses it.

Same harness as test_decode_attention_gpu.py: caches are views [:, :, :203]
of an all-NaN [B, Hkv, 256, D] buffer and every row above a batch row's
position is NaN too, so any use of an invalid row shows up as NaN in the
output while every access stays inside the allocation. Hkv = 3 is odd so a
wrong head stride (H for Hkv or the reverse) lands on another head.

Criterion: max|out - ref| <= 1e-2 * max(1, max|ref|) — the output is a
convex combination of V rows; bf16 rounding of the output is at most 2^-9
relative, a design rounding probabilities to bf16 would add another 2^-9,
fp32 summation order is far smaller; 1e-2 is about twice the sum. With
rope_theta the kernel's fast exp/sin/cos at the positions used here (<= 520)
moves an angle by < 3e-4 rad, i.e. a logit by < 3e-4 of |q||k|/sqrt(D) ~
3e-3 absolute and a probability by that much relative, which the same bound
covers; the reference leaves q unrounded as the kernel does.

Appended K rows with rope: |k_row - want| <= 2^-7 * max|want|, want = the
fp32 CPU rotation rounded to bf16. One bf16 rounding is 2^-9 relative, and
a rotation that differs in the last fp32 bits can move the rounding by one
ulp, 2^-8 of the element's binade. At p = 0 (cos 1, sin 0 exactly) and
without rope the row is k_new bit for bit; V rows always are."""

import math

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, HKV, S_MAX, S_BUF = 2, 3, 203, 256
NAN = float("nan")
THETA = 10000.0
GROUPS = [1, 2, 4, 8]


def _randn(*shape, gen):
    return torch.randn(*shape, generator=gen).to(BF16).cuda()


def _nan_caches(D, pos, gen, append=False, batch_buf=B, b0=0, s_max=S_MAX,
                s_buf=S_BUF):
    """K/V cache views with rows 0..pos[b] valid (0..pos[b]-1 when the
    call appends row pos[b] itself) and NaN everywhere else."""
    out = []
    for _ in range(2):
        buf = torch.full((batch_buf, HKV, s_buf, D), NAN, dtype=BF16,
                         device="cuda")
        c = buf[b0:b0 + B, :, :s_max]
        for b in range(B):
            n = pos[b] + (0 if append else 1)
            c[b, :, :n] = _randn(HKV, n, D, gen=gen)
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


def _check_k_row(got, want32):
    """got: bf16 row(s) the kernel stored; want32: fp32 CPU rotation."""
    want = want32.to(BF16).float()
    err = (got.float().cpu() - want).abs().max().item()
    bound = 2.0 ** -7 * want.abs().max().item()
    assert err <= bound, f"rotated K row: {err} > {bound}"


POS = [[0, 202], [63, 64], [127, 128]]
_pid = lambda p: f"p{p[0]}_{p[1]}"        # noqa: E731


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("pos", POS, ids=_pid)
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_numerics(G, D, splits, pos, rope):
    gen = torch.Generator().manual_seed(G * 1000 + D + splits)
    theta = THETA if rope else None
    kc, vc = _nan_caches(D, pos, gen)
    q = _randn(B, HKV * G, D, gen=gen)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu(),
                                rope_theta=theta)
    out = ops.decode_attention(q, kc, vc, pt, splits=splits,
                               rope_theta=theta)
    _check(out, want)


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("pos", POS, ids=_pid)
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_append(G, D, splits, pos, rope):
    """cache[..., p, :] holds NaN before the call: a finite result proves
    row p is never read. Afterwards row p is the new row (K rotated when
    rope is on) and nothing else in the buffer changed."""
    gen = torch.Generator().manual_seed(11 + splits + G)
    theta = THETA if rope else None
    kc, vc = _nan_caches(D, pos, gen, append=True)
    q = _randn(B, HKV * G, D, gen=gen)
    kn, vn = (_randn(B, HKV, D, gen=gen) for _ in range(2))
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    k0, v0 = kc.clone(), vc.clone()
    kr, vr = _cpu(kc), _cpu(vc)
    want = ref.decode_attention(_cpu(q), kr, vr, pt.cpu(), k_new=_cpu(kn),
                                v_new=_cpu(vn), rope_theta=theta)
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                               splits=splits, rope_theta=theta)
    _check(out, want)
    for b in range(B):
        p = pos[b]
        assert torch.equal(_bits(vc[b, :, p]), _bits(vn[b]))
        if not rope or p == 0:
            assert torch.equal(_bits(kc[b, :, p]), _bits(kn[b]))
        else:
            _check_k_row(kc[b, :, p], kr[b, :, p])
        keep = torch.arange(S_MAX, device="cuda") != p
        assert torch.equal(_bits(kc[b][:, keep]), _bits(k0[b][:, keep]))
        assert torch.equal(_bits(vc[b][:, keep]), _bits(v0[b][:, keep]))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_group_members_are_not_mixed(G, D):
    """Each of the G queries of one K/V head is aligned (8*sqrt(D)/|q|
    scale, logit ~8|q| against ~N(0, 8) for another member's row and
    ~N(0,1) for the rest) with a DIFFERENT cache row, the first of them in
    the last of 3 splits: head h must return its own V row."""
    gen = torch.Generator().manual_seed(7 + G)
    pos = [202, 202]
    rows = [190, 5, 75, 150, 40, 100, 120, 180][:G]
    kc, vc = _nan_caches(D, pos, gen)
    q = _randn(B, HKV * G, D, gen=gen)
    qn = q.float().view(B, HKV, G, D)
    for g, row in enumerate(rows):
        kc[:, :, row] = (8.0 * math.sqrt(D) * qn[:, :, g] /
                         qn[:, :, g].norm(dim=-1, keepdim=True)).to(BF16)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu())
    out = ops.decode_attention(q, kc, vc, pt, splits=3)
    _check(out, want)
    own = torch.stack([_cpu(vc[:, :, row]) for row in rows], dim=2)
    _check(out, own.reshape(B, HKV * G, D))


def test_default_splits_heuristic():
    """splits=None: group >= 4 splits earlier (256 workgroups, >= 256 rows
    per split) than the G <= 2 rule (64 workgroups, >= 512 rows); the
    result is a function of the shapes alone."""
    from tepdist_amd.ops import hip
    assert hip.decode_splits(256, 640, 4) == 1
    assert hip.decode_splits(128, 640, 8) == 2
    assert hip.decode_splits(8, 2048, 4) == 8
    assert hip.decode_splits(128, 640, 2) == 1
    assert hip.decode_splits(16, 2048) == 4 and hip.decode_splits(512, 640) == 1
    G, D, s_max = 4, 64, 1000
    assert hip.decode_splits(B * HKV, s_max, G) == 2
    gen = torch.Generator().manual_seed(6)
    pos = [520, 300]
    kc, vc = _nan_caches(D, pos, gen, append=True, s_max=s_max, s_buf=1024)
    q = _randn(B, HKV * G, D, gen=gen)
    kn, vn = (_randn(B, HKV, D, gen=gen) for _ in range(2))
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(_cpu(q), _cpu(kc), _cpu(vc), pt.cpu(),
                                k_new=_cpu(kn), v_new=_cpu(vn),
                                rope_theta=THETA)
    _check(ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                                rope_theta=THETA), want)


@pytest.mark.parametrize("D", [64, 128])
def test_strided_operands(D):
    """q/k_new/v_new as views of a packed [B, 1, (H + 2 Hkv) D] projection,
    caches as the [1:3] batch slice of a batch-4 buffer."""
    G = 4
    H = HKV * G
    gen = torch.Generator().manual_seed(13)
    pos = [150, 37]
    kc, vc = _nan_caches(D, pos, gen, append=True, batch_buf=4, b0=1)
    qkv = _randn(B, 1, (H + 2 * HKV) * D, gen=gen).view(B, -1)
    q = qkv[:, :H * D].view(B, H, D)
    kn = qkv[:, H * D:(H + HKV) * D].view(B, HKV, D)
    vn = qkv[:, (H + HKV) * D:].view(B, HKV, D)
    assert not q.is_contiguous() and not kc.is_contiguous()
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    kr, vr = _cpu(kc), _cpu(vc)
    want = ref.decode_attention(_cpu(q), kr, vr, pt.cpu(), k_new=_cpu(kn),
                                v_new=_cpu(vn), rope_theta=THETA)
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn, splits=2,
                               rope_theta=THETA)
    _check(out, want)
    for b in range(B):
        _check_k_row(kc[b, :, pos[b]], kr[b, :, pos[b]])
        assert torch.equal(_bits(vc[b, :, pos[b]]), _bits(vn[b]))


def test_unsupported_groupings_are_refused():
    gen = torch.Generator().manual_seed(1)
    pt = torch.tensor([3], dtype=torch.long, device="cuda")
    c = _randn(B, HKV, 16, 64, gen=gen)
    with pytest.raises(ValueError):          # H % Hkv != 0
        ops.decode_attention(_randn(B, HKV * 2 + 1, 64, gen=gen), c,
                             c.clone(), pt)
    with pytest.raises(ValueError):          # G = 3
        ops.decode_attention(_randn(B, HKV * 3, 64, gen=gen), c, c.clone(),
                             pt)
    q = _randn(B, HKV * 2, 64, gen=gen)
    with pytest.raises(ValueError):          # k_new with H heads
        ops.decode_attention(q, c, c.clone(), pt, k_new=q.clone(),
                             v_new=q.clone())


def test_graph_replay():
    """One captured append + rope call replayed while the device position
    advances across a row-group/wave boundary (127 -> 128)."""
    D, G, p0 = 64, 4, 125
    H = HKV * G
    gen = torch.Generator().manual_seed(17)
    kc, vc = _nan_caches(D, [p0, p0], gen, append=True)
    kr, vr = _cpu(kc), _cpu(vc)
    q = _randn(B, H, D, gen=gen)
    kn, vn = (_randn(B, HKV, D, gen=gen) for _ in range(2))
    pos = torch.full((1,), p0, dtype=torch.long, device="cuda")

    def refill():
        q.copy_(_randn(B, H, D, gen=gen))
        for t in (kn, vn):
            t.copy_(_randn(B, HKV, D, gen=gen))

    def expect():
        return ref.decode_attention(_cpu(q), kr, vr, pos.cpu(),
                                    k_new=_cpu(kn), v_new=_cpu(vn),
                                    rope_theta=THETA)

    def call():
        return ops.decode_attention(q, kc, vc, pos, k_new=kn, v_new=vn,
                                    splits=2, rope_theta=THETA)

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
    assert torch.equal(vc[:, :, valid].float().cpu(), vr[:, :, valid])
    assert torch.equal(kc[:, :, :p0].float().cpu(), kr[:, :, :p0])
    # the five appended rows: the CPU cache holds the fp32 rotation rounded
    for p in range(p0, p0 + 5):
        _check_k_row(kc[:, :, p], kr[:, :, p])


def _engine_model():
    from tepdist_amd.models.llama import Llama, LlamaConfig
    cfg = LlamaConfig("decode-gqa-test", n_layer=2, n_embd=256, n_head=4,
                      n_ctx=64, vocab_size=503, n_kv_head=2)  # D 64, G 2
    torch.manual_seed(0)
    return cfg, Llama(cfg, dtype=BF16).cuda().eval()


def test_engine_step_fused_matches_composed():
    from tepdist_amd.inference import Generator
    cfg, model = _engine_model()
    gf = Generator(model, decode_attn="fused")
    gc = Generator(model, decode_attn="composed")
    Hkv, D, S0 = cfg.kv_heads, cfg.n_embd // cfg.n_head, 12
    G = cfg.n_head // Hkv
    ids = torch.randint(0, cfg.vocab_size, (2, S0 + 1), device="cuda")
    kc = [torch.zeros(2, Hkv, 32, D, dtype=BF16, device="cuda")
          for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    with torch.no_grad():
        gc._stack(gc._embed(ids[:, :S0], None), kc, vc, 0)
        x1 = gc._embed(ids[:, S0:], None)
        kf, vf = [t.clone() for t in kc], [t.clone() for t in vc]
        assert gf._fused_decode(x1, D, G) and not gc._fused_decode(x1, D, G)
        hf = gf._stack(x1, kf, vf, S0)
        hc = gc._stack(x1, kc, vc, S0)
    torch.cuda.synchronize()
    err = (hf.float() - hc.float()).abs().max().item()
    bound = 3e-2 * hc.float().abs().max().item()
    print(f"fused vs composed Llama step: max err {err:.3e}, bound "
          f"{bound:.3e}")
    assert err <= bound, (err, bound)
    # layer 0 sees identical inputs: its appended V rows are bit-equal and
    # its K rows agree to the rotation's rounding
    assert torch.equal(_bits(vf[0]), _bits(vc[0]))
    assert torch.equal(_bits(kf[0][:, :, :S0]), _bits(kc[0][:, :, :S0]))
    _check_k_row(kf[0][:, :, S0], kc[0][:, :, S0].float().cpu())


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
