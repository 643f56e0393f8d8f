"""ops.decode_attention / ops.prefill_attention over an MXFP8 KV cache
(mx.MXCache) on the MI355X. Harness of test_decode_attention_gqa_gpu.py:
B = 2, Hkv = 3, caches are [:, :, :203] views of 256-row buffers; outside the
valid rows every code is 0x7f (NaN) and every scale byte 255, so a finite
output proves that nothing invalid was used.

Decode outputs: max|out - ref| <= 1e-2 * max(1, max|ref|), the bf16 file's
bound: ref is the fp32 reference op on the dequantized cache (exact values,
so quantization is no part of the kernel's error), with append on the cache
as the kernel left it, so it holds whichever way a code fell.

Appended rows: V rows, K rows without rope and K rows at p = 0 equal
mx.mx_quantize of the operand byte for byte. With rope, dq(stored) against
dq(mx_quantize(bf16(fp32 CPU rotation))) within 2^-3 (1 + 2^-7) amax of the
block: a rotation differing in the last fp32 bits moves the bf16 rounding by
one ulp, which can flip a code or the block's scale by one e4m3 step, at most
32 scale units against an amax >= 255 (largest ratio over 12.8 M perturbed
elements on the CPU: 0.12549 = 32 / 255).

Prefill: _judge of test_prefill_attention_gpu.py (fp64 oracle, per-element
bound; hence its Hkv = 2) on the dequantized post-call cache."""

import math

import pytest
import torch

from test_prefill_attention_gpu import HKV as P_HKV, _judge
from tepdist_amd import ops
from tepdist_amd.ops import mx
from tepdist_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, HKV, S_MAX, S_BUF = 2, 3, 203, 256
THETA = 10000.0
GROUPS = [1, 2, 4, 8]
POS = [[0, 202], [15, 16], [63, 64], [127, 128]]
_pid = lambda p: f"p{p[0]}_{p[1]}"        # noqa: E731


def _randn(*shape, gen):
    return torch.randn(*shape, generator=gen).to(BF16).cuda()


def _caches(D, n_valid, gen, batch_buf=B, b0=0, s_max=S_MAX, s_buf=S_BUF,
            hkv=HKV):
    """K and V MXCache views whose rows < n_valid[b] hold mx_quantize(randn)
    and every other row of the buffers NaN codes and scale byte 255."""
    out = []
    for _ in range(2):
        codes = torch.full((batch_buf, hkv, s_buf, D), 0x7f,
                           dtype=torch.uint8, device="cuda")
        scales = torch.full((batch_buf, hkv, s_buf, D // 32), 255,
                            dtype=torch.uint8, device="cuda")
        c = mx.MXCache(codes[b0:b0 + B, :, :s_max],
                       scales[b0:b0 + B, :, :s_max])
        for b, n in enumerate(n_valid):
            w = mx.mx_quantize(torch.randn(hkv * n, D, generator=gen), "mxfp8")
            c.codes[b, :, :n] = w.codes.view(hkv, n, D).cuda()
            c.scales[b, :, :n] = w.scales.view(hkv, n, D // 32).cuda()
        out.append(c)
    return out


def _dq(c):
    """fp32 CPU copy of the dequantized cache."""
    torch.cuda.synchronize()
    return mx.cache_dequantize(c.to("cpu")).float()


def _check(out, want):
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert got.shape == want.shape and out.dtype == BF16
    assert torch.isfinite(got).all(), "an invalid (NaN) row was used"
    err = (got - want).abs().max().item()
    bound = 1e-2 * max(1.0, want.abs().max().item())
    assert err <= bound, f"max err {err} > {bound}"


def _bases(kc, vc):
    return [t._base.clone() for c in (kc, vc) for t in (c.codes, c.scales)]


def _same_but_rows(before, kc, vc, pos, T=1):
    """The four whole buffers equal `before` but in rows pos[b] .. + T - 1."""
    after = _bases(kc, vc)
    for b, p in enumerate(pos):
        for t in before + after:
            t[b, :, p:p + T] = 0
    assert all(torch.equal(t0, t1) for t0, t1 in zip(before, after))


def _check_rows(c, b, rows, x32, exact):
    """Cache rows `rows` (a slice) of batch row b against mx_quantize of x32
    [n, Hkv, D] (fp32, CPU) rounded to bf16: byte for byte, or (rotated K)
    within the bound of the module docstring."""
    n, hkv, D = x32.shape
    w = mx.mx_quantize(x32.to(BF16).reshape(-1, D), "mxfp8")
    codes = c.codes[b, :, rows].transpose(0, 1).reshape(-1, D).cpu()
    scales = c.scales[b, :, rows].transpose(0, 1).reshape(-1, D // 32).cpu()
    if exact:
        assert torch.equal(codes, w.codes) and torch.equal(scales, w.scales)
        return
    got = mx.dequantize_ref(mx.MXWeight(codes, scales, "mxfp8", w.shape))
    want = mx.dequantize_ref(w).float().view(-1, D // 32, 32)
    err = (got.float().view_as(want) - want).abs().amax(-1)
    bound = 2.0 ** -3 * (1 + 2.0 ** -7) * want.abs().amax(-1)
    assert (err <= bound).all(), (err.max().item(), bound.min().item())


def _check_new_rows(kc, vc, pos, kn, vn, theta, T=1):
    """The T rows appended at pos[b] (kn, vn [B, T, Hkv, D])."""
    for b, p in enumerate(pos):
        rows = torch.arange(p, p + T)
        k32 = kn[b].float().cpu()
        if theta is not None:
            k32 = ref._rope_at_f32(k32, rows[:, None], theta)
        _check_rows(vc, b, slice(p, p + T), vn[b].float().cpu(), True)
        if theta is None or (p == 0 and T == 1):
            _check_rows(kc, b, slice(p, p + T), k32, True)
        else:
            _check_rows(kc, b, slice(p, p + T), k32, False)
            if p == 0:
                _check_rows(kc, b, slice(0, 1), k32[:1], True)


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("pos", POS, ids=_pid)
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_numerics(G, D, splits, pos, rope):
    gen = torch.Generator().manual_seed(G * 1000 + D + splits)
    theta = THETA if rope else None
    kc, vc = _caches(D, [p + 1 for p in pos], gen)
    q = _randn(B, HKV * G, D, gen=gen)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    want = ref.decode_attention(q.float().cpu(), _dq(kc), _dq(vc), pt.cpu(),
                                rope_theta=theta)
    out = ops.decode_attention(q, kc, vc, pt, splits=splits,
                               rope_theta=theta)
    _check(out, want)
    again = ops.decode_attention(q, kc, vc, pt, splits=splits,
                                 rope_theta=theta)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("pos", POS, ids=_pid)
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_append(G, D, splits, pos, rope):
    """Row p holds NaN codes before the call and is the quantized new row
    after it; no other byte of the buffers changes."""
    gen = torch.Generator().manual_seed(11 + splits + G)
    theta = THETA if rope else None
    kc, vc = _caches(D, pos, gen)
    q = _randn(B, HKV * G, D, gen=gen)
    kn, vn = (_randn(B, HKV, D, gen=gen) for _ in range(2))
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    before = _bases(kc, vc)
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                               splits=splits, rope_theta=theta)
    want = ref.decode_attention(q.float().cpu(), _dq(kc), _dq(vc), pt.cpu(),
                                rope_theta=theta)
    _check(out, want)
    _check_new_rows(kc, vc, pos, kn[:, None], vn[:, None], theta)
    _same_but_rows(before, kc, vc, pos)


DS = lambda D: [0, 7, 8, 31, 32, D - 1]   # noqa: E731
ROWS = [190, 5, 75, 150, 40, 100, 120, 180]


@pytest.mark.parametrize("kind", ["aligned", "onehot"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_placement(G, D, kind):
    """Every query returns one V row to one bf16 rounding: V codes cycle
    through every non-NaN code, V scale bytes change with row and block.
    aligned: member g's query is aligned with K row ROWS[g], one in the last
    of 3 splits. onehot: query i is 16 sqrt(D) at d = DS[i % 6]; all K are 1
    except, per d, a winner row (code 2.0 under byte 129: 8, its block's
    other elements 4) and a decoy (code 8.0 under byte 125: 2), so a wrong
    byte, lane or scale picks another row or ties. The logit gap is >= 60:
    the other 202 rows add at most 202 e^-60 max|V| (an element whose own V
    is zero is not exactly zero)."""
    gen = torch.Generator().manual_seed(7 + G)
    pos, H = [202, 202], HKV * G
    kc, vc = _caches(D, [203, 203], gen)
    good = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f],
                        dtype=torch.uint8)
    r, d = torch.arange(S_MAX)[:, None], torch.arange(D)[None, :]
    for h in range(HKV):
        vc.codes[:, h] = good[(r * D + d + h) % 254].cuda()
        vc.scales[:, h] = (120 + (r + torch.arange(D // 32) + h) % 14) \
            .to(torch.uint8).cuda()
    if kind == "aligned":
        q = _randn(B, H, D, gen=gen)
        qn = q.float().cpu().view(B, HKV, G, D)
        own = torch.tensor(ROWS[:G]).expand(B, HKV, G)
        for g in range(G):
            k = 16.0 * math.sqrt(D) * qn[:, :, g] / \
                qn[:, :, g].norm(dim=-1, keepdim=True)
            w = mx.mx_quantize(k.reshape(-1, D), "mxfp8")
            kc.codes[:, :, ROWS[g]] = w.codes.view(B, HKV, D).cuda()
            kc.scales[:, :, ROWS[g]] = w.scales.view(B, HKV, D // 32).cuda()
    else:
        kc.codes[:] = 0x38
        kc.scales[:] = 127
        for i, dd in enumerate(DS(D)):
            kc.codes[:, :, ROWS[i], dd] = 0x40
            kc.scales[:, :, ROWS[i], dd // 32] = 129
            kc.codes[:, :, ROWS[i] + 1, dd] = 0x50
            kc.scales[:, :, ROWS[i] + 1, dd // 32] = 125
        which = torch.arange(B * H) % 6
        q = torch.zeros(B * H, D)
        q[torch.arange(B * H), torch.tensor(DS(D))[which]] = 16 * math.sqrt(D)
        q = q.to(BF16).cuda().view(B, H, D)
        own = torch.tensor(ROWS)[which].view(B, HKV, G)
    kd, vd = _dq(kc), _dq(vc)
    s = torch.einsum("bhgd,bhsd->bhgs", q.float().cpu().view(B, HKV, G, D),
                     kd) / math.sqrt(D)
    top = s.gather(-1, own[..., None])
    gap = (top - s.masked_fill(torch.arange(S_MAX) == own[..., None],
                               -math.inf).amax(-1, keepdim=True)).min()
    assert gap >= 60, gap
    out = ops.decode_attention(q, kc, vc, torch.tensor(pos, device="cuda"),
                               splits=3)
    want = vd.gather(2, own[..., None].expand(B, HKV, G, D)).view(B, H, D)
    err = (out.float().cpu() - want).abs()
    floor = 202 * math.exp(-60) * vd[:, :, :S_MAX].abs().max()
    assert (err <= 2.0 ** -8 * want.abs() + floor).all(), err.max()


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("p0", [0, 70])
@pytest.mark.parametrize("T", [1, 5, 64, 129])
def test_prefill(T, p0, G, D, rope):
    gen = torch.Generator().manual_seed(T + p0 + G + D)
    theta = THETA if rope else None
    pos = [p0, 70 - p0]
    kc, vc = _caches(D, pos, gen, hkv=P_HKV)
    q = _randn(B, T, P_HKV * G, D, gen=gen)
    kn, vn = (_randn(B, T, P_HKV, D, gen=gen) for _ in range(2))
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    k1, v1, before = kc.clone(), vc.clone(), _bases(kc, vc)
    out = ops.prefill_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                                rope_theta=theta)
    assert torch.isfinite(out.float()).all(), "an invalid (NaN) row was used"
    _judge(out, q, _dq(kc), _dq(vc), pos, theta, "prefill_mx.out")
    _check_new_rows(kc, vc, pos, kn, vn, theta, T)
    again = ops.prefill_attention(q, kc, vc, pt, k_new=kn, v_new=vn,
                                  rope_theta=theta)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    _same_but_rows(before, kc, vc, pos, T)
    if T == 1:      # the decode op on the same inputs, same bound
        od = ops.decode_attention(q[:, 0], k1, v1, pt, k_new=kn[:, 0],
                                  v_new=vn[:, 0], rope_theta=theta)
        _judge(od[:, None], q, _dq(k1), _dq(v1), pos, theta, "decode_mx.out")


@pytest.mark.parametrize("D", [64, 128])
def test_strided_operands(D):
    """Operands as views of the packed projection, caches a batch slice."""
    G = 4
    H = HKV * G
    gen = torch.Generator().manual_seed(13)
    pos = [150, 37]
    kc, vc = _caches(D, pos, gen, batch_buf=4, b0=1)
    qkv = _randn(B, (H + 2 * HKV) * D, gen=gen)
    q = qkv[:, :H * D].view(B, H, D)
    kn = qkv[:, H * D:(H + HKV) * D].view(B, HKV, D)
    vn = qkv[:, (H + HKV) * D:].view(B, HKV, D)
    pt = torch.tensor(pos, dtype=torch.long, device="cuda")
    out = ops.decode_attention(q, kc, vc, pt, k_new=kn, v_new=vn, splits=2,
                               rope_theta=THETA)
    _check(out, ref.decode_attention(q.float().cpu(), _dq(kc), _dq(vc),
                                     pt.cpu(), rope_theta=THETA))
    _check_new_rows(kc, vc, pos, kn[:, None], vn[:, None], THETA)


def test_graph_replay():
    """A captured append + rope call replayed across position 127 -> 128,
    every replay against the eager call on a twin cache."""
    D, G, p0 = 64, 4, 125
    H = HKV * G
    gen = torch.Generator().manual_seed(17)
    kc, vc = _caches(D, [p0, p0], gen)
    ke, ve = kc.clone(), vc.clone()         # the eager twin
    q = _randn(B, H, D, gen=gen)
    kn, vn = (_randn(B, HKV, D, gen=gen) for _ in range(2))
    pos = torch.full((1,), p0, dtype=torch.long, device="cuda")

    def call(k, v):
        return ops.decode_attention(q, k, v, pos, k_new=kn, v_new=vn,
                                    splits=2, rope_theta=THETA)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(kc.clone(), vc.clone())        # warm-up off the real caches
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(kc, vc)
    for i in range(5):
        if i:
            pos.add_(1)
            q.copy_(_randn(B, H, D, gen=gen))
            for t in (kn, vn):
                t.copy_(_randn(B, HKV, D, gen=gen))
        graph.replay()
        eager = call(ke, ve)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
        p = p0 + i
        _check(out, ref.decode_attention(
            q.float().cpu(), _dq(kc), _dq(vc), pos.cpu(), rope_theta=THETA))
        _check_new_rows(kc, vc, [p, p], kn[:, None], vn[:, None], THETA)
    assert torch.equal(kc.codes, ke.codes) and \
        torch.equal(vc.scales, ve.scales)


def test_refusals():
    gen = torch.Generator().manual_seed(1)
    pt = torch.tensor([3], dtype=torch.long, device="cuda")
    kc, vc = _caches(64, [16, 16], gen, s_max=16, s_buf=16)
    q = _randn(B, HKV * 2, 64, gen=gen)
    ops.decode_attention(q, kc, vc, pt)                     # covered
    bf = _randn(B, HKV, 16, 64, gen=gen)
    bad = mx.MXCache(vc.codes, vc.scales[..., :1])          # scale shape
    k96, v96 = _caches(96, [16, 16], gen, s_max=16, s_buf=16)
    for args in [(q, kc, bf), (q, bf, vc),                  # mixed pair
                 (_randn(B, HKV * 3, 64, gen=gen), kc, vc),  # G = 3
                 (_randn(B, HKV, 96, gen=gen), k96, v96),   # D = 96
                 (q, kc, bad)]:
        with pytest.raises(ValueError):
            ops.decode_attention(*args, pt)
        with pytest.raises(ValueError):
            ops.prefill_attention(args[0][:, None], *args[1:], pt)
