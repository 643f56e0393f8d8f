"""ops.prefill_attention (prefill_attention.hip) on the MI355X against the
float64 oracle, per element: |got - fp64| <= 1 bf16 ulp + floor.

Oracle: per batch row the problem is embedded in the square causal one that
fp64_reference.attention_fwd solves: keys/values are cache rows 0 .. p0+T-1
as the kernel left them, queries are p0 zero rows followed by the T query
rows, and the last T rows are compared. The floor is flash_checks.fwd_floors'
`out` floor (the kernel has the flash forward's rounding points). With rope
the oracle rotates q in fp64 and does not round it; the kernel's one bf16
rounding of the rotated q (2^-8 relative per element, plus 4 U for its fp32
rotation) moves a scaled score by at most D_i = (2^-8 + 4U) scale max_j
sum_d |q_id||k_jd|, hence a probability by a factor within exp(+-2 D_i), and
the floor grows by (exp(2 D_i) - 1) sum_j p_ij |v_j|. Appended K rows are held
to rowwise_checks' rope bound against fp64_reference.rope at p0 + t, V rows
are bit-equal.

Caches are [B, Hkv, p0_max + T + 70, D] and hold NaN in every row >= p0 + T
(with append also in rows p0 .. p0+T-1 before the call), so any use of a row
the call may not see turns the output NaN. Shapes: 128 MFMA rows per block =
128/G tokens, 64-row kv tiles."""

import math

import pytest
import torch

import flash_checks as fc
import rowwise_checks as rc
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, HKV, THETA, U = 2, 2, 10000.0, 2.0 ** -24
NAN = float("nan")
P0S = [(0, 200), (1, 65), (63, 64), (64, 0), (65, 1), (200, 63)]


def _roles(G):
    """one row, a partial wave, either side of a block edge, a ragged third
    block"""
    n = 128 // G
    return [1, 5, n - 1, n, n + 1, 2 * n + 3]


# every T role and every p0 with every G in {1, 4, 8} and every D; G = 2 once
CASES = [(D, G, T, P0S[(i + G) % 6]) for D in (64, 128) for G in (1, 4, 8)
         for i, T in enumerate(_roles(G))] + [(64, 2, 65, (63, 200))]
_cid = lambda c: f"D{c[0]}-G{c[1]}-T{c[2]}-p{c[3][0]}_{c[3][1]}"  # noqa: E731


def _inputs(D, G, T, p0, append, seed, v_int=False):
    """q, k_new, v_new [B,T,*,D], NaN caches valid in rows < p0 (append) or
    < p0 + T, positions; all on the GPU."""
    g = rc.gen(seed)
    s_max = max(p0) + T + 70
    q = rc.randn(g, B, T, HKV * G, D).cuda()
    kn, vn = (rc.randn(g, B, T, HKV, D).cuda() for _ in range(2))
    if v_int:
        vn = torch.randint(-8, 9, (B, T, HKV, D), generator=g).to(BF16).cuda()
    kc, vc = (torch.full((B, HKV, s_max, D), NAN, dtype=BF16, device="cuda")
              for _ in range(2))
    for b in range(B):
        n = p0[b] + (0 if append else T)
        kc[b, :, :n] = rc.randn(g, HKV, n, D).cuda()
        vc[b, :, :n] = torch.randint(-8, 9, (HKV, n, D), generator=g) \
            .to(BF16).cuda() if v_int else rc.randn(g, HKV, n, D).cuda()
    return q, kn, vn, kc, vc, torch.tensor(p0, device="cuda")


def _judge(out, q, kc, vc, p0, theta, what):
    """out [B,T,H,D] against the embedded square problem, per batch row."""
    _, T, H, D = q.shape
    G, scale = H // HKV, 1.0 / math.sqrt(D)
    for b in range(B):
        S = p0[b] + T
        q_sq = torch.zeros(S, H, D, dtype=torch.float64)
        q_sq[p0[b]:] = o.f64(q[b])
        if theta is not None:
            q_sq, _ = o.rope(q_sq, S, theta)
        q_sq = q_sq.transpose(0, 1)[None]                      # [1,H,S,D]
        k, v = (o.f64(c[b, :, :S]).repeat_interleave(G, 0)[None]
                for c in (kc, vc))
        ref, rlse, p = o.attention_fwd(q_sq, k, v, True, scale)
        floor, _ = fc.fwd_floors(q_sq, k, v, True, scale, p, rlse)
        if theta is not None:
            dots = q_sq.abs() @ k.abs().transpose(-1, -2)
            dots = dots.masked_fill(torch.ones(S, S).triu(1).bool(), 0.0)
            delta = (2.0 ** -8 + 4 * U) * o.f32r(scale) \
                * dots.max(-1, keepdim=True).values
            floor = floor + torch.expm1(2 * delta) * (p @ v.abs())
        rc.judge(out[b].transpose(0, 1), ref[0, :, p0[b]:],
                 floor[0, :, p0[b]:], f"{what}[b={b}]")


@pytest.mark.parametrize("mode", ["plain", "append_rope"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_randn(case, mode):
    D, G, T, p0 = case
    append = mode != "plain"
    theta = THETA if append else None
    q, kn, vn, kc, vc, pos = _inputs(D, G, T, p0, append, D + G + T)
    out = ops.prefill_attention(q, kc, vc, pos, k_new=kn if append else None,
                                v_new=vn if append else None,
                                rope_theta=theta)
    assert out.shape == q.shape and out.is_contiguous()
    _judge(out, q, kc, vc, p0, theta, f"prefill.out[{_cid(case)} {mode}]")
    for b in range(B if append else 0):
        S = p0[b] + T
        x = torch.zeros(S, HKV, D, dtype=BF16)
        x[p0[b]:] = kn[b].cpu()
        want, ang = o.rope(x, S, THETA)
        rc.judge(kc[b, :, p0[b]:S].transpose(0, 1), want[p0[b]:],
                 rc.rope_floor(x, ang)[p0[b]:], f"prefill.k_rows[{_cid(case)}]")
        rc.assert_bits_equal(vc[b, :, p0[b]:S].transpose(0, 1), vn[b],
                             "appended V rows")
        assert torch.isnan(kc[b, :, S:].float()).all()


@pytest.mark.parametrize("append", [False, True], ids=["plain", "append"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_exact_counts(case, append):
    """q = 0 and integer V: every probability is exactly 1 / (p0 + t + 1) and
    out[t] is the bf16 rounding of the mean of V rows 0 .. p0 + t, which a mask
    off by one key misses. The kernel forms sum * (1 / n) in fp32 (the sum is
    exact), within 2^-22 of the mean, so where the mean is that close to a
    rounding boundary either neighbour is the rounding."""
    D, G, T, p0 = case
    q, kn, vn, kc, vc, pos = _inputs(D, G, T, p0, append, 7 + T, v_int=True)
    out = ops.prefill_attention(torch.zeros_like(q), kc, vc, pos,
                                k_new=kn if append else None,
                                v_new=vn if append else None).cpu()
    for b in range(B):
        S = p0[b] + T
        n = torch.arange(1, S + 1, dtype=torch.float64)[:, None]
        mean = (o.f64(vc[b, :, :S]).cumsum(1) / n)[:, p0[b]:]   # [Hkv,T,D]
        mean = mean.repeat_interleave(G, 0).transpose(0, 1)     # [T,H,D]
        lo, hi = ((mean * f).to(torch.float32).to(BF16)
                  for f in (1 - 2.0 ** -22, 1 + 2.0 ** -22))
        ok = (out[b] == lo) | (out[b] == hi)
        assert ok.all(), (f"b={b}: {int((~ok).sum())} elements are not the "
                          f"mean of rows 0..p0+t; first at "
                          f"{(~ok).nonzero()[0].tolist()}")


def test_packed_views_equal_contiguous_copies():
    D, G, T, p0 = 64, 4, 37, (65, 3)
    H = HKV * G
    q, kn, vn, kc, vc, pos = _inputs(D, G, T, p0, True, 5)
    qkv = torch.cat([t.reshape(B * T, -1) for t in (q, kn, vn)], 1)
    views = [t.view(B, T, -1, D) for t in
             qkv.split([H * D, HKV * D, HKV * D], 1)]
    assert not views[0].is_contiguous()
    kc2, vc2 = kc.clone(), vc.clone()
    a = ops.prefill_attention(q, kc, vc, pos, kn, vn, rope_theta=THETA)
    b = ops.prefill_attention(views[0], kc2, vc2, pos, views[1], views[2],
                              rope_theta=THETA)
    rc.assert_bits_equal(b, a, "out from views")
    rc.assert_bits_equal(kc2, kc, "k cache from views")
    rc.assert_bits_equal(vc2, vc, "v cache from views")


def test_position_is_clamped_and_rest_of_cache_untouched():
    D, G, T = 128, 2, 9
    q, kn, vn, kc, vc, _ = _inputs(D, G, T, (30, 30), True, 9)
    s_max = kc.shape[2]
    kc[:, :, :s_max - T] = 1.0          # a finite prefix under the clamp
    vc[:, :, :s_max - T] = 1.0
    big = torch.empty(B, HKV, s_max + 2, D, dtype=BF16, device="cuda")
    outs = []
    for p in (s_max, s_max - T):
        kb, vb = big.clone().fill_(3.0), big.clone().fill_(3.0)
        k1, v1 = kb[:, :, 1:-1], vb[:, :, 1:-1]   # guard rows around the cache
        k1.copy_(kc), v1.copy_(vc)
        pos = torch.tensor([p], device="cuda")
        outs.append((ops.prefill_attention(q, k1, v1, pos, kn, vn), kb, vb))
        for buf, src in ((kb, kc), (vb, vc)):
            assert (buf[:, :, 0] == 3).all() and (buf[:, :, -1] == 3).all()
            rc.assert_bits_equal(buf[:, :, 1:-1 - T], src[:, :, :s_max - T],
                                 "rows below p0")
    for x, y in zip(outs[0], outs[1]):
        rc.assert_bits_equal(x, y, "positions = S_max vs S_max - T")
    assert torch.isfinite(outs[0][0].float()).all()


def test_graph_replay_and_repeats_are_bit_equal():
    D, G, T = 64, 8, 21
    H = HKV * G
    g = rc.gen(3)
    steps = [[rc.randn(g, B, T, h, D).cuda() for h in (H, HKV, HKV)]
             for _ in range(3)]
    cache = lambda: [torch.zeros(B, HKV, 3 * T + 5, D, dtype=BF16,   # noqa
                                 device="cuda") for _ in range(2)]
    (kc, vc), (kc2, vc2) = cache(), cache()
    q, kn, vn = (t.clone() for t in steps[0])
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    run = lambda *a: ops.prefill_attention(*a, rope_theta=THETA)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = run(q, kc, vc, pos, kn, vn)
    torch.cuda.current_stream().wait_stream(side)
    rc.assert_bits_equal(run(q, kc2, vc2, pos, kn, vn), first, "repeat")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(q, kc, vc, pos, kn, vn)
    for i in (1, 2):
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.fill_(i * T)
        graph.replay()
        eager = run(*steps[i][:1], kc2, vc2, pos.clone(), *steps[i][1:])
        rc.assert_bits_equal(out, eager, f"replay {i}")
        rc.assert_bits_equal(kc, kc2, f"k cache after replay {i}")


@pytest.mark.parametrize("D,G", [(64, 8), (128, 4)])
def test_single_token_agrees_with_decode_attention(D, G):
    """Both kernels within the prefill bound of the shared fp64 value."""
    p0 = (200, 63)
    q, kn, vn, kc, vc, pos = _inputs(D, G, 1, p0, True, 21)
    kc2, vc2 = kc.clone(), vc.clone()
    a = ops.prefill_attention(q, kc, vc, pos, kn, vn, rope_theta=THETA)
    d = ops.decode_attention(q[:, 0], kc2, vc2, pos, k_new=kn[:, 0],
                             v_new=vn[:, 0], rope_theta=THETA)
    _judge(a, q, kc, vc, p0, THETA, "prefill T=1")
    _judge(d[:, None], q, kc2, vc2, p0, THETA, "decode")


def test_refusals():
    q, kn, vn, kc, vc, pos = _inputs(64, 2, 4, (3, 3), True, 1)
    bad = [
        dict(q=q.half(), kc=kc.half(), vc=vc.half(), kn=kn.half(),
             vn=vn.half()),                                    # fp16
        dict(q=q[..., :48].repeat(1, 1, 1, 2), kc=kc[..., :48].repeat(
            1, 1, 1, 2), vc=vc[..., :48].repeat(1, 1, 1, 2), kn=None,
            vn=None),                                          # D = 96
        dict(q=q[:, :, :3].repeat(1, 1, 2, 1)),                # G = 3
        dict(kc=kc[:, :, :3], vc=vc[:, :, :3]),                # T > S_max
        dict(vc=vc.transpose(1, 2).contiguous().transpose(1, 2)),  # strides
    ]
    for kw in bad:
        a = dict(q=q, kc=kc, vc=vc, kn=kn, vn=vn)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.prefill_attention(a["q"], a["kc"], a["vc"], pos, a["kn"],
                                  a["vn"])
