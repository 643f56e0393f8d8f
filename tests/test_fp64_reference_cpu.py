"""Proves the float64 oracles and the derived floors on the CPU.

1. ops/reference.py (fp32 math, bf16 outputs) runs through the same
   check_* functions, shapes and floors as tests/test_rowwise_edges_gpu.py
   and must stay within 1 ulp + floor, except for at most 1 element in
   10 000 per output (cancelled elements). More than that would mean a
   floor was derived wrong. (Dropout and the embedding gather are exact
   comparisons with no floor; the reference's dropout is not Philox, so
   the mask is proved through the port in part 3.)
2. Deliberately wrong variants of the fp32 formulas must FAIL the same
   assertion (and the unmutated formula must pass it), which puts the
   power of the bound on record.
3. The NumPy Philox port behind the dropout mask check.
"""

import math

import numpy as np
import pytest
import torch

import rowwise_checks as rc
from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import reference as ref

BF16 = torch.bfloat16
CAP = 1e-4


# --------------------------------------------------------------------------
# 1. the fp32 reference inside the GPU tests' floors
# --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ln", "add", "add_dsum"])
@pytest.mark.parametrize("cols", rc.NORM_COLS)
def test_reference_layernorm(cols, mode):
    rc.check_layernorm(ref, "cpu", 9, cols, mode=mode, cap=CAP)


@pytest.mark.parametrize("rows,gamma", [(1, "near1"), (9, "randn"),
                                        (1030, "near1"), (1030, "randn"),
                                        (8200, "near1")])
def test_reference_layernorm_rows(rows, gamma):
    for mode in ("ln", "add", "add_dsum"):
        rc.check_layernorm(ref, "cpu", rows, 72, gamma=gamma, mode=mode,
                           cap=CAP)


@pytest.mark.parametrize("cols", rc.NORM_COLS)
def test_reference_rmsnorm(cols):
    rc.check_rmsnorm(ref, "cpu", 9, cols, cap=CAP)


@pytest.mark.parametrize("rows,gamma", [(1, "near1"), (9, "randn"),
                                        (8200, "near1"), (8200, "randn")])
def test_reference_rmsnorm_rows(rows, gamma):
    rc.check_rmsnorm(ref, "cpu", rows, 72, gamma=gamma, cap=CAP)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("sq,sk", rc.SOFTMAX_SHAPES)
def test_reference_softmax(sq, sk, causal):
    rc.check_softmax(ref, "cpu", 3, sq, sk, causal, cap=CAP)


@pytest.mark.parametrize("kind,bh", [("pm80", 3), ("const", 3),
                                     ("randn", 114)])
def test_reference_softmax_inputs(kind, bh):
    for causal in (True, False):
        rc.check_softmax(ref, "cpu", bh, 72, 72, causal,
                         scale=1.0 if kind == "pm80" else 0.125, kind=kind,
                         cap=CAP)


def test_reference_softmax_more_queries_than_keys():
    # as hip.softmax_fwd: fine without the mask, refused with it
    rc.check_softmax(ref, "cpu", 3, 9, 5, causal=False, cap=CAP)
    with pytest.raises(ValueError, match="sq <= sk"):
        ref.softmax_fwd(rc.softmax_scores(3, 9, 5), scale=1.0, causal=True)


@pytest.mark.parametrize("pattern", rc.CE_PATTERNS)
@pytest.mark.parametrize("rows,cols", rc.CE_SHAPES)
def test_reference_cross_entropy(rows, cols, pattern):
    rc.check_cross_entropy(ref, "cpu", rows, cols, pattern, cap=CAP)


@pytest.mark.parametrize("n,dim,vocab,pattern", [
    (4096, 8, 16, "equal"), (100, 100, 101, "distinct"),
    (8200, 64, 300, "random"), (600, 1026, 50, "random")])
def test_reference_embedding_bwd(n, dim, vocab, pattern):
    rc.check_embedding_bwd(ref, "cpu", n, dim, vocab, pattern, cap=CAP)


@pytest.mark.parametrize("rows,cols", rc.BIAS_SHAPES)
def test_reference_bias_sum(rows, cols):
    rc.check_bias_sum(lambda t: t.float().sum(0).to(BF16), "cpu", rows, cols,
                      cap=CAP)


@pytest.mark.parametrize("n", rc.ELEMWISE_N + [8 * 2 ** 20 + 3])
def test_reference_gelu(n):
    rc.check_gelu(ref, "cpu", n, cap=CAP)


@pytest.mark.parametrize("n", rc.ELEMWISE_N + [4 * 2 ** 20 + 3])
def test_reference_swiglu(n):
    rc.check_swiglu(ref, "cpu", n, cap=CAP)


@pytest.mark.parametrize("theta", [10000.0, 500000.0])
@pytest.mark.parametrize("tokens,heads,D,seq_len", [
    (64, 1, 64, 64), (100, 4, 128, 33), (2048, 4, 64, 2048),
    (2048, 1, 128, 2048), (8200, 4, 64, 2048)])
def test_reference_rope(tokens, heads, D, seq_len, theta):
    rc.check_rope(ref, "cpu", tokens, heads, D, seq_len, theta, cap=CAP)


@pytest.mark.parametrize("n", [3, 10007, 2 * 2 ** 20 + 1])
def test_reference_adamw(n):
    rc.check_adamw_single(ref, "cpu", n, cap=CAP)


# --------------------------------------------------------------------------
# 2. mutations: each wrong variant must fail the assertion
# --------------------------------------------------------------------------

def _ln32(x, g, b, eps, div_extra=0):
    x32 = x.float()
    mean = x32.sum(-1) / (x.shape[-1] + div_extra)
    var = (x32 - mean[:, None]).pow(2).sum(-1) / x.shape[-1]
    rstd = torch.rsqrt(var + eps)
    y = (x32 - mean[:, None]) * rstd[:, None] * g.float() + b.float()
    return y.to(BF16), mean, rstd


def _ln_y_floor(x, g, b, rmean, rrstd):
    x64, mabs = o.f64(x), o.f64(x).abs().mean(-1)
    return rc.ELEM * (o.f64(g).abs() * rrstd[:, None]
                     * (x64.abs() + rmean.abs()[:, None] + mabs[:, None])
                     + o.f64(b).abs())


def _ln_inputs(rows=9, cols=72):
    g = rc.gen(5)
    return (rc.randn(g, rows, cols, scale=1.5, shift=0.5),
            rc.randn(g, cols, scale=0.1, shift=1.0),
            rc.randn(g, cols, scale=0.5), rc.randn(g, rows, cols))


def _mut_ln_fwd(eps=1e-5, div_extra=0):
    x, g, b, _ = _ln_inputs()
    ry, rmean, rrstd = o.layernorm_fwd(x, g, b, 1e-5)
    y, _, _ = _ln32(x, g, b, eps, div_extra)
    o.assert_within_ulp(y, ry, _ln_y_floor(x, g, b, rmean, rrstd), "ln.y")


def _mut_rms(with_eps=True):
    # eps only matters where mean(x^2) is not far above it
    gen = rc.gen(6)
    x = rc.randn(gen, 9, 72, scale=2.0 ** -10)
    g = rc.randn(gen, 72, scale=0.1, shift=1.0)
    ry, rrstd = o.rmsnorm_fwd(x, g, 1e-6)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + (1e-6 if with_eps else 0.0))
    y = (xf * rstd[:, None] * g.float()).to(BF16)
    o.assert_within_ulp(y, ry, rc.ELEM * ry.abs(), "rms.y")


def _mut_softmax_causal(shift=0):
    x = rc.softmax_scores(3, 5, 9)
    s32 = x.float() * 0.125
    mask = torch.ones(5, 9, dtype=torch.bool).tril(9 - 5 + shift)
    p = torch.softmax(s32.masked_fill(~mask, -math.inf), -1).to(BF16)
    rp = o.softmax_fwd(x, 0.125, True)
    o.assert_within_ulp(p, rp, rp * rc.ELEM + rc.FTZ, "softmax.p")


def _mut_softmax_max(subtract=True, amp=80.0):
    x = (rc.softmax_scores(3, 72, 72, "pm80").float() * (amp / 80)).to(BF16)
    s32 = x.float()
    if subtract:
        s32 = s32 - s32.max(-1, keepdim=True).values
    e = s32.exp()
    p = (e / e.sum(-1, keepdim=True)).to(BF16)
    rp = o.softmax_fwd(x, 1.0, False)
    o.assert_within_ulp(p, rp, rp * (1.4427 * 2 * amp * rc.U + rc.ELEM)
                        + rc.FTZ, "softmax.p")


def _mut_ce_bwd(onehot=True):
    gen = rc.gen(8)
    logits = rc.randn(gen, 9, 520, scale=3.0)
    t = torch.randint(0, 520, (9,), generator=gen)
    _, lse64, _ = o.cross_entropy_fwd(logits, t)
    lse = lse64.float()
    p = torch.exp(logits.float() - lse[:, None])
    if onehot:
        p[torch.arange(9), t] -= 1.0
    dl = (p * (1.0 / 9)).to(BF16)
    rdl, dscale = o.cross_entropy_bwd(torch.tensor(1.0), logits, t, lse)
    o.assert_within_ulp(dl, rdl, dscale * 16 * rc.U, "ce.dlogits")


def _mut_ln_bwd(drop_last_row=False, drop_c2=False):
    x, g, _, dy = _ln_inputs()
    _, mean, rstd = ref.layernorm_fwd(x, g, g)
    x32, dy32 = x.float(), dy.float()
    xhat = (x32 - mean[:, None]) * rstd[:, None]
    gg = dy32 * g.float()
    c1 = gg.mean(-1, keepdim=True)
    c2 = (gg * xhat).mean(-1, keepdim=True)
    dx = ((gg - c1 - (0 if drop_c2 else xhat * c2)) * rstd[:, None]).to(BF16)
    t = dy32 * xhat
    dg = (t[:-1] if drop_last_row else t).sum(0).to(BF16)
    rdx, rdg, _ = o.layernorm_bwd(dy, x, g, mean, rstd)
    xh64 = (o.f64(x) - o.f64(mean)[:, None]) * o.f64(rstd)[:, None]
    gg64 = o.f64(dy) * o.f64(g)
    fl = rc.ELEM * o.f64(rstd)[:, None] * (
        gg64.abs() + gg64.abs().mean(-1, keepdim=True)
        + xh64.abs() * (gg64 * xh64).abs().mean(-1, keepdim=True))
    o.assert_within_ulp(dx, rdx, fl, "ln.dx")
    o.assert_within_ulp(dg, rdg, 9 * rc.U
                        * (o.f64(dy) * xh64).abs().sum(0), "ln.dgamma")


def _rope32(x, seq_len, theta, shift=0, sign=1.0):
    T, H, D = x.shape
    pos = ((torch.arange(T) % seq_len) + shift).float()
    freq = theta ** (-2.0 * torch.arange(D // 2).float() / D)
    ang = pos[:, None] * freq[None, :]
    c, s = ang.cos()[:, None, :], sign * ang.sin()[:, None, :]
    x1, x2 = x.float()[..., :D // 2], x.float()[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(BF16)


def _mut_rope(shift=0, bwd_sign=-1.0):
    x = rc.randn(rc.gen(9), 100, 2, 64)
    ry, ang = o.rope(x, 33, 10000.0)
    o.assert_within_ulp(_rope32(x, 33, 10000.0, shift), ry,
                        rc.rope_floor(x, ang), "rope.fwd")
    rdx, _ = o.rope(x, 33, 10000.0, backward=True)
    o.assert_within_ulp(_rope32(x, 33, 10000.0, 0, bwd_sign), rdx,
                        rc.rope_floor(x, ang), "rope.bwd")


def _mut_swiglu(swap=False):
    gen = rc.gen(10)
    a, b, dy = (rc.randn(gen, 2055) for _ in range(3))
    da, db = ref.swiglu_bwd(dy, a, b)
    if swap:
        da, db = db, da
    rda, rdb = o.swiglu_bwd(dy, a, b)
    big = o.f64(a).abs().clamp_min(1.0)
    o.assert_within_ulp(da, rda, rc.ELEM * big * (o.f64(dy) * o.f64(b)).abs(),
                        "swiglu.da")
    o.assert_within_ulp(db, rdb, rc.ELEM * big * o.f64(dy).abs(), "swiglu.db")


def _mut_adamw(eps_inside=False):
    hp = rc.ADAMW_HP
    gen = rc.gen(11)
    n, step = 10007, 2
    master = torch.randn(n, generator=gen)
    m0 = torch.randn(n, generator=gen) * 1e-3
    v0 = torch.rand(n, generator=gen) * 1e-6
    grad = rc.adamw_grad(gen, n, torch.float32)
    m = hp["beta1"] * m0 + (1 - hp["beta1"]) * grad
    v = hp["beta2"] * v0 + (1 - hp["beta2"]) * grad * grad
    bc1, bc2 = 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step
    if eps_inside:      # eps divided by sqrt(bc2) along with sqrt(v)
        denom = (v.sqrt() + hp["eps"]) / math.sqrt(bc2)
    else:
        denom = (v / bc2).sqrt() + hp["eps"]
    ma = master * (1 - hp["lr"] * hp["weight_decay"]) \
        - hp["lr"] * (m / bc1) / denom
    rc.adamw_judge((ma.to(BF16), ma, m, v), (master, m0, v0), grad, hp, step,
                   "[mutation]")


MUTATIONS = {
    "ln_eps_1e-3": (_mut_ln_fwd, {}, {"eps": 1e-3}),
    "ln_mean_over_cols_plus_1": (_mut_ln_fwd, {}, {"div_extra": 1}),
    "rms_without_eps": (_mut_rms, {}, {"with_eps": False}),
    "softmax_causal_limit_plus_1": (_mut_softmax_causal, {}, {"shift": 1}),
    "softmax_causal_limit_minus_1": (_mut_softmax_causal, {}, {"shift": -1}),
    # at +-96, not +-80: fp32 holds exp(80) = 5.5e34 and 2048 of them, so
    # without the max the +-80 rows still come out right to the bound (see
    # test_softmax_without_max_is_still_right_at_pm80); exp(88.8) is the
    # first to overflow
    "softmax_no_max_subtraction_pm96": (_mut_softmax_max, {"amp": 96.0},
                                        {"subtract": False, "amp": 96.0}),
    "ce_bwd_without_onehot": (_mut_ce_bwd, {}, {"onehot": False}),
    "dgamma_missing_last_row": (_mut_ln_bwd, {}, {"drop_last_row": True}),
    "dx_missing_c2": (_mut_ln_bwd, {}, {"drop_c2": True}),
    "rope_pos_plus_1": (_mut_rope, {}, {"shift": 1}),
    "rope_bwd_sign_not_flipped": (_mut_rope, {}, {"bwd_sign": 1.0}),
    "swiglu_bwd_da_db_swapped": (_mut_swiglu, {}, {"swap": True}),
    "adamw_eps_scaled_by_bc2": (_mut_adamw, {}, {"eps_inside": True}),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_fails_the_bound(name):
    fn, good, bad = MUTATIONS[name]
    fn(**good)                       # the correct fp32 formula passes
    with pytest.raises(AssertionError, match="outside 1 ulp"):
        fn(**bad)


def test_softmax_without_max_is_still_right_at_pm80():
    """On record because the +-80 case was expected to expose a missing
    max subtraction: in fp32 it cannot. exp(80) = 5.5e34 and a row of 2048
    of them sums to 1.1e38, under the fp32 maximum 3.4e38, and the -80
    entries' true probabilities (< 1e-69) are below the flush-to-zero
    floor either way. The bound is not blind here; the variant is not
    wrong until the inputs reach +-88.8 (the pm96 mutation above)."""
    _mut_softmax_max(subtract=False, amp=80.0)
    assert math.exp(80.0) * 2048 < torch.finfo(torch.float32).max


def test_checker_reports_worst_element():
    ref64 = torch.tensor([[1.0, 2.0], [3.0, -4.0]], dtype=torch.float64)
    got = ref64.to(BF16).clone()
    o.assert_within_ulp(got, ref64, 0.0, "exact")
    got[1, 0] = 3.0 + 2 * 2.0 ** -6          # 2 ulp at 3.0
    with pytest.raises(AssertionError) as e:
        o.assert_within_ulp(got, ref64, 0.0, "probe")
    msg = str(e.value)
    assert "probe" in msg and "(1, 0)" in msg and "2.000 ulp" in msg
    # exactly one ulp passes, the floor is added on top, NaN fails
    got[1, 0] = 3.0 + 2.0 ** -6
    o.assert_within_ulp(got, ref64, 0.0, "one ulp")
    got[1, 0] = 3.0 + 2 * 2.0 ** -6
    o.assert_within_ulp(got, ref64, 2.0 ** -6, "floor")
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        o.assert_within_ulp(got, ref64, 1.0, "nan")
    # fp32 outputs: 2^-23 relative
    f = torch.tensor([1.0 + 2.0 ** -22])
    with pytest.raises(AssertionError):
        o.assert_within_ulp(f, torch.ones(1, dtype=torch.float64), 0.0, "f32")
    o.assert_within_ulp(torch.tensor([1.0 + 2.0 ** -23]),
                        torch.ones(1, dtype=torch.float64), 0.0, "f32")
    assert o.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, -96.0],
                                   dtype=torch.float64)).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.5]


# --------------------------------------------------------------------------
# 3. the NumPy Philox port
# --------------------------------------------------------------------------

def _philox_scalar(ctr, key):
    """The same round written with Python integers. It checks only the
    uint64 vectorisation of the port (masking, the 32 x 32 bit products),
    not the algorithm or its constants: what validates those is the
    bit-for-bit comparison of the port with the mask the HIP kernel writes,
    in tests/test_rowwise_edges_gpu.py."""
    M = 0xFFFFFFFF
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1],
             p0 & M]
        k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
    return c


def test_philox_port_matches_scalar():
    for ctr, key in [((0, 0, 0, 0), (0, 0)),
                     ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)),
                     ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                      (0xA4093822, 0x299F31D0))]:
        got = o.philox4x32_10([np.array([c]) for c in ctr], key)
        assert [int(w[0]) for w in got] == _philox_scalar(ctr, key)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_philox_mask_keep_rate(p):
    n = 2 ** 20
    keep = o.dropout_mask(n, p, seed=(7 << 32) + 12345, offset=3).sum()
    sigma = math.sqrt(n * p * (1 - p))
    assert abs(int(keep) - n * (1 - p)) <= 4 * sigma, (int(keep), sigma)


def test_philox_mask_offsets_and_length():
    seed = (1 << 40) + 99
    a = o.dropout_mask(4099, 0.5, seed, 0)
    b = o.dropout_mask(4099, 0.5, seed, 1)
    assert (a != b).mean() > 0.4            # independent streams
    assert (o.dropout_mask(4099, 0.5, seed + 1, 0) != a).mean() > 0.4
    # element i does not depend on n (nor on n % 4)
    for n in (1, 3, 4, 5, 1023):
        assert np.array_equal(o.dropout_mask(n, 0.5, seed, 0), a[:n])
    assert a.dtype == np.uint8 and set(np.unique(a)) <= {0, 1}
