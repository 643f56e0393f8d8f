"""Cases, inputs and derived error floors shared by
test_fp64_reference_cpu.py (ops/reference.py on the CPU) and
test_rowwise_edges_gpu.py (the HIP kernels): both run the same check_*
functions, with the same seeded CPU inputs and the same floors, against the
float64 oracles of tepdist_amd/ops/fp64_reference.py.

The criterion is assert_within_ulp: |got - fp64| <= 1 ulp(fp64) + floor.
A correctly rounded result of an exact computation uses half an ulp; the
floor is what fp32 arithmetic may add on top. The floors start from
2^-20 (16 fp32 roundings, U = 2^-24 each) of what cancels:

  row ops    2^-20 * the magnitudes of the terms that are added or
             subtracted to form the output. Where nothing cancels this is
             2^-20 of the row's own values; it is kept relative to the
             terms, not to the result, because a result can cancel to far
             below them (RMSNorm dx at cols = 1 is t * eps / x^2, six
             orders under t, and fp32 can do no better than 2^-24 of t).
  columns    R * U * sum_r |term_r| for a sum over R rows in ANY order
             (per-wave partials, atomics).
  GELU and SwiGLU   2^-20 * max(1, |x|), times |dy| in the backward.
  RoPE       (|x1| + |x2|) * angle * 2^-20.

A term would be enlarged only where a kernel measurably exceeded it on the
GPU. None had to be: every kernel meets these floors (docs/KERNELS.md has
the measured figures).

`cap`: None asserts every element (the GPU tests). The CPU proof passes
1e-4: the fp32 reference must stay inside the same floors except for at
most 1 element in 10 000 per output.
"""

import math

import torch

from tepdist_amd.ops import fp64_reference as o

BF16 = torch.bfloat16
U = 2.0 ** -24
ELEM = 2.0 ** -20
FTZ = 2.0 ** -126     # fp32 results below the smallest normal may flush

# per output: the largest error seen, (in ulps over the elements whose floor
# is under 1/8 ulp, in ulps anywhere, as a fraction of the allowed error);
# fp32 outputs in units of 2^-23 relative. Filled by judge(cap=None).
MEASURED = {}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0, shift=0.0, dtype=BF16):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def judge(got, ref64, floor, what, cap=None):
    err, unit, tol = o.ulp_error(got, ref64, floor)
    if cap is not None:
        bad, allowed = int((~(err <= tol)).sum()), int(ref64.numel() * cap)
        assert bad <= allowed, (f"{what}: {bad} of {ref64.numel()} elements "
                                f"outside 1 ulp + floor, {allowed} allowed")
        return
    if err.numel() and torch.isfinite(err).all():
        ulps = torch.nan_to_num(err / unit, nan=0.0, posinf=0.0)
        frac = torch.where(err == 0, err, err / tol)
        plain = (tol - unit) <= unit / 8
        now = (float(ulps[plain].max()) if plain.any() else 0.0,
               float(ulps.max()), float(frac.max()))
        key = what.split("[")[0]
        MEASURED[key] = tuple(map(max, now, MEASURED.get(key, (0, 0, 0))))
    o.assert_within_ulp(got, ref64, floor, what)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_bits_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = bits(got), bits(want)
    if not torch.equal(g, w):
        i = int((g != w).reshape(-1).nonzero()[0])
        raise AssertionError(
            f"{what}: {int((g != w).sum())} of {g.numel()} elements differ, "
            f"first at flat index {i}: {got.reshape(-1)[i].item()!r} vs "
            f"{want.reshape(-1)[i].item()!r}")


# --------------------------------------------------------------------------
# LayerNorm, add + LayerNorm, RMSNorm
# --------------------------------------------------------------------------

NORM_COLS = [1, 7, 8, 9, 72, 511, 512, 513, 1280, 1600, 2560, 3071, 3072]


def _gamma(g, cols, kind):
    if kind == "randn":
        return randn(g, cols)
    return randn(g, cols, scale=0.1, shift=1.0)


def check_layernorm(be, dev, rows, cols, gamma="near1", mode="ln",
                    bwd=True, cap=None, eps=1e-5):
    """mode: 'ln', 'add' (add + LN, dsum None), 'add_dsum'."""
    g = gen(1000 * cols + rows)
    x = randn(g, rows, cols, scale=1.5, shift=0.5)
    gam, bet = _gamma(g, cols, gamma), randn(g, cols, scale=0.5)
    tag = f"[{mode} {rows}x{cols} {gamma}]"
    if mode == "ln":
        y, mean, rstd = be.layernorm_fwd(x.to(dev), gam.to(dev), bet.to(dev),
                                         eps)
        ry, rmean, rrstd = o.layernorm_fwd(x, gam, bet, eps)
        s = x
    else:
        res = randn(g, rows, cols, scale=2.0)
        s_dev, y, mean, rstd = be.add_layernorm_fwd(
            x.to(dev), res.to(dev), gam.to(dev), bet.to(dev), eps)
        s, ry, rmean, rrstd = o.add_layernorm_fwd(x, res, gam, bet, eps)
        assert_bits_equal(s_dev, s, "add_ln.sum" + tag)
    s64, g64, b64 = o.f64(s), o.f64(gam), o.f64(bet)
    mabs = s64.abs().mean(-1)
    # mean = sum / cols: 2^-20 of the summands' magnitudes
    judge(mean, rmean, ELEM * mabs, "ln_fwd.mean" + tag, cap)
    # var sums squares (no cancellation), then the -1/2 power and rsqrt's
    # own ulp: 2^-20 relative
    judge(rstd, rrstd, ELEM * rrstd, "ln_fwd.rstd" + tag, cap)
    # y = (x - mean) * rstd * g + b. Terms: x and mean (whose own error is
    # 2^-20 * mean|x|) scaled by rstd * |g|, and b.
    fl = ELEM * (g64.abs() * rrstd[:, None]
                * (s64.abs() + rmean.abs()[:, None] + mabs[:, None])
                + b64.abs())
    judge(y, ry, fl, "ln_fwd.y" + tag, cap)
    if not bwd:
        return
    dy = randn(g, rows, cols)
    dsum = randn(g, rows, cols) if mode == "add_dsum" else None
    sd, gd, dyd = s.to(dev), gam.to(dev), dy.to(dev)
    if mode == "ln":
        dx, dg, db = be.layernorm_bwd(dyd, sd, gd, mean, rstd)
    else:
        dx, dg, db = be.add_layernorm_bwd(
            dyd, None if dsum is None else dsum.to(dev), sd, gd, mean, rstd)
    # the oracle takes the statistics the backward was given
    rdx, rdg, rdb = o.layernorm_bwd(dy, s, gam, mean, rstd, dsum=dsum)
    rs = o.f64(rstd)[:, None]
    xhat = (s64 - o.f64(mean)[:, None]) * rs
    dy64 = o.f64(dy)
    gg = dy64 * g64
    # dx = (gg - c1 - xhat * c2) * rstd [+ dsum]; c1 = mean(gg) and c2 =
    # mean(gg * xhat) are row reductions: every term at 2^-20
    fl = ELEM * (rs * (gg.abs() + gg.abs().mean(-1, keepdim=True)
                      + xhat.abs() * (gg * xhat).abs().mean(-1, keepdim=True))
                + (0 if dsum is None else o.f64(dsum).abs()))
    judge(dx, rdx, fl, "ln_bwd.dx" + tag, cap)
    judge(dg, rdg, rows * U * (dy64 * xhat).abs().sum(0),
          "ln_bwd.dgamma" + tag, cap)
    judge(db, rdb, rows * U * dy64.abs().sum(0),
          "ln_bwd.dbeta" + tag, cap)


def check_rmsnorm(be, dev, rows, cols, gamma="near1", cap=None, eps=1e-6):
    g = gen(2000 * cols + rows)
    x = randn(g, rows, cols, scale=1.5, shift=0.5)
    gam = _gamma(g, cols, gamma)
    tag = f"[{rows}x{cols} {gamma}]"
    y, rstd = be.rmsnorm_fwd(x.to(dev), gam.to(dev), eps)
    ry, rrstd = o.rmsnorm_fwd(x, gam, eps)
    # as LayerNorm's rstd: a sum of squares, then the -1/2 power
    judge(rstd, rrstd, ELEM * rrstd, "rms_fwd.rstd" + tag, cap)
    # y = x * rstd * g: a product, its only error is relative (rstd's)
    judge(y, ry, ELEM * ry.abs(), "rms_fwd.y" + tag, cap)
    dy = randn(g, rows, cols)
    dx, dg = be.rmsnorm_bwd(dy.to(dev), x.to(dev), gam.to(dev), rstd)
    rdx, rdg = o.rmsnorm_bwd(dy, x, gam, rstd)
    rs = o.f64(rstd)[:, None]
    xh = o.f64(x) * rs
    dy64 = o.f64(dy)
    t = dy64 * o.f64(gam)
    # dx = rstd * (t - xh * mean(t * xh)): the two terms cancel entirely
    # at cols = 1 (xh^2 ~ 1), so the floor is relative to the terms
    fl = ELEM * rs * (t.abs() + xh.abs() * (t * xh).abs().mean(-1,
                                                              keepdim=True))
    judge(dx, rdx, fl, "rms_bwd.dx" + tag, cap)
    judge(dg, rdg, rows * U * (dy64 * xh).abs().sum(0),
          "rms_bwd.dgamma" + tag, cap)


# --------------------------------------------------------------------------
# Softmax
# --------------------------------------------------------------------------

SOFTMAX_SHAPES = [(1, 1), (5, 5), (72, 72), (3, 200), (257, 513),
                  (64, 2048)]


def softmax_scores(bh, sq, sk, kind="randn"):
    g = gen(31 * sq + sk + bh)
    if kind == "pm80":       # only exp(0) and exp(-160) occur
        s = torch.randint(0, 2, (bh, sq, sk), generator=g).float() * 160 - 80
        return s.to(BF16)
    if kind == "const":
        return torch.full((bh, sq, sk), 3.25, dtype=BF16)
    return randn(g, bh, sq, sk, scale=3.0)


def check_softmax(be, dev, bh, sq, sk, causal, scale=0.125, kind="randn",
                  cap=None):
    x = softmax_scores(bh, sq, sk, kind)
    tag = f"[{bh}x{sq}x{sk} {'causal' if causal else 'full'} {kind}]"
    p = be.softmax_fwd(x.to(dev), scale=scale, causal=causal)
    rp = o.softmax_fwd(x, scale, causal)
    # p = exp(a) / sum with a = s - max <= 0. exp through exp2 rounds the
    # argument a * log2(e): relative error |a| * 1.4427 U, plus an ulp or
    # two of exp2 and the division; the denominator is a row reduction of
    # positive terms. All relative to p; results under 2^-126 may flush.
    s = o.f64(x) * o.f32r(scale)
    if causal:
        q = torch.arange(sq)[:, None]
        k = torch.arange(sk)[None, :]
        s = s.masked_fill(k > q + (sk - sq), -math.inf)
    a = (s - s.max(-1, keepdim=True).values).abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    judge(p, rp, rp * (1.4427 * a * U + ELEM) + FTZ, "softmax_fwd.p" + tag,
          cap)
    dp = randn(gen(sq * sk + 7), bh, sq, sk)
    ds = be.softmax_bwd(dp.to(dev), p, scale=scale)
    rds = o.softmax_bwd(dp, p, scale)       # from the p the backward got
    p64, dp64 = o.f64(p), o.f64(dp)
    # ds = scale * p * (dp - dot), dot = sum_k p_k dp_k a row reduction
    fl = ELEM * o.f32r(scale) * p64 * (
        dp64.abs() + (p64 * dp64).abs().sum(-1, keepdim=True)) + FTZ
    judge(ds, rds, fl, "softmax_bwd.ds" + tag, cap)


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------

CE_SHAPES = [(5, 10), (33, 520), (9, 2048), (9, 2056), (2050, 520),
             (4, 50304)]
CE_PATTERNS = ["valid", "some_ignored", "all_ignored", "ign-100_sentinels",
               "ign0"]


def ce_targets(pattern, rows, cols, g):
    """Returns (targets, ignore_index). Row 0 always aims at the last
    class, row 1 at class 0 (the ends of the vocab)."""
    t = torch.randint(0, cols, (rows,), generator=g)
    t[0] = cols - 1
    t[1] = 0
    r = torch.arange(rows)
    if pattern == "valid":
        t[1] = 1 if cols > 1 else 0
        return t, -1
    if pattern == "some_ignored":
        t[r % 3 == 2] = -1
        return t, -1
    if pattern == "all_ignored":
        return torch.full((rows,), -1), -1
    if pattern == "ign-100_sentinels":
        t[r % 4 == 2] = -100          # ignored
        t[r % 4 == 3] = -1            # "not in this vocab shard"
        return t, -100
    if pattern == "ign0":
        t[r % 3 == 2] = 0             # the pad id, also row 1
        return t, 0
    raise AssertionError(pattern)


def check_cross_entropy(be, dev, rows, cols, pattern, cap=None):
    g = gen(rows * 7 + cols)
    logits = randn(g, rows, cols, scale=3.0)
    t, ign = ce_targets(pattern, rows, cols, g)
    tag = f"[{rows}x{cols} {pattern}]"
    loss, lse = be.cross_entropy_fwd(logits.to(dev), t.to(dev), ign)
    rloss, rlse, rnll = o.cross_entropy_fwd(logits, t, ign)
    l64 = o.f64(logits)
    span = l64.max(-1).values - l64.min(-1).values
    # lse = max + log(sum exp(l - max)). Each exp has relative error up to
    # (1.4427 * span + 2) U (argument rounding in exp2 form); the online
    # sum makes 8 adds and 3 rescale operations per 2048-column step of a
    # thread, then a 10-step block reduction; log2 and its scaling add
    # 32 U absolute (log2(sum) <= 16). Relative error of the sum becomes
    # absolute error of the logarithm.
    fl_lse = (1.4427 * span + 11 * math.ceil(cols / 2048) + 48) * U
    judge(lse, rlse, fl_lse, "ce_fwd.lse" + tag, cap)
    n = max(int((t != ign).sum()), 1)
    counted = (rnll != 0)
    # loss = sum(nll) / n: each nll = lse - logit[target] carries lse's
    # floor and one rounding; the sum over rows is one more reduction
    fl_loss = ((fl_lse + 2 * U * rlse.abs())[counted].sum()
               + ELEM * rnll.abs().sum()) / n
    judge(loss.reshape(()), rloss.reshape(()), fl_loss, "ce_fwd.loss" + tag,
          cap)
    dloss = torch.tensor(1.5)
    dl = be.cross_entropy_bwd(dloss.to(dev), logits.to(dev), t.to(dev), lse,
                              ign)
    rdl, dscale = o.cross_entropy_bwd(dloss, logits, t, lse, ign)
    a = (l64 - o.f64(lse)[:, None])
    p = a.exp()
    # dlogits = (exp(a) - onehot) * dscale: exp's relative error as above,
    # and a few U absolute where exp(a) ~ 1 meets the one-hot
    fl = abs(dscale) * (p * (1.4427 * a.abs() + 8) * U + 4 * U) + FTZ
    judge(dl, rdl, fl, "ce_bwd.dlogits" + tag, cap)
    ignored = (t == ign)
    assert not dl.detach().cpu()[ignored].any(), \
        "ce_bwd" + tag + ": an ignored row's gradient is not exact zeros"
    if pattern == "all_ignored":
        assert float(loss) == 0.0, (tag, float(loss))


# --------------------------------------------------------------------------
# Embedding backward, bias sum
# --------------------------------------------------------------------------

def embedding_ids(pattern, n, vocab, g):
    if pattern == "equal":
        return torch.full((n,), vocab // 2)
    if pattern == "distinct":
        assert n <= vocab - 1
        return torch.randperm(vocab - 1, generator=g)[:n]   # V-1 unused
    ids = torch.randint(0, vocab - 1, (n,), generator=g)     # V-1 unused
    ids[0] = 0
    return ids


def check_embedding_bwd(be, dev, n, dim, vocab, pattern, cap=None):
    g = gen(n + dim)
    ids = embedding_ids(pattern, n, vocab, g)
    dy = randn(g, n, dim)
    tag = f"[{n}x{dim} V={vocab} {pattern}]"
    grad = be.embedding_bwd(dy.to(dev), ids.to(dev), vocab)
    ref, abs_sum, cnt = o.embedding_bwd(dy, ids, vocab)
    # a sum of cnt rows in any order (atomics): COL without inner roundings
    judge(grad, ref, cnt[:, None] * U * abs_sum, "embedding_bwd" + tag, cap)
    unused = cnt == 0
    assert unused.any()
    assert not grad.detach().cpu()[unused].any(), \
        "embedding_bwd" + tag + ": unused vocab row is not exact zeros"


BIAS_SHAPES = [(1, 8), (33, 100), (1000, 520), (1000, 512), (4099, 1024)]


def check_bias_sum(fn, dev, rows, cols, cap=None):
    t = randn(gen(rows + cols), rows, cols)
    ref, abs_sum = o.bias_sum(t)
    judge(fn(t.to(dev)), ref, rows * U * abs_sum,
          f"bias_sum[{rows}x{cols}]", cap)


# --------------------------------------------------------------------------
# GELU, SwiGLU
# --------------------------------------------------------------------------

ELEMWISE_N = [1, 7, 8, 9, 2055]


def activation_inputs(n, seed):
    """randn, then (where n allows) a grid over [-12, 12] with +0, -0 and
    the bf16 neighbours of +-6 (saturation of the tanh and the sigmoid)."""
    x = randn(gen(seed), n, scale=2.0)
    grid = torch.cat([torch.linspace(-12, 12, 193),
                      torch.tensor([0.0, -0.0, 6.0, -6.0, 5.96875, 6.03125,
                                    -5.96875, -6.03125])]).to(BF16)
    k = min(n, grid.numel())
    x[n - k:] = grid[:k]
    return x


def check_gelu(be, dev, n, cap=None):
    x = activation_inputs(n, n)
    dy = randn(gen(n + 1), n)
    x64, dy64 = o.f64(x), o.f64(dy)
    big = x64.abs().clamp_min(1.0)
    # y = 0.5 x (1 + t): t = tanh(z) has absolute error dt ~ 2^-21 (the
    # reciprocal's ulp at 2 / (e + 1) <= 2, exp2's ulp, the subtraction),
    # so y errs by 0.5 |x| dt; 2^-20 * max(1, |x|) is twice that
    judge(be.gelu_fwd(x.to(dev)), o.gelu_fwd(x), ELEM * big,
          f"gelu_fwd[{n}]", cap)
    # dgelu = 0.5 (1 + t) + 0.5 x (1 - t^2) z'(x): the forward's floor
    # times |dy|
    judge(be.gelu_bwd(dy.to(dev), x.to(dev)), o.gelu_bwd(dy, x),
          ELEM * dy64.abs() * big, f"gelu_bwd[{n}]", cap)


def check_swiglu(be, dev, n, cap=None):
    a = activation_inputs(n, n + 2)
    b = randn(gen(n + 3), n)
    dy = randn(gen(n + 4), n)
    big = o.f64(a).abs().clamp_min(1.0)
    b64, dy64 = o.f64(b), o.f64(dy)
    # y = a sig(a) b: products of positive-denominator terms, no
    # cancellation; 2^-20 * max(1, |a|), times |b|
    judge(be.swiglu_fwd(a.to(dev), b.to(dev)), o.swiglu_fwd(a, b),
          ELEM * big * b64.abs(), f"swiglu_fwd[{n}]", cap)
    da, db = be.swiglu_bwd(dy.to(dev), a.to(dev), b.to(dev))
    rda, rdb = o.swiglu_bwd(dy, a, b)
    # da = dy b (s + a s (1 - s)): the two terms cancel near a = -1.28
    judge(da, rda, ELEM * big * (dy64 * b64).abs(), f"swiglu_bwd.da[{n}]",
          cap)
    judge(db, rdb, ELEM * big * dy64.abs(), f"swiglu_bwd.db[{n}]", cap)


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------

def rope_floor(x, ang):
    """y = x1 cos - x2 sin (and its partner); the angle pos * freq is formed
    in fp32 from freq = exp(ln(theta) * (-2/D) * d), whose relative error
    (the exponent's roundings, exp) is about 2^-20, and the product with
    pos adds 2^-24: (|x1| + |x2|) * angle * 2^-20."""
    D = x.shape[-1]
    x64 = o.f64(x)
    mag = x64[..., :D // 2].abs() + x64[..., D // 2:].abs()
    fl = mag * ang[:, None, :] * ELEM
    return torch.cat([fl, fl], -1)


def check_rope(be, dev, tokens, heads, D, seq_len, theta, cap=None):
    x = randn(gen(tokens + heads + D), tokens, heads, D)
    tag = f"[{tokens}x{heads}x{D} S={seq_len} theta={theta:g}]"
    y = be.rope_fwd(x.to(dev), seq_len, theta)
    ry, ang = o.rope(x, seq_len, theta)
    judge(y, ry, rope_floor(x, ang), "rope_fwd" + tag, cap)
    # bwd(fwd(x)) against the oracle's inverse rotation of the same y
    dx = be.rope_bwd(y, seq_len, theta)
    rdx, _ = o.rope(y, seq_len, theta, backward=True)
    judge(dx, rdx, rope_floor(y, ang), "rope_bwd" + tag, cap)


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

# exactly representable in fp32, so that "1 - beta" means the same number
# to every implementation (1 - fp32(0.999) differs from fp32(0.001) by
# 5e-5 relative, which is a choice of hyper-parameter, not an error)
ADAMW_HP = dict(lr=2.0 ** -7, beta1=0.90625, beta2=1.0 - 2.0 ** -10,
                eps=2.0 ** -20, weight_decay=0.125)


def adamw_grad(g, n, dtype):
    """Gradients over six decades, with zeros: where |g| ~ eps the
    placement of eps in the denominator matters."""
    mag = 10.0 ** (-torch.randint(0, 7, (n,), generator=g).float())
    gr = torch.randn(n, generator=g) * mag
    gr[::17] = 0.0
    return gr.to(dtype)


def adamw_judge(got, before, grad, hp, step, tag, cap=None):
    """got = (param image, master, exp_avg, exp_avg_sq) after one step from
    `before` = (master, exp_avg, exp_avg_sq), all on the CPU."""
    rma, rm, rv, aux = o.adamw_step(before[0], grad, before[1], before[2],
                                    step=step, **hp)
    g64 = o.f64(grad)
    b1, b2 = aux["b1"], aux["b2"]
    # m = b1 m + (1 - b1) g: two products and a sum, 4 U of the terms
    fl_m = 4 * U * (b1 * o.f64(before[1]).abs() + (1 - b1) * g64.abs())
    fl_v = 4 * U * (b2 * o.f64(before[2]) + (1 - b2) * g64 * g64)
    # master = ma (1 - lr wd) - lr mhat / denom: 4 U on the decayed value,
    # 16 U on the update (bias corrections, sqrt, eps, quotient, and the
    # moments' relative errors), and m's cancellation floor carried through
    fl_ma = 4 * U * o.f64(before[0]).abs() + 16 * U * aux["upd"].abs() \
        + aux["lr"] * fl_m / (aux["bc1"] * aux["denom"])
    judge(got[2], rm, fl_m, "adamw.exp_avg" + tag, cap)
    judge(got[3], rv, fl_v, "adamw.exp_avg_sq" + tag, cap)
    judge(got[1], rma, fl_ma, "adamw.master" + tag, cap)
    judge(got[0], rma, fl_ma, "adamw.param" + tag, cap)


def check_adamw_single(be, dev, n, steps=3, cap=None, hp=ADAMW_HP):
    g = gen(n)
    master = torch.randn(n, generator=g)
    param = master.to(BF16).to(dev)
    master, m, v = master.to(dev), torch.zeros(n).to(dev), \
        torch.zeros(n).to(dev)
    for step in range(1, steps + 1):
        grad = adamw_grad(g, n, torch.float32)
        before = tuple(t.detach().cpu().clone() for t in (master, m, v))
        be.adamw_step(param, master, grad.to(dev), m, v, step=step, **hp)
        adamw_judge((param, master, m, v), before, grad, hp, step,
                    f"[fp32 grad n={n} step {step}]", cap)


def np_mask(n, p, seed, offset):
    return torch.from_numpy(o.dropout_mask(n, p, seed, offset))

