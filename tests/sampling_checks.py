"""Cases and checks shared by test_sampling_cpu.py (ops/reference.py) and
test_sampling_gpu.py (csrc/sampling.hip): both run the same check_*
functions on the same seeded CPU inputs against the float64 oracle
fp64_reference.sample_probs, through ops.sample_logits on `dev`.

The bound on kept-mass and CDF comparisons, for a row of V = vocab logits:

    eps = (4 R + ceil(V / 256) + 64) * U,    U = 2^-24,

R the largest (m - z_i) / T over the kept tokens (finite ones: -inf weighs
exactly 0): the final kept set z >= tau for the CDF comparisons, the set
top-k kept for the kept-mass conditions of top-p, which are fractions of
it. 4 R U covers one fp32 weight exp2((z - m) * c): the subtraction, the
rounded scale c = fp32(log2(e) / T), the product (3 R U relative together)
and the exp2 itself. The accumulation term is the one of fp32 chunked sums.
Both backends do better than it allows: they sum 2^-40 fixed-point integers,
which adds at most V * 2^-40 <= ceil(V / 256) * 2^-32 by truncation and
nothing by summation, so the term is kept as it stands, not narrowed or
widened. Test logits stay within +-8 and T >= 0.5 (R <= 32, eps < 1e-4).
"""

import math

import numpy as np
import torch

from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o

BF16 = torch.bfloat16
U = 2.0 ** -24
U_MIN = 2.0 ** -25            # the smallest uniform the generator gives


def gen(seed):
    return torch.Generator().manual_seed(seed)


def logits(g, B, V, scale=2.5, dtype=torch.float32):
    return (torch.randn(B, V, generator=g) * scale).clamp(-8, 8).to(dtype)


def uniforms(g, B):
    return torch.rand(B, generator=g).clamp(U_MIN, 1.0)


def eps_of(z64, T, tau):
    """The bound for one row (z64: numpy fp64 [V]) over the kept set
    z >= tau (tau None: the whole row). The kept-mass conditions of top-p
    are fractions of what top-k kept, so they take tau = tau_k; the CDF
    comparisons are over the final kept set and take the final tau."""
    kept = z64[np.isfinite(z64)] if tau is None else \
        z64[np.isfinite(z64) & (z64 >= tau)]
    R = float((z64[np.isfinite(z64)].max() - kept.min()) / T) \
        if kept.size else 0.0
    return (4.0 * R + math.ceil(z64.size / 256) + 64.0) * U


def kth_largest(z64, k):
    """Exact k-th largest value, or None when top-k is off."""
    if k <= 0 or k >= z64.size:
        return None
    return float(np.sort(z64)[::-1][k - 1])


def sample(x, dev, **kw):
    """ops.sample_logits on dev with the threshold; CPU tensors back."""
    for key in ("u", "step"):
        if kw.get(key) is not None:
            kw[key] = kw[key].to(dev)
    tok, tau = ops.sample_logits(x.to(dev) if x.device.type != dev else x,
                                 return_threshold=True, **kw)
    assert tok.dtype == torch.int64 and tok.shape == (x.shape[0], 1)
    assert tau.dtype == torch.float32 and tau.shape == (x.shape[0],)
    return tok.cpu()[:, 0], tau.cpu()


def check_rows(x, dev, T, top_k=0, top_p=1.0, u=None, vocab=None,
               call=None):
    """Runs the op on x [B, Vs] (or takes call = (tok, tau)) and holds every
    row to the rules: tau exact for top-k / no filter, the fp64 kept-mass
    conditions for top-p, and the drawn token's fp64 CDF interval around u.
    Returns (tok, tau)."""
    B = x.shape[0]
    V = x.shape[1] if vocab is None else vocab
    tok, tau = call if call is not None else sample(
        x, dev, temperature=T, top_k=top_k, top_p=top_p, u=u, vocab=vocab)
    z_all = x.detach().cpu()[:, :V].double().numpy()
    for b in range(B):
        z, t, i = z_all[b], float(tau[b]), int(tok[b])
        assert 0 <= i < V, (b, i)
        tau_k = kth_largest(z, top_k)
        if top_p >= 1.0:
            want = z.min() if tau_k is None else tau_k
            assert t == want, (b, t, want)
        else:
            assert (z == t).any(), (b, t, "tau is not an input value")
            assert tau_k is None or t >= tau_k, (b, t, tau_k)
            pk = o.sample_probs(z, T, tau_k)
            ge, gt = pk[z >= t].sum(), pk[z > t].sum()
            eps = eps_of(z, T, tau_k)
            assert ge >= top_p - eps, (b, ge, top_p, eps)
            assert gt < top_p + eps, (b, gt, top_p, eps)
        assert z[i] >= t, (b, i, z[i], t)
        if u is not None:
            cdf = np.cumsum(o.sample_probs(z, T, t))
            lo = cdf[i - 1] if i > 0 else 0.0
            ub = float(u[b])
            eps = eps_of(z, T, t)
            assert lo - eps <= ub <= cdf[i] + eps, (b, i, lo, ub, cdf[i], eps)
    return tok, tau


def tied_rows(g, B, V):
    """Rows of few distinct values, so ties straddle every k-th place."""
    return (torch.randn(B, V, generator=g) * 2.0).clamp(-8, 8).mul(2).round() \
        .div(2)


def check_topk_thresholds(dev):
    g = gen(11)
    for V in (64, 503):
        x = tied_rows(g, 3, V)
        for k in (1, 2, 50, V - 1, V, V + 5):
            tok, tau = check_rows(x, dev, 1.0, top_k=k, u=uniforms(g, 3))
            if 0 < k < V:
                want = torch.topk(x, k, dim=-1).values[:, -1]
                assert torch.equal(tau, want), (V, k, tau, want)


def check_topp_thresholds(dev):
    g = gen(12)
    x = torch.cat([logits(g, 2, 503), tied_rows(g, 1, 503)])
    for p in (1e-6, 0.5, 0.9, 0.999):
        check_rows(x, dev, 0.8, top_p=p, u=uniforms(g, 3))
        check_rows(x, dev, 0.8, top_k=50, top_p=p, u=uniforms(g, 3))


def check_no_filter_threshold(dev):
    g = gen(13)
    x = logits(g, 3, 503)
    x[1, 5:40] = float("-inf")
    _, tau = check_rows(x, dev, 1.0, u=uniforms(g, 3))
    assert torch.equal(tau, x.min(-1).values)
    assert tau[1] == float("-inf") and math.isfinite(tau[0])


def check_cdf_sweep(dev, top_k, top_p):
    """One row drawn at N evenly spaced uniforms: the histogram of tokens
    is the fp64 distribution to within the CDF bound at each edge."""
    V, N, T = 503, 8192, 0.8
    z = logits(gen(14), 1, V, scale=2.0)
    u = ((torch.arange(N, dtype=torch.float64) + 0.5) / N).float()
    tok, tau = sample(z.repeat(N, 1), dev, temperature=T, top_k=top_k,
                      top_p=top_p, u=u)
    assert bool((tau == tau[0]).all())
    check_rows(z, dev, T, top_k, top_p, call=(tok[:1], tau[:1]))
    z64 = z[0].double().numpy()
    p64 = o.sample_probs(z64, T, float(tau[0]))
    eps = eps_of(z64, T, float(tau[0]))
    counts = np.bincount(tok.numpy(), minlength=V)
    assert counts[z64 < float(tau[0])].sum() == 0
    worst = np.abs(counts - N * p64).max()
    assert worst <= 2 + 2 * N * eps, (worst, eps)


DRAW_CONFIGS = ((0, 1.0), (5, 1.0), (0, 0.7), (50, 0.9))


def check_draws(dev, V, B, dtype=torch.float32, seed=15, configs=DRAW_CONFIGS,
                T=0.8):
    g = gen(seed + V)
    x = logits(g, B, V, dtype=dtype)
    for top_k, top_p in configs:
        check_rows(x, dev, T, top_k, top_p, u=uniforms(g, B))


def check_u_ends(dev):
    g = gen(16)
    x = logits(g, 2, 503)
    for top_k, top_p in ((0, 1.0), (50, 1.0), (50, 0.9)):
        lo, tau = check_rows(x, dev, 0.8, top_k, top_p,
                             u=torch.full((2,), U_MIN))
        hi, tau2 = check_rows(x, dev, 0.8, top_k, top_p, u=torch.ones(2))
        assert torch.equal(tau, tau2)
        for b in range(2):
            kept = (x[b] >= tau[b]).nonzero()[:, 0]
            assert lo[b] == kept[0] and hi[b] == kept[-1], (lo, hi, kept)


def check_special_rows(dev):
    g = gen(17)
    N = 64
    u = uniforms(g, N)
    u[0], u[1] = U_MIN, 1.0
    # all-equal row: uniform over the row
    flat = torch.full((N, 100), 1.5)
    tok, tau = check_rows(flat, dev, 0.7, u=u)
    assert bool((tau == 1.5).all()) and tok.unique().numel() > 16
    check_rows(flat, dev, 0.7, top_k=10, top_p=0.5, u=u)   # ties: all kept
    # a single finite logit among -inf is always returned
    one = torch.full((N, 77), float("-inf"))
    one[:, 41] = -3.0
    for top_k, top_p in DRAW_CONFIGS:
        tok, _ = sample(one, dev, temperature=0.9, top_k=top_k, top_p=top_p,
                        u=u)
        assert bool((tok == 41).all()), (top_k, top_p, tok)
    # -inf tokens are never returned
    half = logits(g, 1, 200).repeat(N, 1)
    half[:, ::2] = float("-inf")
    half[:, 190:] = float("-inf")
    for top_k, top_p in DRAW_CONFIGS + ((150, 1.0),):
        tok, _ = sample(half, dev, temperature=0.9, top_k=top_k, top_p=top_p,
                        u=u)
        assert bool(torch.isfinite(half[0][tok]).all()), (top_k, top_p)
    # NaN and +inf rows: only the range is promised
    bad = logits(g, 4, 300)
    bad[0] = float("nan")
    bad[1, 7] = float("nan")
    bad[2, 9] = float("inf")
    bad[3] = float("inf")
    for top_k, top_p in DRAW_CONFIGS:
        tok, _ = sample(bad, dev, temperature=0.9, top_k=top_k, top_p=top_p,
                        u=u[:4])
        assert bool(((tok >= 0) & (tok < 300)).all()), (top_k, top_p, tok)
        tok, _ = sample(bad, dev, temperature=0.9, top_k=top_k, top_p=top_p,
                        u=u[:4], vocab=5)
        assert bool(((tok >= 0) & (tok < 5)).all()), (top_k, top_p, tok)


def check_views(dev):
    """Padding columns, strided rows and bf16 input."""
    g = gen(18)
    B, V, Vs = 4, 503, 512
    pad = logits(g, B, Vs)
    pad[:, V:] = 100.0                       # must never be chosen
    u = uniforms(g, B)
    for top_k, top_p in DRAW_CONFIGS:
        check_rows(pad, dev, 0.8, top_k, top_p, u=u, vocab=V)
    kw = dict(temperature=0.8, top_k=40, top_p=0.95, u=u)
    big = logits(g, 2 * B, Vs).to(dev)
    a = sample(big[::2, :V], dev, **kw)      # row stride 2 * Vs
    b = sample(big[::2, :V].contiguous(), dev, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xb = logits(g, B, V, dtype=BF16)
    a = sample(xb, dev, **kw)
    b = sample(xb.float(), dev, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_rows(xb, dev, 0.8, 40, 0.95, u=u, call=a)


def check_philox(dev):
    g = gen(19)
    B, V, seed, pos = 8, 503, 1234567890123, 37
    x = logits(g, B, V)
    kw = dict(temperature=0.8, top_k=50, top_p=0.9)
    step = torch.tensor([pos], dtype=torch.int64)
    u = torch.from_numpy(o.sample_uniform(seed, B, pos))
    assert u.unique().numel() == B and bool(((u > 0) & (u <= 1)).all())
    a = sample(x, dev, seed=seed, step=step, **kw)
    b = sample(x, dev, u=u, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_rows(x, dev, u=u, call=a, T=0.8, top_k=50, top_p=0.9)
    # the draw of row b does not depend on the batch size
    c = sample(x[:3], dev, seed=seed, step=step, **kw)
    assert torch.equal(c[0], a[0][:3])
    # rows of one call use different uniforms; so do other seeds and steps
    same = x[:1].repeat(64, 1)
    t0 = sample(same, dev, seed=seed, step=step, temperature=1.0)[0]
    t1 = sample(same, dev, seed=seed, step=step + 1, temperature=1.0)[0]
    t2 = sample(same, dev, seed=seed + 1, step=step, temperature=1.0)[0]
    assert t0.unique().numel() > 8
    assert not torch.equal(t0, t1) and not torch.equal(t0, t2)


def check_refusals(dev, launched=lambda: 0):
    """Every bad call raises ValueError; `launched` counts launches."""
    x = torch.randn(2, 64, device=dev)
    u = torch.rand(2, device=dev).clamp(U_MIN, 1)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    bad = (
        dict(logits=x, temperature=0.0, u=u),
        dict(logits=x, temperature=-1.0, u=u),
        dict(logits=x, temperature=1.0, u=u, step=step),
        dict(logits=x, temperature=1.0),
        dict(logits=x.t().contiguous().t(), temperature=1.0, u=u),
        dict(logits=x.half(), temperature=1.0, u=u),
        dict(logits=x, temperature=1.0, u=u, vocab=65),
        dict(logits=x, temperature=1.0, u=u, vocab=0),
        dict(logits=torch.zeros(1, (1 << 22) + 1, device=dev),
             temperature=1.0, u=u[:1]),           # sums could overflow
        dict(logits=x, temperature=1.0, u=u,
             out=torch.zeros(2, dtype=torch.int64, device=dev)),
    )
    n0 = launched()
    for kw in bad:
        kw = dict(kw)
        x_ = kw.pop("logits")
        try:
            ops.sample_logits(x_, **kw)
        except ValueError:
            continue
        raise AssertionError(f"accepted {kw}")
    assert launched() == n0
