"""Float64 oracles for the row and elementwise ops and for attention, and
the bound the HIP kernels (and the fp32 ops/reference.py) are held to.

Every function takes the tensors the kernel takes (bf16 / fp32 / int, on
any device), moves them to the CPU, upcasts to float64 and evaluates the
op's mathematical definition. Nothing here calls ops/reference.py or a
kernel: the oracle is independent of both implementations. Scalars that a
kernel receives as `float` (eps, scale, the AdamW hyper-parameters) are
rounded to fp32 first, because that rounded value is the kernel's input.

assert_within_ulp is the one criterion: an output is right when it lies
within one unit in the last place of the float64 value, plus a floor the
caller derives from the fp32 arithmetic of the op (see each test).
"""

from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64
BF16 = torch.bfloat16
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)
GELU_C = 0.044715


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().to(F64)


def f32r(v: float) -> float:
    """v rounded to fp32 (what a kernel's `float` argument holds)."""
    return float(np.float32(v))


# --------------------------------------------------------------------------
# The bound
# --------------------------------------------------------------------------

def ulp_bf16(r: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2|r|) - 7): the spacing of bf16 (8 significant bits) at
    r. Below the smallest normal (and at 0) the subnormal spacing 2^-133."""
    _, e = torch.frexp(r.abs())            # |r| = m * 2^e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, -10000), e)
    return torch.ldexp(torch.ones_like(r), (e - 1).clamp_min(-126) - 7)


def ulp_error(got: torch.Tensor, ref64: torch.Tensor, floor=0.0):
    """Returns (err, unit, tol), elementwise in float64: err = |got -
    ref64|; unit = one bf16 ulp of ref64 for a bf16 output, 2^-23 * |ref64|
    for an fp32 one; tol = unit + floor, the allowed error."""
    g = f64(got)
    assert g.shape == ref64.shape, (g.shape, ref64.shape)
    if got.dtype == BF16:
        unit = ulp_bf16(ref64)
    elif got.dtype == torch.float32:
        unit = ref64.abs() * 2.0 ** -23
    else:
        raise TypeError(f"no ulp bound for {got.dtype}")
    fl = floor if isinstance(floor, torch.Tensor) else \
        torch.tensor(float(floor), dtype=F64)
    return (g - ref64).abs(), unit, (unit + f64(fl)).expand_as(ref64)


def ulp_violations(got: torch.Tensor, ref64: torch.Tensor, floor=0.0):
    """Boolean tensor: where got misses the bound (NaN misses it)."""
    err, _, tol = ulp_error(got, ref64, floor)
    return ~(err <= tol)


def assert_within_ulp(got: torch.Tensor, ref64: torch.Tensor, floor=0.0,
                      what: str = "") -> None:
    """Passes iff elementwise |got - ref64| <= ulp(ref64) + floor (`floor`
    a scalar or a tensor broadcastable to ref64). On failure reports the
    element that exceeds its bound by the largest factor: its index, both
    values, the error in ulps, the floor there and that factor."""
    err, unit, tol = ulp_error(got, ref64, floor)
    bad = ~(err <= tol)
    if bad.any():
        over = torch.where(bad, torch.nan_to_num(err / tol, nan=math.inf),
                           torch.zeros_like(err))
        flat = int(over.reshape(-1).argmax())
        idx = tuple(int(i) for i in
                    np.unravel_index(flat, tuple(err.shape))) \
            if err.dim() else ()
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {err.numel()} elements outside "
            f"1 ulp + floor; worst at {idx}: got {f64(got)[idx].item()!r}, "
            f"fp64 {ref64[idx].item()!r}, error "
            f"{(err[idx] / unit[idx]).item():.3f} ulp, floor there "
            f"{(tol[idx] - unit[idx]).item():.3e}, "
            f"{over[idx].item():.2f} times the bound")


# --------------------------------------------------------------------------
# LayerNorm / add + LayerNorm / RMSNorm
# --------------------------------------------------------------------------

def layernorm_fwd(x, gamma, beta, eps: float = 1e-5):
    """Returns (y, mean, rstd): biased variance, rstd = (var + eps)^-1/2."""
    x, g, b = f64(x), f64(gamma), f64(beta)
    mean = x.sum(-1) / x.shape[-1]
    d = x - mean[:, None]
    rstd = (d.pow(2).sum(-1) / x.shape[-1] + f32r(eps)).pow(-0.5)
    return d * rstd[:, None] * g + b, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dsum=None):
    """Returns (dx, dgamma, dbeta) from the saved fp32 statistics; with
    dsum, dx = dsum + d(ln)/dx (the add + LayerNorm backward)."""
    dy, x, g = f64(dy), f64(x), f64(gamma)
    rs = f64(rstd)[:, None]
    xhat = (x - f64(mean)[:, None]) * rs
    gg = dy * g
    c1 = gg.sum(-1, keepdim=True) / x.shape[-1]
    c2 = (gg * xhat).sum(-1, keepdim=True) / x.shape[-1]
    dx = (gg - c1 - xhat * c2) * rs
    if dsum is not None:
        dx = dx + f64(dsum)
    return dx, (dy * xhat).sum(0), dy.sum(0)


def add_round(x, res):
    """The residual sum as ln_fwd_kernel documents it: x + res formed in
    fp32 and rounded once to bf16 (a bf16 tensor, compared bit for bit)."""
    return (x.detach().cpu().float() + res.detach().cpu().float()).to(BF16)


def add_layernorm_fwd(x, res, gamma, beta, eps: float = 1e-5):
    """Returns (s, y, mean, rstd); statistics are over the rounded sum."""
    s = add_round(x, res)
    return (s,) + layernorm_fwd(s, gamma, beta, eps)


def add_layernorm_bwd(dy, dsum, s, gamma, mean, rstd):
    return layernorm_bwd(dy, s, gamma, mean, rstd, dsum=dsum)


def rmsnorm_fwd(x, gamma, eps: float = 1e-6):
    """Returns (y, rstd), rstd = (mean(x^2) + eps)^-1/2."""
    x, g = f64(x), f64(gamma)
    rstd = (x.pow(2).sum(-1) / x.shape[-1] + f32r(eps)).pow(-0.5)
    return x * rstd[:, None] * g, rstd


def rmsnorm_bwd(dy, x, gamma, rstd):
    """Returns (dx, dgamma) from the saved fp32 rstd."""
    dy, x, g = f64(dy), f64(x), f64(gamma)
    rs = f64(rstd)[:, None]
    xh = x * rs
    t = dy * g
    c = (t * xh).sum(-1, keepdim=True) / x.shape[-1]
    return rs * (t - xh * c), (dy * xh).sum(0)


# --------------------------------------------------------------------------
# Softmax
# --------------------------------------------------------------------------

def softmax_fwd(scores, scale: float = 1.0, causal: bool = False):
    """softmax(scale * scores) over the last dim of [..., sq, sk]; causal:
    query q sees keys k <= q + (sk - sq)."""
    s = f64(scores) * f32r(scale)
    if causal:
        sq, sk = s.shape[-2], s.shape[-1]
        q = torch.arange(sq)[:, None]
        k = torch.arange(sk)[None, :]
        s = s.masked_fill(k > q + (sk - sq), -math.inf)
    e = (s - s.max(-1, keepdim=True).values).exp()
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(dp, p, scale: float = 1.0):
    """ds = scale * p * (dp - sum_k dp_k p_k), from the saved bf16 p."""
    dp, p = f64(dp), f64(p)
    return f32r(scale) * p * (dp - (dp * p).sum(-1, keepdim=True))


# --------------------------------------------------------------------------
# Attention (the flash kernels of csrc/attention.hip)
# --------------------------------------------------------------------------

NO_LSE = -3.0e38      # what the kernels store for a row that saw no key


def attention_scores(q, k, causal: bool, scale: float):
    """Returns (s, allowed): s = scale * q k^T in float64, [B, H, S, S],
    and the boolean [S, S] mask of the keys a query may see (causal: key
    j <= query i). s is left unmasked."""
    S = q.shape[-2]
    s = f64(q) @ f64(k).transpose(-1, -2) * f32r(scale)
    i = torch.arange(S)
    allowed = (i[None, :] <= i[:, None]) if causal else \
        torch.ones(S, S, dtype=torch.bool)
    return s, allowed


def attention_fwd(q, k, v, causal: bool, scale: float):
    """Returns (out, lse, p): p = softmax over the allowed keys of
    scale * q k^T [B, H, S, S], out = p v, lse [B, H, S] the logsumexp of
    the allowed scaled scores."""
    s, allowed = attention_scores(q, k, causal, scale)
    s = s.masked_fill(~allowed, -math.inf)
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    p = e / l
    return p @ f64(v), (m + l.log())[..., 0], p


def attention_p_given_lse(q, k, lse, causal: bool, scale: float):
    """p^ = exp(scale * q k^T - lse) where the key is allowed, 0 where it
    is masked or the row's lse is the NO_LSE sentinel: the probabilities
    the backward forms from the lse it was GIVEN (any shape that reshapes
    to [B, H, S]). With a global lse of more keys a row sums to under 1."""
    s, allowed = attention_scores(q, k, causal, scale)
    l = f64(lse).reshape(s.shape[:-1])[..., None]
    valid = allowed & (l > -1.0e38)
    return torch.where(valid, s - torch.where(valid, l, torch.zeros_like(l)),
                       torch.full_like(s, -math.inf)).exp()


def attention_bwd(dout, q, k, v, out, lse, causal: bool, scale: float):
    """Returns (dq, dk, dv) as a function of the (out, lse) the backward
    was given (as softmax_bwd is of its p): dS = p^ * (dout v^T - delta),
    delta = sum_d dout * out, dq = scale * dS k, dk = scale * dS^T q,
    dv = p^^T dout."""
    ph = attention_p_given_lse(q, k, lse, causal, scale)
    do = f64(dout)
    delta = (do * f64(out)).sum(-1, keepdim=True)
    ds = ph * (do @ f64(v).transpose(-1, -2) - delta)
    sc = f32r(scale)
    return sc * ds @ f64(k), sc * ds.transpose(-1, -2) @ f64(q), \
        ph.transpose(-1, -2) @ do


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------

def _ce_masks(targets, ignore_index):
    t = targets.detach().cpu().long()
    valid = t != ignore_index          # counts towards n, gets a gradient
    has_tgt = valid & (t >= 0)         # negative, not ignored: no one-hot
    return t, valid, has_tgt


def cross_entropy_fwd(logits, targets, ignore_index: int = -1):
    """Returns (loss, lse, nll). A row whose target equals ignore_index adds
    nothing and is not counted; a row with another negative target ("not in
    this vocab shard") adds nothing but is counted. loss = sum / max(n, 1)."""
    l = f64(logits)
    t, valid, has_tgt = _ce_masks(targets, ignore_index)
    m = l.max(-1, keepdim=True).values
    lse = (l - m).exp().sum(-1).log() + m[:, 0]
    picked = l.gather(-1, t.clamp_min(0)[:, None])[:, 0]
    nll = torch.where(has_tgt, lse - picked, torch.zeros_like(lse))
    return nll.sum() / max(int(valid.sum()), 1), lse, nll


def cross_entropy_bwd(dloss, logits, targets, lse, ignore_index: int = -1):
    """dlogits = (softmax - onehot) * dloss / n from the saved fp32 lse:
    zero rows where ignored, no one-hot for the other negative targets. The
    scale dloss / n is formed in fp32, as the wrapper passes it."""
    l = f64(logits)
    t, valid, has_tgt = _ce_masks(targets, ignore_index)
    p = (l - f64(lse)[:, None]).exp()
    onehot = torch.zeros_like(p)
    onehot.scatter_(-1, t.clamp_min(0)[:, None], has_tgt.to(F64)[:, None])
    n = max(int(valid.sum()), 1)
    dscale = float(dloss.detach().cpu().float() / n)
    return (p - onehot) * dscale * valid.to(F64)[:, None], dscale


# --------------------------------------------------------------------------
# Embedding backward, column bias sum
# --------------------------------------------------------------------------

def embedding_bwd(dy, ids, vocab: int):
    """Returns (grad, abs_sum, count): grad[v] = sum of dy rows with id v;
    abs_sum and count are the same reduction over |dy| and over ones (the
    inputs of the column-reduction floor)."""
    d = f64(dy).reshape(-1, dy.shape[-1])
    i = ids.detach().cpu().reshape(-1).long()
    z = torch.zeros(vocab, d.shape[1], dtype=F64)
    cnt = torch.zeros(vocab, dtype=F64).index_add_(
        0, i, torch.ones(i.numel(), dtype=F64))
    return z.index_add(0, i, d), z.index_add(0, i, d.abs()), cnt


def bias_sum(t):
    """Returns (column sums, column sums of |t|)."""
    t = f64(t)
    return t.sum(0), t.abs().sum(0)


# --------------------------------------------------------------------------
# GELU (tanh form), SwiGLU
# --------------------------------------------------------------------------

def _gelu_tanh(x):
    return torch.tanh(SQRT_2_OVER_PI * (x + GELU_C * x ** 3))


def gelu_fwd(x):
    x = f64(x)
    return 0.5 * x * (1.0 + _gelu_tanh(x))


def gelu_bwd(dy, x):
    x = f64(x)
    t = _gelu_tanh(x)
    dt = (1.0 - t * t) * SQRT_2_OVER_PI * (1.0 + 3.0 * GELU_C * x * x)
    return f64(dy) * (0.5 * (1.0 + t) + 0.5 * x * dt)


def swiglu_fwd(a, b):
    a = f64(a)
    return a * torch.sigmoid(a) * f64(b)


def swiglu_bwd(dy, a, b):
    """Returns (da, db)."""
    dy, a, b = f64(dy), f64(a), f64(b)
    s = torch.sigmoid(a)
    return dy * b * s * (1.0 + a * (1.0 - s)), dy * a * s


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------

def rope_angles(tokens: int, D: int, seq_len: int, theta: float):
    """angle[t, d] = (t mod seq_len) * theta^(-2d/D), d in [0, D/2)."""
    pos = (torch.arange(tokens) % seq_len).to(F64)
    d = torch.arange(D // 2, dtype=F64)
    return pos[:, None] * torch.exp(-2.0 * d / D * math.log(f32r(theta)))


def rope(x, seq_len: int, theta: float = 10000.0, backward: bool = False):
    """Rotate-half RoPE of x [tokens, heads, D]; backward is the inverse
    rotation. Returns (y, angle)."""
    T, H, D = x.shape
    ang = rope_angles(T, D, seq_len, theta)
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    if backward:
        s = -s
    x = f64(x)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1), ang


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

def adamw_step(master, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
               weight_decay, step: int):
    """One decoupled-weight-decay Adam step from the given fp32 state.
    Returns (master, exp_avg, exp_avg_sq, aux) in float64; aux holds the
    pieces the error floors are built from: `upd` = lr * mhat / denom (the
    term subtracted), `denom` = sqrt(vhat) + eps, and `bc1`."""
    lr_, b1, b2, eps_, wd = (f32r(v) for v in
                             (lr, beta1, beta2, eps, weight_decay))
    g = f64(grad)
    m = b1 * f64(exp_avg) + (1.0 - b1) * g
    v = b2 * f64(exp_avg_sq) + (1.0 - b2) * g * g
    mhat = m / (1.0 - beta1 ** step)
    vhat = v / (1.0 - beta2 ** step)
    denom = vhat.sqrt() + eps_
    upd = lr_ * mhat / denom
    aux = {"upd": upd, "denom": denom, "bc1": 1.0 - beta1 ** step,
           "lr": lr_, "b1": b1, "b2": b2}
    return f64(master) * (1.0 - lr_ * wd) - upd, m, v, aux


# --------------------------------------------------------------------------
# Dropout mask: Philox4x32-10
# --------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0 = np.uint64(0xD2511F53)
_PHILOX_M1 = np.uint64(0xCD9E8D57)
_PHILOX_W0 = np.uint64(0x9E3779B9)
_PHILOX_W1 = np.uint64(0xBB67AE85)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers:
    as easy as 1, 2, 3", SC'11), written from the published round function
    and constants. counter: four uint64 arrays holding 32-bit words; key:
    two 32-bit ints. Returns the four output words as uint64 arrays.

    The Random123 known-answer vector for an all-zero counter and key is
    remembered as 6627e8d5 e169c58d bc57ac4c 9b00dbd8; no installed
    package here carries it, so it is not used as a self-check."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in counter)
    k0, k1 = np.uint64(key[0]) & _M32, np.uint64(key[1]) & _M32
    for _ in range(10):
        p0 = _PHILOX_M0 * c0           # 32 x 32 bits: fits uint64
        p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + _PHILOX_W0) & _M32
        k1 = (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def dropout_mask(n: int, p: float, seed: int, offset: int) -> np.ndarray:
    """The dropout keep mask (uint8 [n]) as csrc/common.h builds it: key =
    (seed lo, seed hi), counter = (offset lo, offset hi, i//4 lo, i//4 hi),
    element i takes word i % 4, u = (w >> 8) * 2^-24 + 2^-25 in fp32, keep
    iff u > fp32(p). A pure function of (seed, offset, i)."""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    off = np.uint64(offset)
    full = np.full_like(blk, 1)
    words = philox4x32_10(
        (full * (off & _M32), full * (off >> np.uint64(32)),
         blk & _M32, blk >> np.uint64(32)),
        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) \
        + np.float32(2.0 ** -25)
    return (u > np.float32(p)).astype(np.uint8)


def dropout_apply(x, mask, p: float):
    """bf16(x * fp32(1 / (1 - p))) where kept, exact zero elsewhere; the
    scale is the fp32 quotient 1.0f / (1.0f - p) the launcher forms."""
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    y = (x.detach().cpu().float() * float(scale)).to(BF16)
    keep = torch.as_tensor(np.asarray(mask)).reshape(x.shape).bool()
    return torch.where(keep, y, torch.zeros_like(y))


# --------------------------------------------------------------------------
# Token sampling
# --------------------------------------------------------------------------

def sample_uniform(seed: int, B: int, step: int) -> np.ndarray:
    """The fp32 uniforms (0, 1] sample_logits draws for rows 0..B-1 at
    position `step`: first word of Philox4x32-10 with key = (seed lo, seed
    hi) and counter = (step lo, step hi, b lo, b hi), as Philox4(seed,
    subseq = b, offset = step) of csrc/common.h, through u32_to_uniform."""
    rows = np.arange(B, dtype=np.uint64)
    off = np.uint64(step & 0xFFFFFFFFFFFFFFFF)
    full = np.full_like(rows, 1)
    x = philox4x32_10(
        (full * (off & _M32), full * (off >> np.uint64(32)),
         rows & _M32, rows >> np.uint64(32)),
        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]
    return (x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) \
        + np.float32(2.0 ** -25)


def sample_probs(z, temperature: float, tau=None) -> np.ndarray:
    """fp64 probabilities of one row of logits z [V] under sample_logits'
    rules: p_i proportional to exp((z_i - m) / T) over the kept set
    z >= tau (everything when tau is None), exactly 1 weight at z_i == m,
    0 outside the kept set and at -inf."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((z - m) / float(temperature))
    w = np.where(z == m, 1.0, w)
    if tau is not None:
        w = np.where(z >= float(tau), w, 0.0)
    return w / w.sum()
