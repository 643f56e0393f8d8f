"""Pure-PyTorch reference implementations of every planner-sharded op.

These define the exact numerical semantics of the hand-written CDNA4 HIP
kernels in tepdist_amd/ops/csrc/. They are the CPU execution path and the
fp32 baseline that tests/test_*_numerics.py compare the HIP kernels against
(numerics tests for a HIP kernel compare against a plain
PyTorch fp32 reference of the same op).

Conventions:
- Compute dtype bf16, statistics/accumulation fp32 (kernels accumulate in
  fp32 MFMA accumulators / fp32 VGPRs).
- `linear` takes weight in PyTorch layout [out_features, in_features] so the
  forward GEMM is A[M,K] @ B^T with B stored [N,K] (the MFMA kernel's
  preferred k-contiguous layout).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


# --------------------------------------------------------------------------
# GEMM / linear
# --------------------------------------------------------------------------

def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
               act: str = "none") -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """y = act(x @ w^T + bias). Returns (y, pre_act) where pre_act is saved
    only when act != 'none' (needed for backward)."""
    y32 = x.float() @ w.float().t()
    if bias is not None:
        y32 = y32 + bias.float()
    if act == "none":
        return y32.to(x.dtype), None
    elif act == "gelu":
        pre = y32.to(x.dtype)
        return gelu_fwd(pre), pre
    else:
        raise ValueError(f"unknown activation {act}")


def linear_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
               has_bias: bool, act: str, pre_act: Optional[torch.Tensor]):
    """Returns (dx, dw, dbias)."""
    dy32 = dy.float()
    if act == "gelu":
        dy32 = (gelu_bwd(dy, pre_act)).float()
    dx = (dy32 @ w.float()).to(x.dtype)
    dw = (dy32.t() @ x.float()).to(w.dtype)
    db = dy32.sum(dim=0).to(w.dtype) if has_bias else None
    return dx, dw, db


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Plain C = A @ B with fp32 accumulation, output in input dtype.
    Supports batched inputs with broadcasting like torch.matmul."""
    return (a.float() @ b.float()).to(a.dtype)


# --------------------------------------------------------------------------
# GELU (tanh approximation, as GPT-2 uses)
# --------------------------------------------------------------------------

def gelu_fwd(x: torch.Tensor) -> torch.Tensor:
    x32 = x.float()
    y = 0.5 * x32 * (1.0 + torch.tanh(SQRT_2_OVER_PI * (x32 + 0.044715 * x32 ** 3)))
    return y.to(x.dtype)


def gelu_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    x32 = x.float()
    t = torch.tanh(SQRT_2_OVER_PI * (x32 + 0.044715 * x32 ** 3))
    dt = (1.0 - t * t) * SQRT_2_OVER_PI * (1.0 + 3 * 0.044715 * x32 ** 2)
    dgelu = 0.5 * (1.0 + t) + 0.5 * x32 * dt
    return (dy.float() * dgelu).to(dy.dtype)


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------

def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                  eps: float = 1e-5):
    """Row-wise LN over the last dim. Returns (y, mean[f32], rstd[f32])."""
    x32 = x.float()
    mean = x32.mean(dim=-1)
    var = x32.var(dim=-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    xhat = (x32 - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    y = xhat * gamma.float() + beta.float()
    return y.to(x.dtype), mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor,
                  mean: torch.Tensor, rstd: torch.Tensor,
                  dsum: Optional[torch.Tensor] = None):
    """Returns (dx, dgamma, dbeta). With dsum, dx = dsum + d(ln)/dx summed
    in fp32 and rounded once (the add + LayerNorm backward)."""
    x32 = x.float()
    dy32 = dy.float()
    xhat = (x32 - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    dgamma = (dy32 * xhat).sum(dim=tuple(range(dy.dim() - 1)))
    dbeta = dy32.sum(dim=tuple(range(dy.dim() - 1)))
    D = x.shape[-1]
    g = dy32 * gamma.float()
    c1 = g.mean(dim=-1, keepdim=True)
    c2 = (g * xhat).mean(dim=-1, keepdim=True)
    dx = (g - c1 - xhat * c2) * rstd.unsqueeze(-1)
    if dsum is not None:
        dx = dx + dsum.float()
    return dx.to(x.dtype), dgamma.to(gamma.dtype), dbeta.to(gamma.dtype)


def add_layernorm_fwd(x: torch.Tensor, res: torch.Tensor,
                      gamma: torch.Tensor, beta: torch.Tensor,
                      eps: float = 1e-5):
    """s = x + res (fp32 sum rounded once), y = ln(s) with statistics over
    the rounded s. Returns (s, y, mean, rstd)."""
    s = (x.float() + res.float()).to(x.dtype)
    return (s,) + layernorm_fwd(s, gamma, beta, eps)


def add_layernorm_bwd(dy, dsum, s, gamma, mean, rstd):
    """Returns (dx, dgamma, dbeta); dsum may be None."""
    return layernorm_bwd(dy, s, gamma, mean, rstd, dsum=dsum)


# --------------------------------------------------------------------------
# Softmax (fused scale + causal mask + softmax over last dim)
# --------------------------------------------------------------------------

def softmax_fwd(scores: torch.Tensor, scale: float = 1.0,
                causal: bool = False) -> torch.Tensor:
    """p = softmax(scores * scale [+ causal mask]) over the last dim.
    scores: [..., S_q, S_k]."""
    s32 = scores.float() * scale
    if causal:
        sq, sk = scores.shape[-2], scores.shape[-1]
        if sq > sk:
            # the first sq - sk queries would see no key at all (NaN rows)
            raise ValueError(f"causal softmax needs sq <= sk, got sq={sq} "
                             f"sk={sk}")
        mask = torch.ones(sq, sk, dtype=torch.bool, device=scores.device).tril(sk - sq)
        s32 = s32.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s32, dim=-1)
    return p.to(scores.dtype)


def softmax_bwd(dp: torch.Tensor, p: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """ds = scale * p * (dp - sum(dp*p, -1)). The causal mask needs no special
    handling: masked p entries are exactly 0."""
    p32 = p.float()
    dp32 = dp.float()
    dot = (dp32 * p32).sum(dim=-1, keepdim=True)
    return (scale * p32 * (dp32 - dot)).to(p.dtype)


# --------------------------------------------------------------------------
# Attention (composed reference; the GPU path uses batched GEMM kernels +
# the fused softmax kernel, later a fused flash-style kernel)
# --------------------------------------------------------------------------

def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  causal: bool = True):
    """q,k,v: [B, H, S, D]. Returns (out, residuals) with the residuals
    saved for backward (here: the attention probabilities)."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    scores = matmul(q, k.transpose(-1, -2))
    p = softmax_fwd(scores, scale=scale, causal=causal)
    out = matmul(p, v)
    return out, (p,)


def attention_bwd(dout: torch.Tensor, q, k, v, residuals,
                  causal: bool = True):
    (p,) = residuals
    scale = 1.0 / math.sqrt(q.shape[-1])
    dv = matmul(p.transpose(-1, -2), dout)
    dp = matmul(dout, v.transpose(-1, -2))
    ds = softmax_bwd(dp, p, scale=scale)
    dq = matmul(ds, k)
    dk = matmul(ds.transpose(-1, -2), q)
    return dq, dk, dv


def attention_qkv_fwd(qkv: torch.Tensor, heads: int, causal: bool = True):
    """Packed-projection attention (reference): split + transpose, run the
    composed path, return residuals carrying what backward needs."""
    B, S, d3 = qkv.shape
    d = d3 // 3
    D = d // heads
    q, k, v = (t.reshape(B, S, heads, D).transpose(1, 2).contiguous()
               for t in qkv.split(d, dim=-1))
    out4, (p,) = attention_fwd(q, k, v, causal=causal)
    out = out4.transpose(1, 2).reshape(B, S, d)
    return out, (q, k, v, p)


def attention_qkv_bwd(dout: torch.Tensor, qkv: torch.Tensor, heads: int,
                      residuals, causal: bool = True):
    B, S, d3 = qkv.shape
    d = d3 // 3
    D = d // heads
    q, k, v, p = residuals
    dout4 = dout.reshape(B, S, heads, D).transpose(1, 2).contiguous()
    dq, dk, dv = attention_bwd(dout4, q, k, v, (p,), causal=causal)
    def back(t):
        return t.transpose(1, 2).reshape(B, S, d)
    return torch.cat([back(dq), back(dk), back(dv)], dim=-1)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, positions: torch.Tensor,
                     k_new: Optional[torch.Tensor] = None,
                     v_new: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None,
                     rope_theta: Optional[float] = None) -> torch.Tensor:
    """Single-query attention over a KV cache. q: [B, H, D]; k_new/v_new:
    [B, Hkv, D]; k_cache/v_cache: [B, Hkv, S_max, D] with H a multiple of
    Hkv (grouped-query attention: query head h attends K/V head
    h // (H // Hkv)); positions: int64 [1] or [B], clamped into
    [0, S_max-1]. With (k_new, v_new) the new row is first written
    IN PLACE into cache[b, :, p[b]]; batch row b then attends cache rows
    0..p[b] inclusive. Rows above p[b] have no influence whatever they hold
    (NaN included). With rope_theta, q and k_new are first rotated by p[b]
    in fp32 (rope_at's convention): q is used unrounded, the rotated k_new
    is cast to the cache dtype when written, so the cache holds rotated
    rows; without k_new only q is rotated. fp32 math, returns [B, H, D] in
    q.dtype."""
    assert (k_new is None) == (v_new is None)
    B, H, D = q.shape
    Hkv, S_max = k_cache.shape[1], k_cache.shape[2]
    assert H % Hkv == 0, (H, Hkv)
    G = H // Hkv
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    pos = positions.reshape(-1).long().clamp(0, S_max - 1)
    assert pos.numel() in (1, B), positions.shape
    pos = pos.expand(B)
    qf = q.float()
    if rope_theta is not None:
        qf = _rope_at_f32(qf, pos[:, None], rope_theta)
    if k_new is not None:
        assert k_new.shape == (B, Hkv, D) and v_new.shape == k_new.shape
        if rope_theta is not None:
            k_new = _rope_at_f32(k_new, pos[:, None], rope_theta)
        bidx = torch.arange(B, device=q.device)
        k_cache[bidx, :, pos] = k_new.to(k_cache.dtype)
        v_cache[bidx, :, pos] = v_new.to(v_cache.dtype)
    dead = torch.arange(S_max, device=q.device)[None, :] > pos[:, None]
    scores = torch.einsum("bhgd,bhsd->bhgs", qf.reshape(B, Hkv, G, D),
                          k_cache.float()) * scale
    scores = scores.masked_fill(dead[:, None, None, :], float("-inf"))
    p = torch.softmax(scores, dim=-1)
    v32 = v_cache.float().masked_fill(dead[:, None, :, None], 0.0)
    return torch.einsum("bhgs,bhsd->bhgd", p, v32).reshape(B, H, D) \
        .to(q.dtype)


# --------------------------------------------------------------------------
# Embedding
# --------------------------------------------------------------------------

def embedding_fwd(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    return table[ids]


def embedding_bwd(dy: torch.Tensor, ids: torch.Tensor, vocab: int) -> torch.Tensor:
    """Scatter-add gradients into a [vocab, D] table gradient (fp32 accum)."""
    D = dy.shape[-1]
    grad = torch.zeros(vocab, D, dtype=torch.float32, device=dy.device)
    grad.index_add_(0, ids.reshape(-1), dy.reshape(-1, D).float())
    return grad.to(dy.dtype)


# --------------------------------------------------------------------------
# Cross entropy (fused log-softmax + NLL; bwd writes d_logits directly)
# --------------------------------------------------------------------------

def cross_entropy_fwd(logits: torch.Tensor, targets: torch.Tensor,
                      ignore_index: int = -1):
    """logits [M, V], targets [M]. Returns (mean_loss[f32 scalar],
    logsumexp[f32, M]) with lse saved for backward."""
    l32 = logits.float()
    lse = torch.logsumexp(l32, dim=-1)
    valid = targets != ignore_index
    has_tgt = targets >= 0  # negative non-ignore = "no target here"
    tgt = targets.clamp_min(0)
    nll = lse - l32.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    nll = torch.where(valid & has_tgt, nll, torch.zeros_like(nll))
    n = valid.sum().clamp_min(1)
    return nll.sum() / n, lse


def cross_entropy_bwd(dloss: torch.Tensor, logits: torch.Tensor,
                      targets: torch.Tensor, lse: torch.Tensor,
                      ignore_index: int = -1) -> torch.Tensor:
    l32 = logits.float()
    p = torch.exp(l32 - lse.unsqueeze(-1))
    valid = (targets != ignore_index)
    has_tgt = targets >= 0  # negative non-ignore: softmax grad, no onehot
    tgt = targets.clamp_min(0)
    p.scatter_add_(-1, tgt.unsqueeze(-1),
                   -has_tgt.to(torch.float32).unsqueeze(-1))
    n = valid.sum().clamp_min(1).float()
    p = p * (dloss.float() / n)
    p = torch.where(valid.unsqueeze(-1), p, torch.zeros_like(p))
    return p.to(logits.dtype)


# --------------------------------------------------------------------------
# Dropout (counter-based Philox so the mask is reproducible from (seed,
# offset) without storing it; the HIP kernel uses the same construction)
# --------------------------------------------------------------------------

def _philox_mask(shape, p: float, seed: int, offset: int, device) -> torch.Tensor:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed * 1000003 + offset)
    return (torch.rand(shape, generator=g, device="cpu") >= p).to(device)


def dropout_fwd(x: torch.Tensor, p: float, seed: int, offset: int):
    if p == 0.0:
        return x, None
    mask = _philox_mask(x.shape, p, seed, offset, x.device)
    scale = 1.0 / (1.0 - p)
    return (x.float() * mask.float() * scale).to(x.dtype), mask


def dropout_bwd(dy: torch.Tensor, mask: Optional[torch.Tensor], p: float):
    if p == 0.0 or mask is None:
        return dy
    scale = 1.0 / (1.0 - p)
    return (dy.float() * mask.float() * scale).to(dy.dtype)


# --------------------------------------------------------------------------
# AdamW fused step (bf16 params + fp32 master/moments)
# --------------------------------------------------------------------------

def adamw_step(param_bf16: torch.Tensor, master: torch.Tensor,
               grad: torch.Tensor, exp_avg: torch.Tensor,
               exp_avg_sq: torch.Tensor, lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int):
    """In-place AdamW on the fp32 master copy; bf16 param refreshed from it.
    grad may be bf16 or fp32."""
    g = grad.float()
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt().add_(eps)
    master.mul_(1 - lr * weight_decay)
    master.addcdiv_(exp_avg / bc1, denom, value=-lr)
    param_bf16.copy_(master.to(param_bf16.dtype))


# --------------------------------------------------------------------------
# RMSNorm / RoPE / SwiGLU (llama-family ops; torch fp32-semantics references)
# --------------------------------------------------------------------------

def rmsnorm_fwd(x: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-6):
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = (xf * rstd) * gamma.float()
    return y.to(x.dtype), rstd.squeeze(-1)


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor,
                rstd: torch.Tensor):
    xf, dyf, gf = x.float(), dy.float(), gamma.float()
    r = rstd.unsqueeze(-1)
    xh = xf * r
    dg = (dyf * xh).sum(0)
    t = dyf * gf
    dx = r * (t - xh * (t * xh).mean(-1, keepdim=True))
    return dx.to(x.dtype), dg.to(gamma.dtype)


def rope_fwd(x: torch.Tensor, seq_len: int, theta: float = 10000.0):
    """x [tokens, heads, D] (tokens = batch*seq flattened, position =
    token % seq_len); rotate-half convention."""
    T, H, D = x.shape
    pos = (torch.arange(T, device=x.device) % seq_len).float()
    i = torch.arange(D // 2, device=x.device).float()
    freq = theta ** (-2.0 * i / D)
    ang = pos[:, None] * freq[None, :]
    cos, sin = ang.cos()[:, None, :], ang.sin()[:, None, :]
    xf = x.float()
    x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
    y = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    return y.to(x.dtype)


def _rope_at_f32(x: torch.Tensor, positions: torch.Tensor, theta: float):
    D = x.shape[-1]
    i = torch.arange(D // 2, device=x.device).float()
    freq = theta ** (-2.0 * i / D)
    ang = positions.to(x.device)[..., None].float() * freq
    cos, sin = ang.cos(), ang.sin()
    xf = x.float()
    x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_at(x: torch.Tensor, positions: torch.Tensor,
            theta: float = 10000.0):
    """rope_fwd's rotation at explicit positions: x [..., D], positions an
    integer tensor broadcast over x's leading dims (e.g. [T, 1] against
    [B, T, H, D]). Torch ops on the tensors' device only, no host sync, so
    it runs inside a captured decode step with the position on the
    device."""
    return _rope_at_f32(x, positions, theta).to(x.dtype)


def rope_bwd(dy: torch.Tensor, seq_len: int, theta: float = 10000.0):
    """The inverse rotation (transpose of an orthogonal map)."""
    T, H, D = dy.shape
    pos = (torch.arange(T, device=dy.device) % seq_len).float()
    i = torch.arange(D // 2, device=dy.device).float()
    freq = theta ** (-2.0 * i / D)
    ang = pos[:, None] * freq[None, :]
    cos, sin = ang.cos()[:, None, :], ang.sin()[:, None, :]
    df = dy.float()
    d1, d2 = df[..., :D // 2], df[..., D // 2:]
    dx = torch.cat([d1 * cos + d2 * sin, d2 * cos - d1 * sin], dim=-1)
    return dx.to(dy.dtype)


def swiglu_fwd(a: torch.Tensor, b: torch.Tensor):
    af = a.float()
    return (af * torch.sigmoid(af) * b.float()).to(a.dtype)


def swiglu_bwd(dy: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    af, bf, dyf = a.float(), b.float(), dy.float()
    sig = torch.sigmoid(af)
    silu = af * sig
    da = dyf * bf * (sig + silu * (1.0 - sig))
    db = dyf * silu
    return da.to(a.dtype), db.to(b.dtype)


# --------------------------------------------------------------------------
# MoE routing / dispatch / combine (any dtype, any device; the rules the
# fused kernels in csrc/moe_route.hip implement)
# --------------------------------------------------------------------------

def _acc_dtype(t: torch.Tensor):
    return torch.promote_types(t.dtype, torch.float32)


def moe_route(gates: torch.Tensor, k: int, capacity: int):
    """gates [T, E] -> (topi [T, k], slot [T, k], src [E*C], counts [E]),
    all int32. topi[t, j] is the expert with the j-th largest gate, ties to
    the lower expert index (stable descending sort). slot = e*C + pos with
    pos the number of earlier flat entries (t*k + j order) that chose e, or
    -1 where pos >= C. src is the inverse map (-1 for an empty slot).
    counts[e] is the number of selections of e before capacity dropping."""
    T, E = gates.shape
    C = int(capacity)
    g = gates if gates.dtype in (torch.float32, torch.float64) \
        else gates.float()
    topi = torch.sort(g, dim=-1, descending=True,
                      stable=True).indices[:, :k]
    flat_e = topi.reshape(-1)
    n = flat_e.numel()
    order = torch.argsort(flat_e, stable=True)
    counts = torch.bincount(flat_e, minlength=E)
    offs = torch.cumsum(counts, 0) - counts
    r = torch.arange(n, device=gates.device)
    pos = torch.empty_like(r)
    pos[order] = r - offs[flat_e[order]]
    keep = pos < C
    slot = torch.where(keep, flat_e * C + pos, torch.full_like(pos, -1))
    src = torch.full((E * C,), -1, dtype=torch.long, device=gates.device)
    src[slot[keep]] = r[keep]
    i32 = torch.int32
    return (topi.to(i32).contiguous(), slot.reshape(T, k).to(i32),
            src.to(i32), counts.to(i32))


def moe_dispatch_fwd(x: torch.Tensor, src: torch.Tensor, k: int):
    """D[s] = x[src[s] // k] for a filled slot, zeros for an empty one."""
    s = src.long()
    rows = x[s.clamp_min(0) // k]
    return torch.where((s >= 0).unsqueeze(-1), rows, torch.zeros_like(rows))


def moe_dispatch_bwd(dD: torch.Tensor, slot: torch.Tensor):
    """dx[t] = sum over kept j of dD[slot[t, j]] (fp32 sum, one rounding)."""
    s = slot.long()
    rows = dD[s.clamp_min(0)].to(_acc_dtype(dD))             # [T, k, d]
    rows = torch.where((s >= 0).unsqueeze(-1), rows, torch.zeros_like(rows))
    return rows.sum(1).to(dD.dtype)


def moe_combine_fwd(y: torch.Tensor, w: torch.Tensor, slot: torch.Tensor):
    """out[t] = sum over kept j of w[t, j] * y[slot[t, j]]; dropped entries
    are selected away, so a never-filled slot of y has no influence."""
    s = slot.long()
    acc = _acc_dtype(y)
    rows = y[s.clamp_min(0)].to(acc) * w.to(acc).unsqueeze(-1)
    rows = torch.where((s >= 0).unsqueeze(-1), rows, torch.zeros_like(rows))
    return rows.sum(1).to(y.dtype)


def moe_combine_bwd(dout: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                    slot: torch.Tensor, src: torch.Tensor):
    """dy[s] = w[src[s]] * dout[src[s] // k] (zeros for an empty slot);
    dw[t, j] = dot(y[slot[t, j]], dout[t]) in fp32 (0 where dropped)."""
    k = slot.shape[1]
    acc = _acc_dtype(y)
    s = src.long()
    sc = s.clamp_min(0)
    dy = w.reshape(-1)[sc].to(acc).unsqueeze(-1) * dout[sc // k].to(acc)
    dy = torch.where((s >= 0).unsqueeze(-1), dy, torch.zeros_like(dy))
    sl = slot.long()
    dw = (y[sl.clamp_min(0)].to(acc) * dout.to(acc).unsqueeze(1)).sum(-1)
    dw = torch.where(sl >= 0, dw, torch.zeros_like(dw))
    return dy.to(y.dtype), dw.to(w.dtype)


# --------------------------------------------------------------------------
# Token sampling: temperature, top-k, top-p, inverse-CDF draw
# --------------------------------------------------------------------------
#
# The rules (also the HIP kernel's, csrc/sampling.hip):
#   1. top-k: tau_k = the top_k-th largest logit; z >= tau_k is kept (ties
#      at the threshold included). top_k == 0 or >= vocab: no filter.
#   2. w_i = exp2((z_i - m) * fp32(log2(e) / T)) in fp32, m the row maximum;
#      exactly 1 at z_i == m and exactly 0 at -inf. Each weight becomes the
#      integer q_i = trunc(w_i * 2^40) and every sum below is an integer
#      sum: exact, the same in any order, monotone along the row.
#   3. top-p acts on what top-k left: tau_p = the largest input value whose
#      kept tokens z >= tau_p weigh >= ceil(fp32(top_p) * W_k), W_k the
#      kept total. top_p >= 1: no filter. tau = max(tau_k, tau_p); with no
#      filter tau is the row minimum.
#   4. the token is the smallest index whose running sum of kept q reaches
#      ceil(u * W) clamped to [1, W] (W the final kept total), else the
#      last kept index; clamped to [0, vocab).
#   5. u is given, or u_b = (x >> 8) * 2^-24 + 2^-25 with x the first word
#      of Philox4x32-10(key = seed, counter = (step, b)); clamped to
#      [2^-25, 1].

_LOG2E = 1.4426950408889634
SAMPLE_FIX_BITS = 40
SAMPLE_MAX_VOCAB = 1 << 22      # vocab * 2^40 stays below 2^62


def sample_check(logits, temperature, top_k, top_p, step, u, vocab, out):
    """Argument checks of sample_logits, shared by both backends; returns
    (B, vocab). Raises ValueError before anything is launched."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("sample_logits: logits must be [B, V], B, V >= 1")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("sample_logits: logits must be fp32 or bf16, got "
                         f"{logits.dtype}")
    B, Vs = logits.shape
    if Vs > 1 and logits.stride(1) != 1:
        raise ValueError("sample_logits: the last dim must be contiguous")
    vocab = Vs if vocab is None else int(vocab)
    if not 1 <= vocab <= Vs:
        raise ValueError(f"sample_logits: vocab {vocab} not in [1, {Vs}]")
    if vocab > SAMPLE_MAX_VOCAB:
        raise ValueError(f"sample_logits: vocab {vocab} > 2^22 (the 64-bit "
                         "sums of 2^40-scaled weights would overflow)")
    if not temperature > 0:
        raise ValueError("sample_logits: temperature must be > 0 (greedy "
                         "decoding is argmax, not this op)")
    if top_k < 0 or not top_p > 0:
        raise ValueError("sample_logits: top_k >= 0 and top_p > 0")
    if (u is None) == (step is None):
        raise ValueError("sample_logits: give exactly one of u and step")
    if u is not None and (u.dtype != torch.float32 or u.device != logits.device
                          or tuple(u.shape) != (B,)):
        raise ValueError("sample_logits: u must be fp32 [B] on the logits' "
                         "device")
    if step is not None and (step.dtype != torch.int64 or step.numel() != 1
                             or step.device != logits.device):
        raise ValueError("sample_logits: step must be an int64 tensor with "
                         "one element on the logits' device")
    if out is not None and (out.dtype != torch.int64
                            or tuple(out.shape) != (B, 1)
                            or out.device != logits.device
                            or not out.is_contiguous()):
        raise ValueError("sample_logits: out must be a contiguous int64 "
                         "[B, 1] on the logits' device")
    return B, vocab


def sample_logits(logits: torch.Tensor, temperature: float, top_k: int = 0,
                  top_p: float = 1.0, seed: int = 0,
                  step: Optional[torch.Tensor] = None,
                  u: Optional[torch.Tensor] = None,
                  vocab: Optional[int] = None,
                  out: Optional[torch.Tensor] = None,
                  return_threshold: bool = False):
    B, vocab = sample_check(logits, temperature, top_k, top_p, step, u,
                            vocab, out)
    f32 = torch.float32
    z = logits[:, :vocab].float()
    z = torch.where(z == 0, torch.zeros_like(z), z)          # -0 -> +0
    if u is None:
        from tepdist_amd.ops.fp64_reference import sample_uniform
        u = torch.from_numpy(sample_uniform(
            seed, B, int(step.reshape(-1)[0]))).to(z.device)
    u = torch.nan_to_num(u.float(), nan=0.0).clamp(2.0 ** -25, 1.0)
    t32 = torch.tensor(temperature, dtype=f32).item()
    c = torch.tensor(_LOG2E / t32, dtype=f32)
    m = torch.where(torch.isnan(z), torch.full_like(z, float("-inf")),
                    z).amax(-1, keepdim=True)
    w = torch.exp2((z - m) * c)
    w = torch.where(z == m, torch.ones_like(w), w)
    w = torch.where(w >= 0, w.clamp(max=1.0), torch.zeros_like(w))
    q = (w.double() * float(2 ** SAMPLE_FIX_BITS)).long()
    zero = torch.zeros_like(q)
    tau = z.amin(-1)
    if 0 < top_k < vocab:
        tau = z.topk(top_k, dim=-1).values[:, -1]
        q = torch.where(z >= tau[:, None], q, zero)
    p32 = torch.tensor(min(top_p, 1.0), dtype=f32).double()
    if p32 < 1.0:
        Wk = q.sum(-1)
        t = torch.minimum(torch.ceil(p32 * Wk.double()).long(),
                          Wk).clamp(min=1)
        zs, idx = z.sort(dim=-1, descending=True, stable=True)
        cum = q.gather(-1, idx).cumsum(-1)
        pos = (cum < t[:, None]).sum(-1)
        tau_p = zs.gather(-1, pos.clamp(max=vocab - 1)[:, None])[:, 0]
        tau = torch.where((pos < vocab) & (Wk > 0), tau_p, tau)
        q = torch.where(z >= tau[:, None], q, zero)
    cum = q.cumsum(-1)
    W = cum[:, -1]
    tq = torch.minimum(torch.ceil(u.double() * W.double()).long(),
                       W).clamp(min=1)
    tok = (cum < tq[:, None]).sum(-1)
    kept = z >= tau[:, None]
    last = (kept * torch.arange(vocab, device=z.device)).amax(-1)
    tok = torch.where(tok < vocab, tok, last).clamp(0, vocab - 1)[:, None]
    if out is not None:
        out.copy_(tok)
        tok = out
    return (tok, tau) if return_threshold else tok
