"""Autograd-facing op layer with device dispatch.

Every op the planner shards goes through here. Dispatch:
  - CUDA (= ROCm/MI355X) tensors -> tepdist_amd.ops.hip (hand-written CDNA4
    HIP kernels; raises ImportError loudly if the extension is missing on a
    GPU machine — no silent eager fallback).
  - CPU tensors -> tepdist_amd.ops.reference (pure torch; used by CPU tests
    and as the numerics baseline).
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from tepdist_amd.ops import reference as ref


def _backend(t: torch.Tensor):
    if t.is_cuda:
        from tepdist_amd.ops import hip as be  # loud ImportError if .so missing
        return be
    return ref


# --------------------------------------------------------------------------


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, act: str):
        be = _backend(x)
        x2d = x.reshape(-1, x.shape[-1])
        y, pre_act = be.linear_fwd(x2d, w, bias, act)
        ctx.save_for_backward(x2d, w, pre_act if pre_act is not None else torch.empty(0))
        ctx.has_bias = bias is not None
        ctx.act = act
        ctx.in_shape = x.shape
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, w, pre_act = ctx.saved_tensors
        if ctx.act == "none":
            pre_act = None
        be = _backend(dy)
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx, dw, db = be.linear_bwd(dy2d, x2d, w, ctx.has_bias, ctx.act, pre_act)
        return dx.reshape(ctx.in_shape), dw, db, None


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
           act: str = "none") -> torch.Tensor:
    """y = act(x @ w^T + bias); w in [out, in] layout."""
    return LinearFn.apply(x, w, bias, act)


class MlpFn(torch.autograd.Function):
    """Fused transformer MLP: gelu epilogues ride the producing GEMMs
    (hip.mlp_fwd/mlp_bwd — hipBLASLt GELU_AUX_BIAS / DGELU_BGRAD, measured
    per shape against the composed path)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        be = _backend(x)
        x2d = x.reshape(-1, x.shape[-1]).contiguous()
        y, (h, pre) = be.mlp_fwd(x2d, w1, b1, w2, b2)
        ctx.save_for_backward(x2d, w1, w2, h, pre)
        ctx.in_shape = x.shape
        return y.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, w1, w2, h, pre = ctx.saved_tensors
        be = _backend(dy)
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx, dw1, db1, dw2, db2 = be.mlp_bwd(dy2d, x2d, w1, w2, h, pre)
        return dx.reshape(ctx.in_shape), dw1, db1, dw2, db2


def mlp(x, w1, b1, w2, b2):
    """Transformer MLP y = gelu(x@w1^T+b1)@w2^T+b2 (both biases
    required). GPU runs the fused-epilogue path; CPU composes the
    reference linears (same autograd surface)."""
    if x.is_cuda:
        return MlpFn.apply(x, w1, b1, w2, b2)
    return linear(linear(x, w1, b1, act="gelu"), w2, b2)


class MatmulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        be = _backend(a)
        ctx.save_for_backward(a, b)
        return be.matmul(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        be = _backend(dc)
        dc = dc.contiguous()
        da = be.matmul(dc, b.transpose(-1, -2))
        db = be.matmul(a.transpose(-1, -2), dc)
        return da, db


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return MatmulFn.apply(a, b)


# --------------------------------------------------------------------------


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        be = _backend(x)
        x2d = x.reshape(-1, x.shape[-1])
        y, mean, rstd = be.layernorm_fwd(x2d, gamma, beta, eps)
        ctx.save_for_backward(x2d, gamma, mean, rstd)
        ctx.in_shape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, gamma, mean, rstd = ctx.saved_tensors
        be = _backend(dy)
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx, dgamma, dbeta = be.layernorm_bwd(dy2d, x2d, gamma, mean, rstd)
        return dx.reshape(ctx.in_shape), dgamma, dbeta, None


def layernorm(x, gamma, beta, eps: float = 1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


# --------------------------------------------------------------------------


class AddLayerNormFn(torch.autograd.Function):
    """Fused residual add + layernorm: one kernel produces BOTH the
    residual sum (bf16-rounded once, bit-identical to a separate add) and
    the normalized output; backward folds the straight-through gradient
    into the layernorm dx pass (kills the autograd grad-sum add)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        ctx.set_materialize_grads(False)
        be = _backend(x)
        x2d = x.reshape(-1, x.shape[-1])
        r2d = res.reshape(-1, res.shape[-1])
        s, y, mean, rstd = be.add_layernorm_fwd(x2d, r2d, gamma, beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        ctx.in_shape = x.shape
        return s.reshape(x.shape), y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dsum, dy):
        s, gamma, mean, rstd = ctx.saved_tensors
        be = _backend(dy if dy is not None else dsum)
        if dy is None:
            # normalized output unused: grads flow through the sum only
            d = dsum.reshape(ctx.in_shape)
            return d, d, None, None, None
        dy2d = dy.reshape(-1, dy.shape[-1])
        ds2d = None if dsum is None else dsum.reshape(-1, dsum.shape[-1])
        dx, dg, db = be.add_layernorm_bwd(dy2d, ds2d, s, gamma, mean, rstd)
        dx = dx.reshape(ctx.in_shape)
        return dx, dx, dg, db, None


def add_layernorm(x, res, gamma, beta, eps: float = 1e-5):
    """(s, y) = (x + res, layernorm(x + res)). Fused on GPU; composed on
    CPU with identical autograd semantics."""
    if x.is_cuda:
        return AddLayerNormFn.apply(x, res, gamma, beta, eps)
    s = x + res
    return s, layernorm(s, gamma, beta, eps)


class SoftmaxFn(torch.autograd.Function):
    """Fused scale + optional causal mask + softmax over the last dim."""

    @staticmethod
    def forward(ctx, scores, scale, causal):
        be = _backend(scores)
        p = be.softmax_fwd(scores, scale=scale, causal=causal)
        ctx.save_for_backward(p)
        ctx.scale = scale
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        be = _backend(dp)
        ds = be.softmax_bwd(dp.contiguous(), p, scale=ctx.scale)
        return ds, None, None


def softmax(scores, scale: float = 1.0, causal: bool = False):
    return SoftmaxFn.apply(scores, scale, causal)


# --------------------------------------------------------------------------


class AttentionFn(torch.autograd.Function):
    """Causal multi-head attention on [B, H, S, D] tensors."""

    @staticmethod
    def forward(ctx, q, k, v, causal):
        be = _backend(q)
        out, residuals = be.attention_fwd(q, k, v, causal=causal)
        ctx.save_for_backward(q, k, v, *residuals)
        ctx.causal = causal
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, *residuals = ctx.saved_tensors
        be = _backend(dout)
        dq, dk, dv = be.attention_bwd(dout.contiguous(), q, k, v,
                                      tuple(residuals), causal=ctx.causal)
        return dq, dk, dv, None


def attention(q, k, v, causal: bool = True):
    return AttentionFn.apply(q, k, v, causal)


class AttentionQKVFn(torch.autograd.Function):
    """Attention on the packed qkv projection [B, S, 3*H*D]: the GPU flash
    kernels consume/produce the packed layout directly (no transposes)."""

    @staticmethod
    def forward(ctx, qkv, heads, causal):
        be = _backend(qkv)
        r = be.attention_qkv_fwd(qkv, heads, causal=causal) \
            if hasattr(be, "attention_qkv_fwd") else None
        if r is None:  # hip fallback for unsupported head dims
            r = ref.attention_qkv_fwd(qkv.cpu(), heads, causal) \
                if not qkv.is_cuda else _qkv_composed(be, qkv, heads, causal)
        out, residuals = r
        ctx.save_for_backward(qkv, *residuals)
        ctx.heads = heads
        ctx.causal = causal
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, *residuals = ctx.saved_tensors
        be = _backend(dout)
        dqkv = be.attention_qkv_bwd(dout.contiguous(), qkv, ctx.heads,
                                    tuple(residuals), causal=ctx.causal)
        return dqkv, None, None


def _qkv_composed(be, qkv, heads, causal):
    B, S, d3 = qkv.shape
    d = d3 // 3
    D = d // heads
    q, k, v = (t.reshape(B, S, heads, D).transpose(1, 2).contiguous()
               for t in qkv.split(d, dim=-1))
    out4, res = be.attention_fwd(q, k, v, causal=causal)
    return out4.transpose(1, 2).reshape(B, S, d), (q, k, v) + res


def attention_qkv(qkv, heads: int, causal: bool = True):
    return AttentionQKVFn.apply(qkv, heads, causal)


def decode_attention(q, k_cache, v_cache, positions, k_new=None, v_new=None,
                     scale: Optional[float] = None,
                     splits: Optional[int] = None,
                     rope_theta: Optional[float] = None):
    """Single-query attention over a KV cache (inference only, no
    autograd). q [B, H, D], k_new/v_new [B, Hkv, D], caches
    [B, Hkv, S_max, D], positions int64 [1] or [B] on the tensors' device.
    Hkv < H is grouped-query attention: query head h attends K/V head
    h // (H // Hkv). With (k_new, v_new) the new row is written in place
    into cache[b, :, positions[b]] and attended to; otherwise cache rows
    0..positions[b] are attended. With `rope_theta`, q and k_new are
    rotated (rotate-half, as ops.rope) by the clamped position first: q in
    fp32 without rounding, k_new rounded once to the cache dtype, so the
    cache holds rotated rows. `splits` (GPU only) pins the KV split count;
    None = host heuristic."""
    for t in (q, k_cache, v_cache, k_new, v_new):
        assert t is None or not t.requires_grad, \
            "decode_attention has no backward"
    be = _backend(q)
    if be is ref:
        return ref.decode_attention(q, k_cache, v_cache, positions, k_new,
                                    v_new, scale, rope_theta)
    return be.decode_attention(q, k_cache, v_cache, positions, k_new, v_new,
                               scale, splits, rope_theta)


def sample_logits(logits, *, temperature: float, top_k: int = 0,
                  top_p: float = 1.0, seed: int = 0, step=None, u=None,
                  vocab: Optional[int] = None, out=None,
                  return_threshold: bool = False):
    """One sampled token per row: int64 [B, 1] (inference only, no
    autograd). logits [B, Vs] fp32 or bf16, last dim contiguous, any row
    stride; only columns < vocab (default Vs) take part. temperature > 0.
    top_k: keep the top_k largest logits, ties at the k-th value included
    (0 or >= vocab: off). top_p: of what top-k left, keep the smallest set
    of largest logits holding >= top_p of the mass (>= 1: off). The token
    is drawn by inverse CDF in index order from `u` (fp32 [B]) or, with
    `step` (int64 [1] on the logits' device, read on the device), from the
    first Philox4x32-10 word of (seed, row, step): the same on CPU and GPU,
    for any batch size, in a graph or out of one. `out` (int64 [B, 1]) is
    written in place and returned. return_threshold: also returns the
    final threshold tau (fp32 [B]): logits >= tau were kept. The token is
    always in [0, vocab). The rules in full: ops/reference.py."""
    assert not logits.requires_grad, "sample_logits has no backward"
    return _backend(logits).sample_logits(
        logits, temperature, top_k, top_p, seed, step, u, vocab, out,
        return_threshold)


# --------------------------------------------------------------------------
# MoE routing / dispatch / combine
# --------------------------------------------------------------------------


class MoERoute(NamedTuple):
    """Slot maps of one routing decision (all int32): topi [T, k] chosen
    experts, slot [T, k] = e*C + pos or -1 (dropped), src [E*C] = t*k + j
    or -1 (empty), counts [E] selections per expert before dropping."""
    topi: torch.Tensor
    slot: torch.Tensor
    src: torch.Tensor
    counts: torch.Tensor


def moe_route(gates, k: int, capacity: int) -> MoERoute:
    """Top-k routing with static capacity for gates [T, E] (no autograd).
    Ties go to the lower expert index; positions within an expert follow
    the flat (t, j) order. See reference.moe_route for the exact rules."""
    return MoERoute(*_backend(gates).moe_route(gates.detach(), k, capacity))


class MoEDispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, src, slot):
        ctx.save_for_backward(slot)
        return _backend(x).moe_dispatch_fwd(x.contiguous(), src,
                                            slot.shape[1])

    @staticmethod
    def backward(ctx, dD):
        (slot,) = ctx.saved_tensors
        return _backend(dD).moe_dispatch_bwd(dD.contiguous(), slot), \
            None, None


def moe_dispatch(x, route: MoERoute):
    """x [T, d] -> D [E*C, d]: slot s holds the token route.src[s] // k, an
    empty slot holds zeros. Autograd to x."""
    return MoEDispatchFn.apply(x, route.src, route.slot)


class MoECombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, w, slot, src):
        y = y.contiguous()
        w = w.contiguous()
        ctx.save_for_backward(y, w, slot, src)
        return _backend(y).moe_combine_fwd(y, w, slot)

    @staticmethod
    def backward(ctx, dout):
        y, w, slot, src = ctx.saved_tensors
        dy, dw = _backend(dout).moe_combine_bwd(dout.contiguous(), y, w,
                                                slot, src)
        return dy, dw, None, None


def moe_combine(y, weights, route: MoERoute):
    """y [E*C, d], weights [T, k] fp32 -> out [T, d] = sum over kept j of
    weights[t, j] * y[route.slot[t, j]]. Autograd to y and weights; what a
    never-filled slot of y holds does not reach the output."""
    return MoECombineFn.apply(y, weights, route.slot, route.src)


# --------------------------------------------------------------------------


class GeluFn(torch.autograd.Function):
    """Standalone tanh-gelu (the IR's `gelu` op; linear fuses its own)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _backend(x).gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _backend(x).gelu_bwd(dy.contiguous(), x)


def gelu(x):
    return GeluFn.apply(x)


class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table):
        be = _backend(table)
        ctx.save_for_backward(ids)
        ctx.vocab = table.shape[0]
        return be.embedding_fwd(ids, table)

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        be = _backend(dy)
        return None, be.embedding_bwd(dy.contiguous(), ids, ctx.vocab)


def embedding(ids, table):
    return EmbeddingFn.apply(ids, table)


# --------------------------------------------------------------------------


class CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        be = _backend(logits)
        loss, lse = be.cross_entropy_fwd(logits, targets, ignore_index)
        ctx.save_for_backward(logits, targets, lse)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse = ctx.saved_tensors
        be = _backend(logits)
        dl = be.cross_entropy_bwd(dloss, logits, targets, lse, ctx.ignore_index)
        return dl, None, None


def cross_entropy(logits, targets, ignore_index: int = -1):
    """Mean NLL over non-ignored targets; logits [M, V], targets [M]."""
    return CrossEntropyFn.apply(logits, targets, ignore_index)


# --------------------------------------------------------------------------


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        be = _backend(x)
        y, mask = be.dropout_fwd(x, p, seed, offset)
        ctx.save_for_backward(mask if mask is not None else torch.empty(0))
        ctx.p = p
        ctx.has_mask = mask is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        be = _backend(dy)
        dx = be.dropout_bwd(dy.contiguous(), mask if ctx.has_mask else None, ctx.p)
        return dx, None, None, None


def dropout(x, p: float, seed: int = 0, offset: int = 0):
    if p == 0.0:
        return x
    return DropoutFn.apply(x, p, seed, offset)


def adamw_step(param, master, grad, exp_avg, exp_avg_sq, *, lr, beta1=0.9,
               beta2=0.999, eps=1e-8, weight_decay=0.01, step=1):
    be = _backend(param)
    be.adamw_step(param, master, grad, exp_avg, exp_avg_sq, lr, beta1, beta2,
                  eps, weight_decay, step)


# --------------------------------------------------------------------------
# RMSNorm / RoPE / SwiGLU (llama family)
# --------------------------------------------------------------------------


class RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, eps):
        be = _backend(x)
        x2d = x.reshape(-1, x.shape[-1])
        y, rstd = be.rmsnorm_fwd(x2d, gamma, eps)
        ctx.save_for_backward(x2d, gamma, rstd)
        ctx.in_shape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, gamma, rstd = ctx.saved_tensors
        be = _backend(dy)
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx, dg = be.rmsnorm_bwd(dy2d, x2d, gamma, rstd)
        return dx.reshape(ctx.in_shape), dg, None


def rmsnorm(x, gamma, eps: float = 1e-6):
    return RMSNormFn.apply(x, gamma, eps)


class RoPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seq_len, theta):
        be = _backend(x)
        ctx.seq_len, ctx.theta = seq_len, theta
        return be.rope_fwd(x.contiguous(), seq_len, theta)

    @staticmethod
    def backward(ctx, dy):
        be = _backend(dy)
        return be.rope_bwd(dy.contiguous(), ctx.seq_len, ctx.theta), \
            None, None


def rope(x, seq_len: int, theta: float = 10000.0):
    """Rotary position embedding over [tokens, heads, head_dim]
    (rotate-half convention; position = token index % seq_len)."""
    return RoPEFn.apply(x, seq_len, theta)


class SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        be = _backend(a)
        ctx.save_for_backward(a, b)
        return be.swiglu_fwd(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        be = _backend(dy)
        da, db = be.swiglu_bwd(dy.contiguous(), a.contiguous(),
                               b.contiguous())
        return da, db


def swiglu(a, b):
    return SwiGLUFn.apply(a, b)

