"""Autoregressive generation with a KV cache (serving path; beyond the
reference's training-only scope).

Prefill runs the flash kernels over the whole prompt while recording K/V;
decode steps run one token at a time against the cache (at q_len = 1 the
GEMV-shaped attention is bandwidth bound — the cache layout
[B, H, S_max, D] keeps the K/V reads contiguous). decode_attn selects how:
"fused" = ops.decode_attention, one kernel per layer that appends the new
K/V row and attends over the valid rows only; "composed" = batched
matmuls + softmax over the cache; "auto" (default, or
TEPDIST_DECODE_ATTN) = fused for bf16 with head dim 64/128 on the GPU
(measured +51% decode tokens/s, docs/KERNELS.md), composed otherwise and
on CPU. The engine reads the model's parameters directly (tp = 1
layout of models/gpt2.py), so no changes to the training forward.

Llama models (models/llama.py, MHA or grouped-query) are served by the
same Generator: caches are [B, Hkv, S_max, D] and hold ROTATED K rows; the
fused step is one ops.decode_attention(..., rope_theta=...) per layer that
rotates q and the new K row at the device position, appends and attends
with each K/V row read once per query group. "auto" fuses every group
size the kernel covers (FUSED_GROUPS): measured 4-10x faster per call than
the composed GQA step at every (D, G), 2.1x decode tokens/s on
llama-1b-gqa (docs/KERNELS.md "Decode attention: GQA + RoPE").

Sampling (temperature > 0, top-k, top-p): generate(..., sampler=) or
TEPDIST_SAMPLER picks "host" (default: softmax on the device, draw on the
CPU, eager loop), "device" (ops.sample_logits, which on the GPU keeps the
sampled step inside the captured decode graph) or "auto"
(docs/KERNELS.md "Sampling").

Decode-step linears (decode_linear=, or TEPDIST_DECODE_LINEAR): "gemm"
(default) = ops.linear at every site, as before; "skinny" = every
single-token linear runs ops.linear_decode / ops.swiglu_linear_decode (the
skinny weight-streaming kernel, with the residual add, bias + gelu and
SwiGLU folded into its epilogue) and a site the kernel does not cover
raises; "auto" = the same at the sites the kernel covers and measured
faster than the library (hip.skinny_auto), ops.linear elsewhere
(docs/KERNELS.md "Decode linears"). Prefill is untouched.

Prefill attention (prefill_attn=, or TEPDIST_PREFILL_ATTN): every pass over
more than one token, the first chunk and a continuation chunk alike.
"composed" (default) = as before: the first chunk ropes, writes the cache,
expands K/V to H heads and runs the training flash forward; a continuation
chunk runs batched matmuls + softmax over the cache. "fused" = one
ops.prefill_attention per layer on views of the packed projection: it
rotates q and the chunk's K rows at the device position, appends K/V to the
cache and attends cache rows 0 .. pos + t with each K/V row staged once per
query group; a site the kernel does not cover raises. "auto" = fused where
the kernel covers the call and hip.prefill_auto has it measured ahead,
composed elsewhere and on CPU (docs/KERNELS.md "Prefill attention over the
cache"). generate(..., prefill_chunk=c) feeds the prompt in chunks of c
tokens.

Weight format (weight_format=, or TEPDIST_WEIGHT_FORMAT): "bf16" (default)
= the model's own weights, every path above as it was. "mxfp8" / "mxfp4" =
weight-only OCP MX quantization (ops/mx.py): the constructor quantizes every
block linear and the head once (Llama: qkv, o, gate, up, down, lm_head;
GPT-2: qkv, proj, fc, out and wte as the head; embedding lookups, norms and
biases stay bf16), and the model served is the quantized model at every
site. A single-token site the MX plan covers runs ops.linear_decode_mx /
ops.swiglu_linear_decode_mx with its fused epilogue, whatever decode_linear
says: there is no "auto" rule, since going back to the bf16 weights would
change the model. Every other site (T > 1, M > 64) runs ops.mx_dequantize
into one scratch buffer sized for the largest weight, allocated once so a
captured step can reuse it, then ops.linear (docs/KERNELS.md "Decode
linears: MX weights"), unless mx_linear says otherwise.

Those other MX sites (mx_linear=, or TEPDIST_MX_LINEAR): "dequant" (default)
= the dequantize-then-ops.linear path above, unchanged. "fused" = every MX
site the skinny MX kernel does not take runs ops.linear_mx, the LDS-tiled
kernel that reads codes and scales as they lie, with the residual add and
bias + gelu in its epilogue (Llama's gate and up are two calls and then
ops.swiglu); a site it does not cover raises. "auto" = the same where the
plan covers the site and hip.mx_gemm_auto has it measured ahead, the
dequantize path elsewhere and on CPU. All three serve the same quantized
model: only the order of the fp32 sums differs (docs/KERNELS.md "Prefill and
large-batch linears: MX weights").

Activation format (act_format=, or TEPDIST_ACT_FORMAT): "bf16" (default) =
every path above as it was. "mxfp8" = W4A8 / W8A8: the input of every
quantized linear (quantized_params) is quantized to MXFP8 by the rule of
ops/mx.py, at every site and every T, so prefill and decode serve one model,
and it is a different model from the weight-only one. It needs a
weight_format other than "bf16" and mx_linear left at its default. Sites of
T > 1 or M > 64 run ops.linear_mx_a8, the scaled-MFMA kernel that multiplies
codes by codes (Llama's gate and up share one ops.mx_quantize_act of the
normed input, then ops.swiglu); a site its plan refuses raises. Single-token
sites the skinny MX plan covers run ops.mx_quantize_act(x, roundtrip=True)
into a buffer allocated once, then ops.linear_decode_mx /
ops.swiglu_linear_decode_mx as before: the same values, only the order of
the fp32 sum differs. "mxfp4" = W4A4: the same routing with e2m1 activation
blocks (ops.mx_quantize_act(..., fmt="mxfp4"), ops.linear_mx_a8 on the
e2m1 x e2m1 form of the scaled MFMA), valid only with weight_format="mxfp4"
(W8A4 is not built) and mx_linear at its default; yet another model. There
is no "auto" rule yet (docs/KERNELS.md "MX weights x MXFP8 activations", "MX
weights x MXFP4 activations").

Llama's MLP under an MX act_format (mx_mlp=, or TEPDIST_MX_MLP): "composed"
(default) = the path above, unchanged. "fused" = at the sites of T > 1 or
M > 64 the MLP is three launches: ops.mx_quantize_act of the normed input,
ops.linear_mx_a8(..., act="swiglu", up=, out_format=act_format), which
computes gate, up and silu(g) * u in one kernel and writes the hidden
activations as MX codes, and ops.linear_mx_a8 of those codes against w_down
with the residual. It rounds silu(g) * u once where the composed path rounds
g and u to bf16 first: yet another model, on CPU (the reference ops) and GPU
alike. It needs an act_format other than "bf16"; single-token sites and GPT-2
are unchanged (docs/KERNELS.md "Fused SwiGLU gate/up on MX activations").

KV cache format (kv_format=, or TEPDIST_KV_FORMAT): "bf16" (default) = every
path above as it was. "mxfp8" = the caches are mx.MXCache (e4m3 codes and one
e8m0 scale byte per 32 elements of a row, 51.6 % of the bf16 bytes): every
K/V row is quantized by the rule of ops/mx.py as it is appended, and every
attention reads the quantized rows, so prefill and decode serve one model, a
different one from the bf16-cache model; nothing selects it automatically.
Single-token steps run ops.decode_attention and passes over more than one
token ops.prefill_attention (the first chunk included) on the MXCache,
whatever decode_attn and prefill_attn say. Where the GPU kernels do not cover
the model (head dim, group size, dtype) and on CPU, the same two ops run as
the reference ops on the same MXCache; there is never a bf16 copy of the
cache (docs/KERNELS.md "MXFP8 KV cache")."""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

from tepdist_amd import ops
from tepdist_amd.models.llama import Llama
from tepdist_amd.ops import mx
from tepdist_amd.ops import reference as ref

# query-group sizes H / Hkv the fused decode kernel covers
FUSED_GROUPS = (1, 2, 4, 8)


class Generator:
    def __init__(self, model, max_seq: Optional[int] = None,
                 decode_attn: Optional[str] = None,
                 decode_linear: Optional[str] = None,
                 prefill_attn: Optional[str] = None,
                 weight_format: Optional[str] = None,
                 mx_linear: Optional[str] = None,
                 act_format: Optional[str] = None,
                 kv_format: Optional[str] = None,
                 mx_mlp: Optional[str] = None):
        assert model.env.tp_size == 1, "generation engine: tp=1 layout"
        self.m = model
        self.cfg = model.cfg
        self.llama = isinstance(model, Llama)
        # K/V heads of the caches (GQA: fewer than the query heads)
        self.kv_heads = self.cfg.kv_heads if self.llama else self.cfg.n_head
        self.max_seq = max_seq or self.cfg.n_ctx
        if decode_attn is None:
            decode_attn = os.environ.get("TEPDIST_DECODE_ATTN", "auto")
        if decode_attn not in ("fused", "composed", "auto"):
            raise ValueError(
                f"decode_attn must be 'fused', 'composed' or 'auto', "
                f"got {decode_attn!r}")
        self.decode_attn = decode_attn
        if decode_linear is None:
            decode_linear = os.environ.get("TEPDIST_DECODE_LINEAR", "gemm")
        if decode_linear not in ("gemm", "skinny", "auto"):
            raise ValueError(
                f"decode_linear must be 'gemm', 'skinny' or 'auto', "
                f"got {decode_linear!r}")
        self.decode_linear = decode_linear
        if prefill_attn is None:
            prefill_attn = os.environ.get("TEPDIST_PREFILL_ATTN", "composed")
        if prefill_attn not in ("composed", "fused", "auto"):
            raise ValueError(
                f"prefill_attn must be 'composed', 'fused' or 'auto', "
                f"got {prefill_attn!r}")
        self.prefill_attn = prefill_attn
        if weight_format is None:
            weight_format = os.environ.get("TEPDIST_WEIGHT_FORMAT", "bf16")
        if weight_format not in ("bf16",) + mx.FORMATS:
            raise ValueError(
                f"weight_format must be 'bf16', 'mxfp8' or 'mxfp4', "
                f"got {weight_format!r}")
        self.weight_format = weight_format
        if mx_linear is None:
            mx_linear = os.environ.get("TEPDIST_MX_LINEAR", "dequant")
        if mx_linear not in ("dequant", "fused", "auto"):
            raise ValueError(
                f"mx_linear must be 'dequant', 'fused' or 'auto', "
                f"got {mx_linear!r}")
        self.mx_linear = mx_linear
        if act_format is None:
            act_format = os.environ.get("TEPDIST_ACT_FORMAT", "bf16")
        if act_format not in ("bf16",) + mx.FORMATS:
            raise ValueError(
                f"act_format must be 'bf16', 'mxfp8' or 'mxfp4', "
                f"got {act_format!r}")
        if act_format == "mxfp8" and (weight_format == "bf16"
                                      or mx_linear != "dequant"):
            raise ValueError(
                "act_format='mxfp8' needs an MX weight_format and mx_linear "
                f"at its default, got weight_format={weight_format!r}, "
                f"mx_linear={mx_linear!r}")
        if act_format == "mxfp4" and (weight_format != "mxfp4"
                                      or mx_linear != "dequant"):
            raise ValueError(
                "act_format='mxfp4' needs weight_format='mxfp4' (W8A4 is not "
                "built) and mx_linear at its default, got weight_format="
                f"{weight_format!r}, mx_linear={mx_linear!r}")
        self.act_format = act_format
        if kv_format is None:
            kv_format = os.environ.get("TEPDIST_KV_FORMAT", "bf16")
        if kv_format not in ("bf16", "mxfp8"):
            raise ValueError(
                f"kv_format must be 'bf16' or 'mxfp8', got {kv_format!r}")
        self.kv_format = kv_format
        if mx_mlp is None:
            mx_mlp = os.environ.get("TEPDIST_MX_MLP", "composed")
        if mx_mlp not in ("composed", "fused"):
            raise ValueError(
                f"mx_mlp must be 'composed' or 'fused', got {mx_mlp!r}")
        if mx_mlp == "fused" and act_format == "bf16":
            raise ValueError(
                "mx_mlp='fused' needs an MX act_format, got act_format="
                f"{act_format!r}")
        self.mx_mlp = mx_mlp
        # id(parameter) -> its MXWeight; empty = serve the bf16 weights
        self.mxw = {}
        if weight_format != "bf16":
            ws = self.quantized_params(model)
            self.mxw = {id(w): mx.mx_quantize(w, weight_format) for w in ws}
            self._dq = torch.empty(max(w.numel() for w in ws),
                                   dtype=torch.bfloat16, device=ws[0].device)
            if act_format != "bf16":    # round trip of a single-token input
                self._xr = torch.empty(64 * max(w.shape[1] for w in ws),
                                       dtype=torch.bfloat16,
                                       device=ws[0].device)

    @staticmethod
    def quantized_params(model):
        """The weights a weight_format other than "bf16" quantizes: every
        block linear and the head."""
        if isinstance(model, Llama):
            names, head = ("w_qkv", "w_o", "w_gate", "w_up", "w_down"), \
                model.lm_head
        else:
            names, head = ("w_qkv", "w_proj", "w_fc", "w_out"), model.wte
        return [getattr(b, n) for b in model.blocks for n in names] + [head]

    def _mx_site(self, x2, mw, bias=None, act="none", residual=None,
                 mw_up=None) -> bool:
        """Whether a single-token site on x2 [M, K] runs the MX decode ops:
        on CUDA where the MX plan covers it, on CPU (the reference op)
        always."""
        if not x2.is_cuda:
            return True
        from tepdist_amd.ops import hip
        return not hip.skinny_mx_why_not(
            x2, mw, hip.skinny_epi(bias, act, residual), mw_up, residual)

    def _mx_fused(self, x2, mw, bias=None, act="none", residual=None) -> bool:
        """Whether an MX site on x2 [M, K] that the skinny MX kernel left
        runs ops.linear_mx. "dequant": never. "fused": always (on the GPU a
        site the plan does not cover raises; on CPU it is the reference
        op). "auto": on the GPU, where the plan covers the site and
        hip.mx_gemm_auto has it measured ahead; never on CPU."""
        if self.mx_linear == "dequant":
            return False
        if not x2.is_cuda:
            return self.mx_linear == "fused"
        from tepdist_amd.ops import hip
        epi = hip.skinny_epi(bias, act, residual)
        why = hip.mx_gemm_why_not(x2, mw, epi, residual)
        if self.mx_linear == "fused":
            if why:
                raise ValueError(
                    f"mx_linear='fused': site x{tuple(x2.shape)} w"
                    f"{tuple(mw.shape)} is not covered: {why}")
            return True
        return not why and hip.mx_gemm_auto(
            x2.shape[0], mw.shape[0], mw.shape[1], mx.bits(mw.fmt), epi)

    def _roundtrip(self, x2):
        """The act_format round trip of x2 [M, K] in the buffer of the
        single-token sites (M <= 64 there): valid until the next call."""
        M, K = x2.shape
        out = self._xr[:M * K].view(M, K) \
            if M * K <= self._xr.numel() and x2.dtype == self._xr.dtype \
            else None
        return ops.mx_quantize_act(x2, roundtrip=True, out=out,
                                   fmt=self.act_format)

    def _dequantized(self, mw, dtype):
        """bf16 weight of mw in the shared scratch buffer: valid until the
        next call."""
        N, K = mw.shape
        w = ops.mx_dequantize(mw, out=self._dq[:N * K].view(N, K))
        return w if dtype == w.dtype else w.to(dtype)

    def new_caches(self, B: int, S_max: int, device, dtype):
        """Per-layer K and V caches [B, Hkv, S_max, D] in self.kv_format."""
        D = self.cfg.n_embd // self.cfg.n_head
        n = self.cfg.n_layer
        if self.kv_format == "mxfp8":
            return tuple([mx.kv_cache(B, self.kv_heads, S_max, D, device)
                          for _ in range(n)] for _ in range(2))
        return tuple([torch.zeros(B, self.kv_heads, S_max, D, dtype=dtype,
                                  device=device) for _ in range(n)]
                     for _ in range(2))

    def _kv8_ops(self, x, kc, H, Hkv, D):
        """The module whose decode_attention / prefill_attention serve MXFP8
        caches, or None for bf16 caches: the public ops (the HIP kernels) on
        the GPU where they cover the model, the reference ops on the same
        MXCache elsewhere and on CPU."""
        if not isinstance(kc[0], mx.MXCache):
            return None
        if x.is_cuda:
            from tepdist_amd.ops import hip
            if not hip.prefill_why_not(x.dtype, H, Hkv, D):
                return ops
        return ref

    def _fused_decode(self, x, D, G: int = 1) -> bool:
        """Whether single-token steps on tensors like x run the fused
        ops.decode_attention. On CUDA the kernel covers bf16 with head dim
        64/128 and G = H / Hkv query heads per K/V head in FUSED_GROUPS;
        anything else stays composed (same policy as hip.attention_fwd).
        On CPU only an explicit "fused" selects the reference op, so
        "auto" leaves the CPU engine as it was."""
        if self.decode_attn == "composed":
            return False
        if x.is_cuda:
            return x.dtype == torch.bfloat16 and D in (64, 128) \
                and G in FUSED_GROUPS
        return self.decode_attn == "fused"

    def _fused_prefill(self, x, H, Hkv, D) -> bool:
        """Whether a pass of T > 1 tokens x [B, T, H * D] runs
        ops.prefill_attention. "fused": always (on the GPU the op raises at
        a site the kernel does not cover; on CPU it is the reference op).
        "auto": on the GPU, where the kernel covers the call and
        hip.prefill_auto has it measured ahead; never on CPU."""
        if self.prefill_attn != "auto":
            return self.prefill_attn == "fused"
        if not x.is_cuda:
            return False
        from tepdist_amd.ops import hip
        return not hip.prefill_why_not(x.dtype, H, Hkv, D) and \
            hip.prefill_auto(x.shape[0], x.shape[1], Hkv, H // Hkv, D)

    def _skinny_site(self, x2, w, bias=None, act="none", residual=None,
                     w_up=None) -> bool:
        """Whether a single-token linear site on x2 [M, K] runs the decode
        ops. "gemm": never. On CUDA the skinny plan decides: a site it does
        not cover raises under "skinny" and stays on ops.linear under
        "auto", as does a covered site that hip.skinny_auto leaves out. On CPU only an explicit "skinny" selects the reference op."""
        if self.decode_linear == "gemm":
            return False
        if not x2.is_cuda:
            return self.decode_linear == "skinny"
        from tepdist_amd.ops import hip
        epi = hip.skinny_epi(bias, act, residual)
        why = hip.skinny_why_not(x2, w, epi, w_up, residual)
        if not why and self.decode_linear == "auto" and not hip.skinny_auto(
                x2.shape[0], w.shape[0], w.shape[1], epi, w_up is not None):
            return False            # covered, but measured no faster
        if why and self.decode_linear == "skinny":
            raise ValueError(
                f"decode_linear='skinny': site x{tuple(x2.shape)} w"
                f"{tuple(w.shape)} is not covered: {why}")
        return not why

    def _linear(self, x, w, bias=None, act="none", residual=None,
                decode=False):
        """residual + act(x @ w^T + bias) in residual's shape (x's leading
        dims without one). decode: a single-token site, which may run
        ops.linear_decode with everything in its epilogue."""
        mw = self.mxw.get(id(w))
        if mw is not None:
            x2 = x.reshape(-1, x.shape[-1])
            r2 = None if residual is None else \
                residual.reshape(-1, w.shape[0])
            if self.act_format != "bf16":
                if decode and self._mx_site(x2, mw, bias, act, r2):
                    y = ops.linear_decode_mx(self._roundtrip(x2), mw, bias,
                                             act, r2)
                else:
                    y = ops.linear_mx_a8(x2, mw, bias, act, r2,
                                         self.act_format)
                return y.reshape(*x.shape[:-1], w.shape[0]) \
                    if residual is None else y.reshape(residual.shape)
            if decode and self._mx_site(x2, mw, bias, act, r2):
                y = ops.linear_decode_mx(x2, mw, bias, act, r2)
                return y.reshape(*x.shape[:-1], w.shape[0]) \
                    if residual is None else y.reshape(residual.shape)
            if self._mx_fused(x2, mw, bias, act, r2):
                y = ops.linear_mx(x2, mw, bias, act, r2)
                return y.reshape(*x.shape[:-1], w.shape[0]) \
                    if residual is None else y.reshape(residual.shape)
            w = self._dequantized(mw, x.dtype)
        elif decode:
            x2 = x.reshape(-1, x.shape[-1])
            r2 = None if residual is None else \
                residual.reshape(-1, w.shape[0])
            if self._skinny_site(x2, w, bias, act, r2):
                y = ops.linear_decode(x2, w, bias, act, r2)
                return y.reshape(*x.shape[:-1], w.shape[0]) \
                    if residual is None else y.reshape(residual.shape)
        y = ops.linear(x, w, bias, act)
        return y if residual is None else residual + y.reshape(residual.shape)

    # -- one transformer stack pass over new tokens x [B, T, d], with
    # caches kc/vc [L][B, H, S_max, D] filled up to `pos` -----------------

    def _stack(self, x, kc, vc, pos):
        if self.llama:
            return self._stack_llama(x, kc, vc, pos)
        cfg = self.cfg
        B, T, d = x.shape
        H = cfg.n_head
        D = d // H
        scale = 1.0 / math.sqrt(D)
        fused = T == 1 and self._fused_decode(x, D)
        pf = T > 1 and self._fused_prefill(x, H, H, D)
        att = self._kv8_ops(x, kc, H, H, D)
        if att is not None:        # MXFP8 caches: always the two cache ops
            fused, pf = T == 1, T > 1
        else:
            att = ops
        if fused or pf:
            pos_t = torch.full((1,), pos, device=x.device, dtype=torch.long)
        for li, blk in enumerate(self.m.blocks):
            h = ops.layernorm(x, blk.ln1_g, blk.ln1_b, cfg.ln_eps)
            qkv = self._linear(h, blk.w_qkv, blk.b_qkv, decode=T == 1)
            if pf:
                # one op: cache append at pos.. and attention over
                # 0..pos + t, on views of the packed projection
                q4 = qkv.view(B, T, 3, H, D)
                a = att.prefill_attention(q4[:, :, 0], kc[li], vc[li], pos_t,
                                          k_new=q4[:, :, 1],
                                          v_new=q4[:, :, 2]).reshape(B, T, d)
            elif fused:
                # one kernel: cache append at pos + attention over 0..pos,
                # reading q/k/v as views of the packed projection
                q3 = qkv.view(B, 3, H, D)
                a = att.decode_attention(q3[:, 0], kc[li], vc[li], pos_t,
                                         k_new=q3[:, 1],
                                         v_new=q3[:, 2]).reshape(B, 1, d)
            else:
                q, k, v = qkv.split(d, dim=-1)

                def heads(t):
                    return t.reshape(B, T, H, D).transpose(1, 2)  # [B,H,T,D]
                qh, kh, vh = heads(q), heads(k), heads(v)
                kc[li][:, :, pos:pos + T] = kh
                vc[li][:, :, pos:pos + T] = vh
                if T > 1 and pos == 0:
                    a = ops.attention(qh.contiguous(), kh.contiguous(),
                                      vh.contiguous(), causal=True)
                else:
                    # decode: q over the whole cache (composed, GEMV-shaped)
                    kall = kc[li][:, :, :pos + T]
                    vall = vc[li][:, :, :pos + T]
                    scores = ops.matmul(qh.contiguous(),
                                        kall.transpose(-1, -2)) * scale
                    if T > 1:  # chunked prefill continuation: causal inside
                        qpos = torch.arange(pos, pos + T, device=x.device)
                        kpos = torch.arange(pos + T, device=x.device)
                        mask = kpos[None, :] > qpos[:, None]
                        scores = scores.masked_fill(mask, float("-inf"))
                    p = torch.softmax(scores.float(), dim=-1).to(vall.dtype)
                    a = ops.matmul(p, vall.contiguous())
                a = a.transpose(1, 2).reshape(B, T, d)
            x = self._linear(a, blk.w_proj, blk.b_proj, residual=x,
                             decode=T == 1)
            h = ops.layernorm(x, blk.ln2_g, blk.ln2_b, cfg.ln_eps)
            h = self._linear(h, blk.w_fc, blk.b_fc, act="gelu",
                             decode=T == 1)
            x = self._linear(h, blk.w_out, blk.b_out, residual=x,
                             decode=T == 1)
        return x

    def _logits(self, x):
        if self.llama:
            h = ops.rmsnorm(x[:, -1], self.m.ln_f_g, self.cfg.rms_eps)
            return self._linear(h, self.m.lm_head,   # untied head
                                decode=x.shape[1] == 1)[:, None]
        x = ops.layernorm(x, self.m.lnf_g, self.m.lnf_b, self.cfg.ln_eps)
        return self._linear(x[:, -1:], self.m.wte,   # last position only
                            decode=x.shape[1] == 1)

    def _embed(self, ids, pos_ids):
        """Input embedding of ids [B, T]; pos_ids [T] (or [1]) only feeds
        GPT-2's learned position table (Llama's positions enter by rope)."""
        if self.llama:
            B, T = ids.shape
            return ops.embedding(ids.reshape(-1), self.m.wte).reshape(
                B, T, -1)
        return ops.embedding(ids, self.m.wte) + ops.embedding(pos_ids,
                                                              self.m.wpe)

    # -- Llama block: RMSNorm -> packed qkv [q | k | v] -> rope ->
    # attention -> w_o, RMSNorm -> SwiGLU. `positions` is a device int64
    # tensor ([T], or [1] in the graph step); the caches hold rotated K ---

    def _llama_mlp(self, x, blk):
        cfg = self.cfg
        B, T, d = x.shape
        hn = ops.rmsnorm(x.reshape(B * T, d), blk.ln2_g, cfg.rms_eps)
        mg, mu = self.mxw.get(id(blk.w_gate)), self.mxw.get(id(blk.w_up))
        if mg is not None and self.act_format != "bf16":
            if T == 1 and self._mx_site(hn, mg, mw_up=mu):
                h = ops.swiglu_linear_decode_mx(self._roundtrip(hn), mg, mu)
            elif self.mx_mlp == "fused":    # quantizer, gate/up/swiglu, down
                xq = ops.mx_quantize_act(hn, fmt=self.act_format)
                hq = ops.linear_mx_a8(xq, mg, act="swiglu", up=mu,
                                      out_format=self.act_format)
                y = ops.linear_mx_a8(hq, self.mxw[id(blk.w_down)],
                                     residual=x.reshape(B * T, d))
                return y.reshape(x.shape)
            else:               # one quantization, shared by gate and up
                xq = ops.mx_quantize_act(hn, fmt=self.act_format)
                h = ops.swiglu(ops.linear_mx_a8(xq, mg),
                               ops.linear_mx_a8(xq, mu))
        elif mg is not None and T == 1 and self._mx_site(hn, mg, mw_up=mu):
            h = ops.swiglu_linear_decode_mx(hn, mg, mu)
        elif mg is not None and self._mx_fused(hn, mg) \
                and self._mx_fused(hn, mu):
            h = ops.swiglu(ops.linear_mx(hn, mg), ops.linear_mx(hn, mu))
        elif mg is not None:    # one scratch buffer: gate, then up
            g = ops.linear(hn, self._dequantized(mg, hn.dtype))
            h = ops.swiglu(g, ops.linear(hn, self._dequantized(mu, hn.dtype)))
        elif T == 1 and self._skinny_site(hn, blk.w_gate, w_up=blk.w_up):
            h = ops.swiglu_linear_decode(hn, blk.w_gate, blk.w_up)
        else:
            h = ops.swiglu(ops.linear(hn, blk.w_gate),
                           ops.linear(hn, blk.w_up))
        return self._linear(h, blk.w_down, residual=x, decode=T == 1)

    def _llama_qkv(self, x, blk):
        """Packed projection [B*T, (H + 2 Hkv) D] and its q/k/v views."""
        cfg = self.cfg
        B, T, d = x.shape
        H, Hkv = cfg.n_head, self.kv_heads
        D = d // H
        h = ops.rmsnorm(x.reshape(B * T, d), blk.ln1_g, cfg.rms_eps)
        qkv = self._linear(h, blk.w_qkv, decode=T == 1)
        return (qkv[:, :H * D].view(B, T, H, D),
                qkv[:, H * D:(H + Hkv) * D].view(B, T, Hkv, D),
                qkv[:, (H + Hkv) * D:].view(B, T, Hkv, D))

    def _gqa_attend(self, qh, kall, vall, dead):
        """Composed attention of qh [B, H, T, D] (rotated) over cache rows
        kall/vall [B, Hkv, S, D] without expanding them: the G query heads
        of a group are batched into the row dim, [B, Hkv, G*T, D] @ K^T.
        dead: bool mask broadcastable to [T, S], or None."""
        B, H, T, D = qh.shape
        Hkv, S = kall.shape[1], kall.shape[2]
        G = H // Hkv
        q4 = qh.reshape(B, Hkv, G * T, D)
        scores = ops.matmul(q4.contiguous(), kall.transpose(-1, -2)) \
            * (1.0 / math.sqrt(D))
        if dead is not None:
            scores = scores.view(B, Hkv, G, T, S).masked_fill(
                dead, float("-inf")).view(B, Hkv, G * T, S)
        p = torch.softmax(scores.float(), dim=-1).to(vall.dtype)
        return ops.matmul(p, vall.contiguous()).reshape(B, H, T, D)

    def _stack_llama(self, x, kc, vc, pos):
        cfg = self.cfg
        B, T, d = x.shape
        H, Hkv = cfg.n_head, self.kv_heads
        D, G = d // H, H // Hkv
        theta = cfg.rope_theta
        fused = T == 1 and self._fused_decode(x, D, G)
        pf = T > 1 and self._fused_prefill(x, H, Hkv, D)
        att = self._kv8_ops(x, kc, H, Hkv, D)
        if att is not None:        # MXFP8 caches: always the two cache ops
            fused, pf = T == 1, T > 1
        else:
            att = ops
        prefill = T > 1 and pos == 0
        if fused or pf:
            pos_t = torch.full((1,), pos, device=x.device, dtype=torch.long)
        elif not prefill:
            qpos = torch.arange(pos, pos + T, device=x.device)
            dead = None
            if T > 1:  # chunked prefill continuation: causal inside
                kpos = torch.arange(pos + T, device=x.device)
                dead = kpos[None, :] > qpos[:, None]
        for li, blk in enumerate(self.m.blocks):
            q, k, v = self._llama_qkv(x, blk)
            if pf:
                # one op: rope of q and the chunk's K rows at pos + t, cache
                # append, attention over 0..pos + t, K/V read at Hkv heads
                a = att.prefill_attention(q, kc[li], vc[li], pos_t, k_new=k,
                                          v_new=v, rope_theta=theta)
            elif fused:
                # one kernel: rope of q and the new K row at pos, cache
                # append, attention over 0..pos, on views of the projection
                a = att.decode_attention(q[:, 0], kc[li], vc[li], pos_t,
                                         k_new=k[:, 0], v_new=v[:, 0],
                                         rope_theta=theta)
            else:
                if prefill:
                    q = ops.rope(q.reshape(B * T, H, D), T, theta)
                    k = ops.rope(k.reshape(B * T, Hkv, D), T, theta)
                else:
                    q = ref.rope_at(q, qpos[:, None], theta)
                    k = ref.rope_at(k, qpos[:, None], theta)
                qh = q.reshape(B, T, H, D).transpose(1, 2)
                kh = k.reshape(B, T, Hkv, D).transpose(1, 2)
                vh = v.transpose(1, 2)
                kc[li][:, :, pos:pos + T] = kh
                vc[li][:, :, pos:pos + T] = vh
                if prefill:
                    a = ops.attention(
                        qh.contiguous(),
                        kh.repeat_interleave(G, dim=1).contiguous(),
                        vh.repeat_interleave(G, dim=1).contiguous(),
                        causal=True)
                else:
                    a = self._gqa_attend(qh, kc[li][:, :, :pos + T],
                                         vc[li][:, :, :pos + T], dead)
                a = a.transpose(1, 2)
            x = self._linear(a.reshape(B * T, d), blk.w_o, residual=x,
                             decode=T == 1)
            x = self._llama_mlp(x, blk)
        return x

    def _emit(self, x, tok, cur_t, sample):
        """Tail of a static decode step: the next token into tok, cur_t
        advanced. sample None = greedy; else the sample_logits keywords,
        and the token is drawn on the device at the position it is written
        to (cur_t after the increment), straight from the head's output:
        no fp32 copy, no slice, nothing read back."""
        if sample is None:
            logits = self._logits(x).float()[:, -1, :self.cfg.vocab_size]
            tok.copy_(logits.argmax(-1, keepdim=True))
            cur_t.add_(1)
            return
        cur_t.add_(1)
        ops.sample_logits(self._logits(x)[:, -1], vocab=self.cfg.vocab_size,
                          step=cur_t, out=tok, **sample)

    def _decode_step_llama(self, tok, cur_t, kc, vc, kpos, sample=None):
        cfg = self.cfg
        B = tok.shape[0]
        H, Hkv, d = cfg.n_head, self.kv_heads, cfg.n_embd
        D, G = d // H, H // Hkv
        theta = cfg.rope_theta
        x = self._embed(tok, cur_t)
        fused = self._fused_decode(x, D, G)
        att = self._kv8_ops(x, kc, H, Hkv, D)
        if att is not None:
            fused = True
        else:
            att = ops
        if not fused:
            dead = (kpos > cur_t)                   # [S_max] device bool
        for li, blk in enumerate(self.m.blocks):
            q, k, v = self._llama_qkv(x, blk)
            if fused:
                # the kernel reads cur_t on the device: rotates by it,
                # appends at it and attends rows 0..cur_t only
                a = att.decode_attention(q[:, 0], kc[li], vc[li], cur_t,
                                         k_new=k[:, 0], v_new=v[:, 0],
                                         rope_theta=theta)
            else:
                qh = ref.rope_at(q, cur_t, theta).transpose(1, 2)
                kc[li].index_copy_(
                    2, cur_t, ref.rope_at(k, cur_t, theta).transpose(1, 2))
                vc[li].index_copy_(2, cur_t, v.transpose(1, 2))
                a = self._gqa_attend(qh, kc[li], vc[li], dead)
                a = a.transpose(1, 2)
            x = self._linear(a.reshape(B, d), blk.w_o, residual=x,
                             decode=True)
            x = self._llama_mlp(x, blk)
        self._emit(x, tok, cur_t, sample)

    # -- static-shape greedy decode step (hipGraph-capturable) -----------
    #
    # Eager per-token decode is LAUNCH-bound (~1000 kernels/token across
    # 24 layers). This step runs on fixed buffers only: embeds tok at the
    # device-side position cur_t, writes K/V into the cache at cur_t
    # (index_copy_, no host sync), attends over the FULL S_max cache with
    # a kpos > cur_t mask (exp(-inf) = 0 makes it bitwise equal to
    # slicing), argmaxes, feeds the next token back into tok, and
    # advances cur_t — so a captured graph replays autonomously.

    def _decode_step(self, tok, cur_t, kc, vc, kpos, sample=None):
        if self.llama:
            return self._decode_step_llama(tok, cur_t, kc, vc, kpos, sample)
        cfg = self.cfg
        B = tok.shape[0]
        H, d = cfg.n_head, self.m.wte.shape[1]
        D = d // H
        scale = 1.0 / math.sqrt(D)
        x = ops.embedding(tok.reshape(-1), self.m.wte).reshape(B, 1, d) \
            + ops.embedding(cur_t, self.m.wpe)
        fused = self._fused_decode(x, D)
        att = self._kv8_ops(x, kc, H, H, D)
        if att is not None:
            fused = True
        else:
            att = ops
        if not fused:
            mask = (kpos > cur_t)                   # [S_max] device bool
        for li, blk in enumerate(self.m.blocks):
            h = ops.layernorm(x, blk.ln1_g, blk.ln1_b, cfg.ln_eps)
            qkv = self._linear(h, blk.w_qkv, blk.b_qkv, decode=True)
            if fused:
                # the kernel reads cur_t on the device: appends k/v at
                # cur_t and attends rows 0..cur_t only (no S_max sweep)
                q3 = qkv.view(B, 3, H, D)
                a = att.decode_attention(q3[:, 0], kc[li], vc[li], cur_t,
                                         k_new=q3[:, 1],
                                         v_new=q3[:, 2]).reshape(B, 1, d)
            else:
                q, k, v = qkv.split(d, dim=-1)
                qh = q.reshape(B, 1, H, D).transpose(1, 2)
                kc[li].index_copy_(2, cur_t,
                                   k.reshape(B, 1, H, D).transpose(1, 2))
                vc[li].index_copy_(2, cur_t,
                                   v.reshape(B, 1, H, D).transpose(1, 2))
                scores = ops.matmul(qh.contiguous(),
                                    kc[li].transpose(-1, -2)) * scale
                scores = scores.masked_fill(mask, float("-inf"))
                p = torch.softmax(scores.float(), dim=-1).to(x.dtype)
                a = ops.matmul(p, vc[li])
                a = a.transpose(1, 2).reshape(B, 1, d)
            x = self._linear(a, blk.w_proj, blk.b_proj, residual=x,
                             decode=True)
            h = ops.layernorm(x, blk.ln2_g, blk.ln2_b, cfg.ln_eps)
            h = self._linear(h, blk.w_fc, blk.b_fc, act="gelu", decode=True)
            x = self._linear(h, blk.w_out, blk.b_out, residual=x,
                             decode=True)
        self._emit(x, tok, cur_t, sample)

    def _host_token(self, x, temperature, top_k, top_p, gen):
        """Greedy, or the host sampler: filters and softmax where the
        logits live, torch.multinomial on the CPU."""
        logits = self._logits(x).float()[:, -1]       # [B, V]
        logits = logits[:, :self.cfg.vocab_size]       # drop pad rows
        if not temperature > 0:
            return logits.argmax(-1, keepdim=True)
        logits = logits / temperature
        if top_k > 0:
            kth = logits.topk(top_k, dim=-1).values[:, -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        probs = torch.softmax(logits, dim=-1)
        if top_p < 1.0:
            # keep the most probable tokens up to the first whose running
            # mass reaches top_p, its ties included
            sp = probs.sort(dim=-1, descending=True).values
            n = (sp.cumsum(-1) < top_p).sum(-1, keepdim=True)
            thr = sp.gather(-1, n.clamp(max=sp.shape[-1] - 1))
            probs = probs.masked_fill(probs < thr, 0.0)
        return torch.multinomial(probs.cpu(), 1,
                                 generator=gen).to(logits.device)

    @torch.no_grad()
    def generate(self, ids: torch.Tensor, max_new_tokens: int,
                 temperature: float = 0.0, top_k: int = 0,
                 seed: int = 0, top_p: float = 1.0,
                 sampler: Optional[str] = None,
                 prefill_chunk: Optional[int] = None) -> torch.Tensor:
        """prefill_chunk: feed the prompt through the stack in chunks of
        that many tokens (None = one chunk). top_p: nucleus sampling on what top-k left (1.0 = off). sampler
        (else TEPDIST_SAMPLER, else "host") says where temperature > 0
        draws: "host" = softmax on the device, torch.multinomial on the
        CPU from torch.Generator(seed), one [B, V] copy and one sync per
        token; "device" = ops.sample_logits, drawn from Philox(seed, row,
        position), which on the GPU keeps sampling inside the captured
        decode graph like greedy; "auto" = device on the GPU for fp32/bf16
        models, host otherwise. The two samplers draw different (equally
        valid) tokens for the same seed, so the default stays "host"."""
        cfg = self.cfg
        if sampler is None:
            sampler = os.environ.get("TEPDIST_SAMPLER", "host")
        if sampler not in ("host", "device", "auto"):
            raise ValueError(
                f"sampler must be 'host', 'device' or 'auto', "
                f"got {sampler!r}")
        B, S0 = ids.shape
        H, d = cfg.n_head, cfg.n_embd
        D = d // H
        S_max = min(self.max_seq, S0 + max_new_tokens)
        dev = next(self.m.parameters()).device
        dt = next(self.m.parameters()).dtype
        kc, vc = self.new_caches(B, S_max, dev, dt)
        if sampler == "auto":
            sampler = "device" if ids.is_cuda and dt in (
                torch.float32, torch.bfloat16) else "host"
        # sample_logits keywords when tokens are drawn on the device
        sample = None
        if temperature > 0 and sampler == "device":
            sample = dict(temperature=temperature, top_k=top_k, top_p=top_p,
                          seed=seed)
        else:
            gen = torch.Generator(device="cpu").manual_seed(seed)

        out = ids
        pos_ids = torch.arange(S0, device=dev)
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be >= 1, "
                             f"got {prefill_chunk!r}")
        if prefill_chunk is None or prefill_chunk >= S0:
            x = self._embed(ids, pos_ids)
            x = self._stack(x, kc, vc, 0)
        else:
            for c0 in range(0, S0, prefill_chunk):
                c1 = min(c0 + prefill_chunk, S0)
                x = self._embed(ids[:, c0:c1], pos_ids[c0:c1])
                x = self._stack(x, kc, vc, c0)
        cur = S0

        # greedy or device-sampled decode on GPU: static-buffer steps,
        # hipGraph-captured after two eager warmups (the eager per-token
        # loop is launch-bound; replaying one recorded step removes ~1000
        # launches/token). TEPDIST_DECODE_GRAPH=0 forces eager.
        if ((temperature == 0 or sample is not None) and ids.is_cuda
                and S_max > S0
                and max_new_tokens >= 8
                and os.environ.get("TEPDIST_DECODE_GRAPH", "1") != "0"):
            cur_t = torch.full((1,), S0, device=dev, dtype=torch.long)
            if sample is None:
                logits = self._logits(x).float()[:, -1, :cfg.vocab_size]
                tok = logits.argmax(-1, keepdim=True)
            else:
                tok = ops.sample_logits(self._logits(x)[:, -1],
                                        vocab=cfg.vocab_size, step=cur_t,
                                        **sample)
            outs = [tok.clone()]
            kpos = torch.arange(S_max, device=dev)
            n_rest = min(max_new_tokens, S_max - S0) - 1
            graph = None
            done = 0
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(min(2, n_rest)):
                        self._decode_step(tok, cur_t, kc, vc, kpos, sample)
                        outs.append(tok.clone())
                        done += 1
                torch.cuda.current_stream().wait_stream(side)
                if done < n_rest:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._decode_step(tok, cur_t, kc, vc, kpos, sample)
            except Exception:
                graph = None           # capture failed: stay eager
            while done < n_rest:
                if graph is not None:
                    graph.replay()
                else:
                    self._decode_step(tok, cur_t, kc, vc, kpos, sample)
                outs.append(tok.clone())
                done += 1
            return torch.cat([ids] + outs, dim=1)
        for _ in range(max_new_tokens):
            if cur >= S_max:
                break
            pos = torch.full((1,), cur, device=dev, dtype=torch.long)
            if sample is not None:
                # drawn where the logits live, at the position written to
                nxt = ops.sample_logits(self._logits(x)[:, -1],
                                        vocab=cfg.vocab_size, step=pos,
                                        **sample)
            else:
                nxt = self._host_token(x, temperature, top_k, top_p, gen)
            out = torch.cat([out, nxt], dim=1)
            x = self._embed(nxt, pos)
            x = self._stack(x, kc, vc, cur)
            cur += 1
        return out
