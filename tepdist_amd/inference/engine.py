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
(docs/KERNELS.md "Sampling")."""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

from tepdist_amd import ops
from tepdist_amd.models.llama import Llama
from tepdist_amd.ops import reference as ref

# query-group sizes H / Hkv the fused decode kernel covers
FUSED_GROUPS = (1, 2, 4, 8)


class Generator:
    def __init__(self, model, max_seq: Optional[int] = None,
                 decode_attn: Optional[str] = None):
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
        if fused:
            pos_t = torch.full((1,), pos, device=x.device, dtype=torch.long)
        for li, blk in enumerate(self.m.blocks):
            h = ops.layernorm(x, blk.ln1_g, blk.ln1_b, cfg.ln_eps)
            qkv = ops.linear(h, blk.w_qkv, blk.b_qkv)      # [B,T,3d]
            if fused:
                # one kernel: cache append at pos + attention over 0..pos,
                # reading q/k/v as views of the packed projection
                q3 = qkv.view(B, 3, H, D)
                a = ops.decode_attention(q3[:, 0], kc[li], vc[li], pos_t,
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
            x = x + ops.linear(a, blk.w_proj, blk.b_proj)
            h = ops.layernorm(x, blk.ln2_g, blk.ln2_b, cfg.ln_eps)
            h = ops.linear(h, blk.w_fc, blk.b_fc, act="gelu")
            x = x + ops.linear(h, blk.w_out, blk.b_out)
        return x

    def _logits(self, x):
        if self.llama:
            h = ops.rmsnorm(x[:, -1], self.m.ln_f_g, self.cfg.rms_eps)
            return ops.linear(h, self.m.lm_head)[:, None]   # untied head
        x = ops.layernorm(x, self.m.lnf_g, self.m.lnf_b, self.cfg.ln_eps)
        return ops.linear(x[:, -1:], self.m.wte)   # last position only

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
        h = ops.swiglu(ops.linear(hn, blk.w_gate), ops.linear(hn, blk.w_up))
        return x + ops.linear(h, blk.w_down).reshape(B, T, d)

    def _llama_qkv(self, x, blk):
        """Packed projection [B*T, (H + 2 Hkv) D] and its q/k/v views."""
        cfg = self.cfg
        B, T, d = x.shape
        H, Hkv = cfg.n_head, self.kv_heads
        D = d // H
        h = ops.rmsnorm(x.reshape(B * T, d), blk.ln1_g, cfg.rms_eps)
        qkv = ops.linear(h, blk.w_qkv)
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
        prefill = T > 1 and pos == 0
        if fused:
            pos_t = torch.full((1,), pos, device=x.device, dtype=torch.long)
        elif not prefill:
            qpos = torch.arange(pos, pos + T, device=x.device)
            dead = None
            if T > 1:  # chunked prefill continuation: causal inside
                kpos = torch.arange(pos + T, device=x.device)
                dead = kpos[None, :] > qpos[:, None]
        for li, blk in enumerate(self.m.blocks):
            q, k, v = self._llama_qkv(x, blk)
            if fused:
                # one kernel: rope of q and the new K row at pos, cache
                # append, attention over 0..pos, on views of the projection
                a = ops.decode_attention(q[:, 0], kc[li], vc[li], pos_t,
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
            x = x + ops.linear(a.reshape(B * T, d), blk.w_o).reshape(B, T, d)
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
        if not fused:
            dead = (kpos > cur_t)                   # [S_max] device bool
        for li, blk in enumerate(self.m.blocks):
            q, k, v = self._llama_qkv(x, blk)
            if fused:
                # the kernel reads cur_t on the device: rotates by it,
                # appends at it and attends rows 0..cur_t only
                a = ops.decode_attention(q[:, 0], kc[li], vc[li], cur_t,
                                         k_new=k[:, 0], v_new=v[:, 0],
                                         rope_theta=theta)
            else:
                qh = ref.rope_at(q, cur_t, theta).transpose(1, 2)
                kc[li].index_copy_(
                    2, cur_t, ref.rope_at(k, cur_t, theta).transpose(1, 2))
                vc[li].index_copy_(2, cur_t, v.transpose(1, 2))
                a = self._gqa_attend(qh, kc[li], vc[li], dead)
                a = a.transpose(1, 2)
            x = x + ops.linear(a.reshape(B, d), blk.w_o).reshape(B, 1, d)
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
        if not fused:
            mask = (kpos > cur_t)                   # [S_max] device bool
        for li, blk in enumerate(self.m.blocks):
            h = ops.layernorm(x, blk.ln1_g, blk.ln1_b, cfg.ln_eps)
            qkv = ops.linear(h, blk.w_qkv, blk.b_qkv)
            if fused:
                # the kernel reads cur_t on the device: appends k/v at
                # cur_t and attends rows 0..cur_t only (no S_max sweep)
                q3 = qkv.view(B, 3, H, D)
                a = ops.decode_attention(q3[:, 0], kc[li], vc[li], cur_t,
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
            x = x + ops.linear(a, blk.w_proj, blk.b_proj)
            h = ops.layernorm(x, blk.ln2_g, blk.ln2_b, cfg.ln_eps)
            h = ops.linear(h, blk.w_fc, blk.b_fc, act="gelu")
            x = x + ops.linear(h, blk.w_out, blk.b_out)
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
                 sampler: Optional[str] = None) -> torch.Tensor:
        """top_p: nucleus sampling on what top-k left (1.0 = off). sampler
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
        kc = [torch.zeros(B, self.kv_heads, S_max, D, dtype=dt, device=dev)
              for _ in range(cfg.n_layer)]
        vc = [torch.zeros(B, self.kv_heads, S_max, D, dtype=dt, device=dev)
              for _ in range(cfg.n_layer)]
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
        x = self._embed(ids, pos_ids)
        x = self._stack(x, kc, vc, 0)
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
