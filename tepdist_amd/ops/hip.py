"""GPU backend: wraps the hand-written gfx950 kernels (_tepdist_hip.so) with
the same function signatures as tepdist_amd/ops/reference.py.

This module import FAILS LOUDLY if the extension is missing — on a GPU
machine there is no silent eager fallback (the HIP path must be the one that
runs; see repo policy / driver's native-code check).
"""

from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

try:
    from tepdist_amd.ops import _tepdist_hip as ext
except ImportError as e:  # pragma: no cover
    raise ImportError(
        "tepdist_amd HIP extension not built. Run "
        "`python tepdist_amd/ops/build_ext.py` (hipcc cross-compiles on a "
        "GPU-less box). No eager fallback is provided on GPU.") from e

BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _layout2d(t: torch.Tensor, kc_expected_inner: bool):
    """Given a 2-D (or batched view flattened) operand, return (kc, ld).
    kc=True means the contraction dim is the fastest-varying (stride 1)."""
    assert t.dim() == 2
    if t.stride(1) == 1:
        return True, t.stride(0)
    if t.stride(0) == 1:
        return False, t.stride(1)
    raise ValueError(f"operand must be contiguous in one dim, strides={t.stride()}")


# --------------------------------------------------------------------------
# GEMM family
# --------------------------------------------------------------------------
#
# Backend policy ("measure, don't guess" made literal): the hand-written
# 256x256 MFMA pipeline owns FUSED GEMMs (bias / bias+gelu dual-output
# epilogues) where a library call would pay an extra full pass over C;
# hipBLASLt (torch.matmul/F.linear on ROCm) is the right tool for PLAIN
# GEMMs — measured on the flagship shapes (benchmarks/shapes65k.py,
# profiles/shapes65k_*.json) it runs them 1.2-1.4x our pipeline AND
# consumes transposed operand layouts natively, which removes the
# dgrad/wgrad canonicalization transposes (9.6% of the r1 step) outright.
# Mode "auto" times both paths once per (site, shape) at first use and
# caches the winner; TEPDIST_GEMM_BACKEND=hip|blaslt pins a backend
# (kill-switch + pure-hand-kernel demonstration mode).

_GEMM_BACKEND = os.environ.get("TEPDIST_GEMM_BACKEND", "auto")
_gemm_choice = {}


def _pick_backend(key, hip_fn, blt_fn):
    """Returns the cached winner for `key`, timing both once if unseen."""
    if _GEMM_BACKEND == "hip":
        return hip_fn
    if _GEMM_BACKEND == "blaslt":
        return blt_fn
    got = _gemm_choice.get(key)
    if got is not None:
        return hip_fn if got == "hip" else blt_fn
    if torch.cuda.is_current_stream_capturing():
        return hip_fn  # never tune inside a hipGraph capture
    import time as _time

    def _t(fn):
        fn()
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(3):          # best-of-3 x 2 iters: noise-robust
            t0 = _time.perf_counter()
            fn()
            fn()
            torch.cuda.synchronize()
            best = min(best, _time.perf_counter() - t0)
        return best

    th, tb = _t(hip_fn), _t(blt_fn)
    _gemm_choice[key] = "hip" if th <= tb else "blaslt"
    return hip_fn if th <= tb else blt_fn


def _gemm_raw(a: torch.Tensor, b_stored: torch.Tensor, a_kc: bool, b_kc: bool,
              M: int, N: int, K: int, lda: int, ldb: int,
              sa: int, sb: int, batch: int, bias=None, epi: int = 0,
              out=None, out_pre=None, device=None, colsum_out=None):
    """colsum_out (bf16 [M]): also receives the column sums of a k-outer A
    (A stored [K][M]), where the plan gives the 256 kernel; ext.gemm throws
    elsewhere."""
    dev = device if device is not None else a.device
    c = out if out is not None else torch.empty(
        (batch, M, N) if batch > 1 else (M, N), dtype=BF16, device=dev)
    cp = out_pre
    if epi >= 2 and cp is None:
        cp = torch.empty_like(c)

    # kernel choice and split-K are planned in csrc/gemm_plan.h, which also
    # sizes the fp32 room for a split plan's partials and for column-sum
    # parts (ext.gemm reduces both; none of it needs zeroing)
    ws_floats = ext.gemm_ws_floats(M, N, K, lda, ldb, a_kc, b_kc, epi, batch,
                                   colsum_out is not None)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev) \
        if ws_floats else None
    ext.gemm(a.data_ptr(), b_stored.data_ptr(), c.data_ptr(), _p(cp), _p(bias),
             M, N, K, lda, ldb, N, sa, sb, M * N, batch, a_kc, b_kc, epi,
             _p(ws), _stream(), _p(colsum_out))
    return c, cp


def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
               act: str = "none") -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    assert x.dtype == BF16 and w.dtype == BF16, "hip backend is bf16-only"
    x = x.contiguous()
    M, K = x.shape
    N = w.shape[0]
    if act == "none":
        epi = 1 if bias is not None else 0
    elif act == "gelu":
        epi = 2 if bias is not None else 3
    else:
        raise ValueError(act)

    def _hip():
        return _gemm_raw(x, w, True, True, M, N, K, K, w.stride(0), 0, 0, 1,
                         bias=bias, epi=epi)

    def _blt():
        # hipBLASLt GEMM (+fused bias via addmm); gelu applies through our
        # elementwise kernel so fwd/bwd use the same tanh approximation
        pre = torch.nn.functional.linear(x, w, bias)
        if act != "gelu":
            return pre, None
        y = torch.empty_like(pre)
        ext.gelu_fwd(pre.data_ptr(), y.data_ptr(), pre.numel(), _stream())
        return y, pre

    fn = _pick_backend(("lin_f", M, N, K, epi), _hip, _blt)
    return fn()


def _bias_sum(t: torch.Tensor) -> torch.Tensor:
    """Column sums of contiguous t [rows, cols] as bf16 [cols] (the bias
    gradient), accumulated in a zeroed fp32 workspace."""
    rows, cols = t.shape
    db = torch.empty(cols, dtype=BF16, device=t.device)
    ws = torch.zeros(cols, dtype=torch.float32, device=t.device)
    ext.bias_sum(t.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, cols,
                 _stream())
    return db


def gelu_fwd(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    y = torch.empty_like(x)
    ext.gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream())
    return y


def gelu_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(dy)
    ext.gelu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), dy.numel(),
                 _stream())
    return dx


# --------------------------------------------------------------------------
# Fused transformer MLP (hipBLASLt fused epilogues)
# --------------------------------------------------------------------------
#
# The gelu between the two MLP GEMMs costs two full HBM round-trips as
# standalone kernels (read+write of the [T, 4d] tensor fwd AND bwd). The
# hipBLASLt epilogues fold them into the producing GEMMs: GELU_AUX_BIAS on
# the c_fc forward (pre-gelu saved as the aux buffer the backward needs
# anyway) and DGELU_BGRAD on the proj dgrad (gelu' applied to the GEMM
# result + the fc bias gradient reduced in the same pass). Fused vs
# composed is measured per shape at first use like every other GEMM site;
# TEPDIST_MLP_FUSED=0|1 pins.

try:
    from tepdist_amd.ops import _tepdist_blt as _blt
except Exception:                      # extension not built
    _blt = None

_MLP_FUSED = os.environ.get("TEPDIST_MLP_FUSED", "auto")


def _blt_mlp_gelu(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    M, K = x.shape
    N = w1.shape[0]
    y = torch.empty(M, N, dtype=BF16, device=x.device)
    aux = torch.empty(M, N, dtype=BF16, device=x.device)
    _blt.blt_fused(0, M, N, K, w1.data_ptr(), x.data_ptr(), y.data_ptr(),
                   b1.data_ptr(), aux.data_ptr(), _stream())
    return y, aux


def _blt_mlp_dgelu(dy: torch.Tensor, w2: torch.Tensor, pre: torch.Tensor):
    M, N = dy.shape
    K = w2.shape[1]
    dh = torch.empty(M, K, dtype=BF16, device=dy.device)
    db1 = torch.empty(K, dtype=BF16, device=dy.device)
    _blt.blt_fused(1, M, N, K, w2.data_ptr(), dy.data_ptr(), dh.data_ptr(),
                   db1.data_ptr(), pre.data_ptr(), _stream())
    return dh, db1


_blt_ok = True    # flipped off permanently on the first library refusal
                  # (e.g. "no algo for fused epilogue" on this shape set)


def _blt_usable() -> bool:
    return _blt is not None and _blt_ok and _MLP_FUSED != "0"


def mlp_fwd(x, w1, b1, w2, b2):
    """y = gelu(x@w1^T+b1) @ w2^T + b2. Returns (y, (h, pre)): the
    post-gelu activation and the pre-gelu aux for backward."""
    global _blt_ok
    x = x.contiguous()
    res = {}

    def _fused():
        h, pre = _blt_mlp_gelu(x, w1, b1)
        res["h"], res["pre"] = h, pre
        return linear_fwd(h, w2, b2, "none")[0]

    def _composed():
        h, pre = linear_fwd(x, w1, b1, "gelu")
        res["h"], res["pre"] = h, pre
        return linear_fwd(h, w2, b2, "none")[0]

    if not _blt_usable():
        y = _composed()
    elif _MLP_FUSED == "1":
        y = _fused()
    else:
        try:
            y = _pick_backend(("mlp_f", x.shape[0], w1.shape[0],
                               x.shape[1]), _fused, _composed)()
        except RuntimeError:
            _blt_ok = False
            y = _composed()
    return y, (res["h"], res["pre"])


def mlp_bwd(dy, x, w1, w2, h, pre):
    """Backward of mlp_fwd. Returns (dx, dw1, db1, dw2, db2)."""
    global _blt_ok
    dy = dy.contiguous()
    out = {}

    def _fused():
        # proj dgrad with the DGELU_BGRAD epilogue: one library call
        # yields dgelu'd dh AND the fc bias grad
        dh, db1 = _blt_mlp_dgelu(dy, w2, pre)
        dw2, db2 = wgrad(dy, h, True)
        dx, dw1, _ = linear_bwd(dh, x, w1, False, "none", None)
        out["r"] = (dx, dw1, db1, dw2, db2)

    def _composed():
        # exactly the unfused two-linear backward: per-shape autotuned,
        # the hand path keeps its fused gelu'-in-transpose wgrad trick
        dh_post, dw2, db2 = linear_bwd(dy, h, w2, True, "none", None)
        dx, dw1, db1 = linear_bwd(dh_post, x, w1, True, "gelu", pre)
        out["r"] = (dx, dw1, db1, dw2, db2)

    def _hand_dgelu():
        # the fusion the library cannot express on this stack: proj dgrad
        # on the 256 schedule with a dgelu epilogue reading the saved
        # pre-activation — dh = (dy @ w2) * gelu'(pre) in ONE kernel, the
        # standalone gelu_bwd pass disappears
        M, N2 = dy.shape
        K2 = w2.shape[1]
        w2T = transpose2d(w2)                       # [4d, d] KC
        dh, _ = _gemm_raw(dy, w2T, True, True, M, K2, N2, N2, N2, 0, 0, 1,
                          epi=4, out_pre=pre)
        dw2, db2 = wgrad(dy, h, True)
        # db1 = column sums of dh: from the in-place wgrad's fragments where
        # linear_bwd takes that branch, its streaming _bias_sum elsewhere
        dx, dw1, db1 = linear_bwd(dh, x, w1, True, "none", None)
        out["r"] = (dx, dw1, db1, dw2, db2)

    def _base():
        # hand-dgelu vs composed, measured per shape (only where the plan
        # gives the dgelu epilogue, epi 4, a kernel; TEPDIST_GEMM_BACKEND
        # pins propagate through _pick_backend)
        M, N2 = dy.shape
        K2 = w2.shape[1]
        if (ext.gemm_plan(M, K2, N2, N2, N2, True, True, 4, 1)[0] == 256
                and pre.is_contiguous()):
            _pick_backend(("mlp_bh", dy.shape[0], dy.shape[1],
                           w2.shape[1]), _hand_dgelu, _composed)()
        else:
            _composed()

    if not _blt_usable():
        _base()
    elif _MLP_FUSED == "1":
        _fused()
    else:
        try:
            _pick_backend(("mlp_b", dy.shape[0], dy.shape[1],
                           w2.shape[1]), _fused, _base)()
        except RuntimeError:
            _blt_ok = False
            _base()
    return out["r"]


def transpose2d(t: torch.Tensor) -> torch.Tensor:
    """Materialized bf16 transpose (tiled LDS kernel)."""
    R, C = t.shape[-2], t.shape[-1]
    batch = t.numel() // (R * C)
    t = t.contiguous()
    out = torch.empty((*t.shape[:-2], C, R), dtype=t.dtype, device=t.device)
    ext.transpose(t.data_ptr(), out.data_ptr(), R, C, R * C, R * C, batch,
                  _stream())
    return out


def _wgrad_in_place(dyl: torch.Tensor, x: torch.Tensor) -> bool:
    """Whether the plan gives wgrad of dyl [M,N] and x [M,K], two k-outer
    operands, the 256 kernel that reads them as they lie."""
    (M, N), K = dyl.shape, x.shape[1]
    return dyl.stride(-1) == 1 and x.stride(-1) == 1 and ext.gemm_plan(
        N, K, M, dyl.stride(0), x.stride(0), False, False, 0, 1)[0] == 256


def wgrad(dyl: torch.Tensor, x: torch.Tensor, has_bias: bool):
    """(dw, db) = (dyl^T @ x, column sums of dyl or None). Where the 256
    kernel reads both operands in place its column-sum variant forms db from
    the dy fragments it holds anyway: one hand call, no second pass over
    dyl, no atomics. Measured per shape against the library GEMM plus the
    streaming bias sum, bias and bias-less sites apart."""
    M, N = dyl.shape
    K = x.shape[1]
    def _db():  # the streaming pass wants whole rows
        return _bias_sum(dyl.contiguous()) if has_bias else None

    if not _wgrad_in_place(dyl, x):
        return matmul(dyl.t(), x), _db()

    def _hand():
        db = torch.empty(N, dtype=BF16, device=dyl.device) \
            if has_bias else None
        dw = _gemm_raw(dyl, x, False, False, N, K, M, dyl.stride(0),
                       x.stride(0), 0, 0, 1, colsum_out=db)[0]
        return dw, db

    def _lib():
        return torch.matmul(dyl.t(), x), _db()

    return _pick_backend(("lin_bw", M, N, K, has_bias), _hand, _lib)()


def linear_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
               has_bias: bool, act: str, pre_act: Optional[torch.Tensor]):
    dy = dy.contiguous()
    M, N = dy.shape
    K = w.shape[1]

    # wgrad dW[N,K] = dy^T[N,M] @ x[M,K] has both operands k-outer (the
    # contraction index M is the slow dimension of dy and of x). Where the
    # plan gives such a call the 256 kernel, it reads dy and x in place: no
    # activation transpose, and dgrad and wgrad each take the backend that
    # measured faster for them (inside a graph capture both stay hand).
    if _wgrad_in_place(dy, x):
        if act == "gelu":
            dyl = torch.empty_like(dy)
            ext.gelu_bwd(dy.data_ptr(), pre_act.data_ptr(), dyl.data_ptr(),
                         dy.numel(), _stream())
        else:
            dyl = dy

        def _dx_hip():
            wT = transpose2d(w)    # [K, N]: the weight, a few microseconds
            return _gemm_raw(dyl, wT, True, True, M, K, N, N, N, 0, 0, 1)[0]

        dx = _pick_backend(("lin_bx", M, N, K), _dx_hip,
                           lambda: torch.matmul(dyl, w))()
        dw, db = wgrad(dyl, x, has_bias)
        return dx, dw, db

    def _hip():
        # canonicalize to KC x KC: one tuned GEMM schedule serves every
        # case, with materialized transposes.
        dyl = dy
        wT = transpose2d(w)        # [K, N]
        # fused gelu-backward: the wgrad transpose of dy applies gelu'(pre)
        # in the same pass and emits BOTH layouts (saves the separate
        # elementwise kernel's full read+write). Bias sums stay a separate
        # streaming pass — folding them into the transpose as LDS atomics
        # measured ~3x slower transposes (per-element atomic serialization).
        dyT = torch.empty(N, M, dtype=BF16, device=dy.device)
        if act == "gelu":
            dy_eff = torch.empty_like(dyl)
            ext.transpose_dy(dyl.data_ptr(), pre_act.data_ptr(),
                             dyT.data_ptr(), dy_eff.data_ptr(), 0, M, N,
                             _stream())
            dyl = dy_eff
        else:
            ext.transpose_dy(dyl.data_ptr(), 0, dyT.data_ptr(), 0, 0, M, N,
                             _stream())
        xT = transpose2d(x)        # [K, M]
        # dx[M,K] = dy[M,N] @ w[N,K]: A=dy KC (k=N), B=w^T stored [K,N] KC
        dx, _ = _gemm_raw(dyl, wT, True, True, M, K, N, N, N, 0, 0, 1)
        # dw[N,K] = dy^T[N,M] @ x[M,K]: A=dy^T KC (k=M), B=x^T [K,M] KC
        dw, _ = _gemm_raw(dyT, xT, True, True, N, K, M, M, M, 0, 0, 1)
        return dx, dw, dyl

    def _blt():
        # hipBLASLt consumes the natural layouts (NN dgrad, TN wgrad):
        # no transposes at all
        if act == "gelu":
            dyl = torch.empty_like(dy)
            ext.gelu_bwd(dy.data_ptr(), pre_act.data_ptr(), dyl.data_ptr(),
                         dy.numel(), _stream())
        else:
            dyl = dy
        dx = torch.matmul(dyl, w)        # [M,N] @ [N,K]
        dw = torch.matmul(dyl.t(), x)    # [N,M] @ [M,K]
        return dx, dw, dyl

    fn = _pick_backend(("lin_b", M, N, K, act), _hip, _blt)
    dx, dw, dy_eff = fn()
    db = None
    if has_bias:
        db = _bias_sum(dy_eff)
    return dx, dw, db


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """C = A @ B with fp32 accumulation (plain GEMM: measured backend
    choice between the MFMA pipeline and hipBLASLt per shape/layout)."""
    key = ("mm", tuple(a.shape), tuple(b.shape),
           a.stride(-1) == 1, b.stride(-1) == 1)
    return _pick_backend(key, lambda: _matmul_hip(a, b),
                         lambda: torch.matmul(a, b))()


def _matmul_hip(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Hand MFMA path: accepts transposed views of the last two dims
    without materializing (mapped to kernel layout flags).
    Shapes: [M,K]@[K,N] or batched [B,M,K]@[B,K,N] (B may broadcast)."""
    assert a.dtype == BF16 and b.dtype == BF16
    squeeze = a.dim() == 2 and b.dim() == 2
    lead_shape = (a if a.dim() >= b.dim() else b).shape[:-2]
    if a.dim() == 2:
        a = a.unsqueeze(0)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    # flatten leading batch dims (transposed views of the last two dims keep
    # a flattenable layout since the batch dims stay contiguous)
    if a.dim() > 3:
        a = a.reshape(-1, *a.shape[-2:]) if a.stride(-1) == 1 else \
            a.transpose(-1, -2).reshape(-1, a.shape[-1], a.shape[-2]).transpose(-1, -2)
    if b.dim() > 3:
        b = b.reshape(-1, *b.shape[-2:]) if b.stride(-1) == 1 else \
            b.transpose(-1, -2).reshape(-1, b.shape[-1], b.shape[-2]).transpose(-1, -2)
    M, K = a.shape[-2], a.shape[-1]
    K2, N = b.shape[-2], b.shape[-1]
    assert K == K2, (a.shape, b.shape)
    batch = max(a.shape[0], b.shape[0])

    def layout(t, contraction_is_last: bool):
        # returns (kc, ld, batch_stride)
        if t.stride(-1) == 1:
            inner_last = True
            ld = t.stride(-2)
        elif t.stride(-2) == 1:
            inner_last = False
            ld = t.stride(-1)
        else:
            t = t.contiguous()
            inner_last = True
            ld = t.stride(-2)
        kc = (inner_last == contraction_is_last)
        bs = t.stride(0) if t.shape[0] > 1 else 0
        return t, kc, ld, bs

    a, a_kc, lda, sa = layout(a, contraction_is_last=True)
    b, b_kc, ldb, sb = layout(b, contraction_is_last=False)
    # canonicalize big single GEMMs to KC x KC (unlocks the 256x256
    # deep-pipelined kernel; the transpose is memory-bound and cheap)
    if batch == 1 and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 \
            and K >= 512 and not (
                # two k-outer operands run on the 256 kernel as they lie
                not a_kc and not b_kc and ext.gemm_plan(
                    M, N, K, lda, ldb, False, False, 0, 1)[0] == 256):
        if not a_kc:
            a = transpose2d(a.reshape(K, M)).reshape(1, M, K)
            a_kc, lda = True, K
        if not b_kc:
            b = transpose2d(b.reshape(K, N)).reshape(1, N, K)
            b_kc, ldb = True, K
    # b layout: contraction dim is -2; b_kc means the contraction dim has the
    # larger stride... map: for B operand the kernel's b_kc=True expects
    # storage [N,K] (k inner). b's contraction dim is -2; if b.stride(-1)==1
    # (inner is N) then storage is [K,N] => b_kc=False.
    c, _ = _gemm_raw(a, b, a_kc, b_kc, M, N, K, lda, ldb, sa, sb, batch,
                     device=a.device)
    if squeeze:
        return c.reshape(M, N)
    return c.reshape(*lead_shape, M, N)


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------

LN_PART_ROWS = 1024  # 256 blocks * 4 waves


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                  eps: float = 1e-5):
    x = x.contiguous()
    rows, cols = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    ext.layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                      y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows,
                      cols, eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor,
                  mean: torch.Tensor, rstd: torch.Tensor):
    dy = dy.contiguous()
    rows, cols = x.shape
    part = min(LN_PART_ROWS, max(4, (rows + 3) // 4 * 4))
    part = (part // 4) * 4
    dx = torch.empty_like(x)
    dg_part = torch.empty(part, cols, dtype=torch.float32, device=x.device)
    db_part = torch.empty(part, cols, dtype=torch.float32, device=x.device)
    dgamma = torch.empty_like(gamma)
    dbeta = torch.empty_like(gamma)
    ext.layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(),
                      mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                      dg_part.data_ptr(), db_part.data_ptr(),
                      dgamma.data_ptr(), dbeta.data_ptr(), rows, cols, part,
                      _stream())
    return dx, dgamma, dbeta


def add_layernorm_fwd(x, res, gamma, beta, eps: float = 1e-5):
    """Fused residual add + layernorm: s = x + res (bf16-rounded once),
    y = ln(s). The standalone add kernel's write+read of `s` disappears.
    Returns (s, y, mean, rstd)."""
    x, res = x.contiguous(), res.contiguous()
    rows, cols = x.shape
    s = torch.empty_like(x)
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    ext.layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                      y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows,
                      cols, eps, _stream(), res.data_ptr(), s.data_ptr())
    return s, y, mean, rstd


def add_layernorm_bwd(dy, dsum, s, gamma, mean, rstd):
    """Backward of add_layernorm: dx = dsum + d(ln)/ds in one pass
    (the autograd grad-accumulation add disappears). dsum may be None
    (sum unused elsewhere). Returns (dx, dgamma, dbeta); dres == dx."""
    dy = dy.contiguous()
    dsum = dsum.contiguous() if dsum is not None else None
    rows, cols = s.shape
    part = min(LN_PART_ROWS, max(4, (rows + 3) // 4 * 4))
    part = (part // 4) * 4
    dx = torch.empty_like(s)
    dg_part = torch.empty(part, cols, dtype=torch.float32, device=s.device)
    db_part = torch.empty(part, cols, dtype=torch.float32, device=s.device)
    dgamma = torch.empty_like(gamma)
    dbeta = torch.empty_like(gamma)
    ext.layernorm_bwd(dy.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                      mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                      dg_part.data_ptr(), db_part.data_ptr(),
                      dgamma.data_ptr(), dbeta.data_ptr(), rows, cols, part,
                      _stream(),
                      0 if dsum is None else dsum.data_ptr())
    return dx, dgamma, dbeta


# --------------------------------------------------------------------------
# Softmax / attention
# --------------------------------------------------------------------------

def softmax_fwd(scores: torch.Tensor, scale: float = 1.0,
                causal: bool = False) -> torch.Tensor:
    scores = scores.contiguous()
    sq, sk = scores.shape[-2], scores.shape[-1]
    if causal and sq > sk:
        # query q sees keys <= q + (sk - sq): the first sq - sk queries
        # would see no key at all (an empty softmax, NaN in the kernel)
        raise ValueError(f"causal softmax needs sq <= sk, got sq={sq} "
                         f"sk={sk}")
    rows = scores.numel() // sk
    p = torch.empty_like(scores)
    ext.softmax_fwd(scores.data_ptr(), p.data_ptr(), rows, sk, sq, scale,
                    causal, _stream())
    return p


def softmax_bwd(dp: torch.Tensor, p: torch.Tensor,
                scale: float = 1.0) -> torch.Tensor:
    dp = dp.contiguous()
    sk = p.shape[-1]
    rows = p.numel() // sk
    ds = torch.empty_like(p)
    ext.softmax_bwd(dp.data_ptr(), p.data_ptr(), ds.data_ptr(), rows, sk,
                    scale, _stream())
    return ds


_ATTN_IMPL = os.environ.get("TEPDIST_ATTN", "flash")


def _check_attention_operands(name: str, q: torch.Tensor, **others):
    """The flash launch takes B, H, S, D from q alone and reads every
    operand as bf16 of that shape: anything else would be misread (a
    shorter k out of bounds), so it is refused before any launch."""
    if q.dim() != 4:
        raise ValueError(f"{name}: q must be [B, H, S, D], got "
                         f"{tuple(q.shape)}")
    for what, t in (("q", q),) + tuple(others.items()):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{name}: {what} is {t.dtype}, the flash "
                             "kernels are bf16-only")
        if t.shape != q.shape:
            raise ValueError(f"{name}: {what} is {tuple(t.shape)}, q is "
                             f"{tuple(q.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name}: {what} is on {t.device}, q on "
                             f"{q.device}")


def _check_lse(name: str, lse: torch.Tensor, bh: int, S: int):
    if lse.dtype != torch.float32 or lse.numel() != bh * S:
        raise ValueError(f"{name}: lse must be fp32 with {bh} x {S} "
                         f"elements, got {lse.dtype} {tuple(lse.shape)}")
    return lse.contiguous()


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  causal: bool = True):
    """Fused flash attention (no S x S matrix in HBM); saves (out, lse)
    for the fused backward. Falls back to the composed GEMM+softmax path
    for head dims other than 64/128 or TEPDIST_ATTN=composed."""
    B, H, S, D = q.shape
    scale = 1.0 / math.sqrt(D)
    if _ATTN_IMPL == "composed" or D not in (64, 128):
        scores = matmul(q, k.transpose(-1, -2))
        p = softmax_fwd(scores, scale=scale, causal=causal)
        out = matmul(p, v)
        return out, (p,)
    _check_attention_operands("attention_fwd", q, k=k, v=v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty_like(q)
    lse = torch.empty(B * H, S, dtype=torch.float32, device=q.device)
    sd = (H * S * D, S * D, D)
    ext.attention_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                      out.data_ptr(), lse.data_ptr(), B, H, S, D, scale,
                      causal, *sd, *sd, _stream())
    return out, (out, lse)


def attention_bwd(dout: torch.Tensor, q, k, v, residuals,
                  causal: bool = True):
    B, H, S, D = q.shape
    scale = 1.0 / math.sqrt(D)
    if len(residuals) == 1:  # composed path
        (p,) = residuals
        dv = matmul(p.transpose(-1, -2), dout)
        dp = matmul(dout, v.transpose(-1, -2))
        ds = softmax_bwd(dp, p, scale=scale)
        dq = matmul(ds, k)
        dk = matmul(ds.transpose(-1, -2), q)
        return dq, dk, dv
    out, lse = residuals
    _check_attention_operands("attention_bwd", q, k=k, v=v, out=out,
                              dout=dout)
    lse = _check_lse("attention_bwd", lse, B * H, S)
    # the launch below passes contiguous strides: whatever views the caller
    # saved (a transposed q from reshape(B, S, H, D).transpose(1, 2)) are
    # made contiguous first, a no-op for tensors that already are, and the
    # gradients are allocated contiguous, not with a view's strides
    q, k, v, out, dout = (t.contiguous() for t in (q, k, v, out, dout))
    delta = torch.empty(B * H, S, dtype=torch.float32, device=q.device)
    dq, dk, dv = (torch.empty(q.shape, dtype=q.dtype, device=q.device)
                  for _ in range(3))
    sd = (H * S * D, S * D, D)
    ext.attention_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                      out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                      delta.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                      dv.data_ptr(), B, H, S, D, scale, causal, *sd, *sd,
                      _stream())
    return dq, dk, dv


_DECODE_SPLITS = os.environ.get("TEPDIST_DECODE_SPLITS")


def decode_splits(bh: int, s_max: int, group: int = 1) -> int:
    """KV splits for decode_attention: a static function of the shapes
    (bh = B*Hkv workgroups per split, S_max, group = H/Hkv) only (no
    device read, so a captured launch keeps its grid). Measured
    (docs/KERNELS.md "Decode attention", profiles/decode_attention.json):
    the combine launch costs 2-3 us, so at S_max 640 one workgroup per
    (b, h) wins from B*H = 64 up (6.8 vs 8.1 us at 64, 17.8 vs 20.5 us at
    512); splitting pays only when few (b, h) pairs stream a long cache
    (B*H = 16, S_max 2048: 14.3 us unsplit, 9.4 us at 4 splits, 10.1 at
    8). Hence: double while the grid stays within 64 workgroups and each
    split keeps >= 512 rows. With group >= 4 a workgroup serves 4-8
    queries in 180-244 VGPRs (two waves per SIMD), there are 1/group as
    many workgroups and each takes longer, so filling the 256 CUs pays
    earlier (profiles/decode_attention_gqa.json: B*Hkv = 128, S_max 640,
    G = 8, D = 64: 26.2 us unsplit, 21.0 at 2, 22.6 at 4; B*Hkv = 256,
    G = 4: 15.1 unsplit, 19.7 at 2): double while the grid stays within
    256 workgroups and each split keeps >= 256 rows.
    TEPDIST_DECODE_SPLITS pins a value."""
    if _DECODE_SPLITS:
        return max(1, min(32, int(_DECODE_SPLITS)))
    max_wg, min_rows = (256, 256) if group >= 4 else (64, 512)
    s = 1
    while s < 16 and bh * s * 2 <= max_wg and s_max // (s * 2) >= min_rows:
        s *= 2
    return s


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, positions: torch.Tensor,
                     k_new: Optional[torch.Tensor] = None,
                     v_new: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None,
                     splits: Optional[int] = None,
                     rope_theta: Optional[float] = None) -> torch.Tensor:
    """Fused single-query attention over a KV cache (decode_attention.hip).
    Same semantics as reference.decode_attention, including the in-place
    cache write of (k_new, v_new) at the device-side position, grouped
    queries (caches and new rows with Hkv heads, H / Hkv in {1, 2, 4, 8})
    and the in-kernel rotation of q and k_new when rope_theta is given.
    Strided [B, H, D] views (e.g. of the packed qkv projection) and cache
    slices are consumed without a copy."""
    if q.dim() != 3 or k_cache.dim() != 4:
        raise ValueError("decode_attention: q [B,H,D], caches "
                         "[B,Hkv,S_max,D]")
    B, H, D = q.shape
    Hkv, S_max = k_cache.shape[1], k_cache.shape[2]
    if q.dtype != BF16 or k_cache.dtype != BF16 or v_cache.dtype != BF16:
        raise ValueError("decode_attention: hip backend is bf16-only")
    if D not in (64, 128):
        raise ValueError(f"decode_attention: head dim {D} not in (64, 128)")
    if (k_new is None) != (v_new is None):
        raise ValueError("decode_attention: k_new and v_new go together")
    if Hkv < 1 or H % Hkv != 0 or H // Hkv not in (1, 2, 4, 8):
        raise ValueError(f"decode_attention: {H} query heads over {Hkv} "
                         "K/V heads: the group size must be 1, 2, 4 or 8")
    if tuple(k_cache.shape) != (B, Hkv, S_max, D) or \
            v_cache.shape != k_cache.shape or \
            v_cache.stride() != k_cache.stride():
        raise ValueError("decode_attention: k_cache/v_cache must be "
                         "[B,Hkv,S_max,D] with equal strides")
    if q.stride(2) != 1 or k_cache.stride(3) != 1:
        raise ValueError("decode_attention: D must be contiguous")
    if rope_theta is not None and not rope_theta > 0:
        raise ValueError("decode_attention: rope_theta must be positive")
    n_bs = n_hs = 0
    if k_new is not None:
        if k_new.dtype != BF16 or v_new.dtype != BF16 or \
                tuple(k_new.shape) != (B, Hkv, D) or \
                v_new.shape != k_new.shape or \
                k_new.stride() != v_new.stride() or k_new.stride(2) != 1:
            raise ValueError("decode_attention: k_new/v_new must be bf16 "
                             "[B,Hkv,D] with equal strides, D contiguous")
        n_bs, n_hs = k_new.stride(0), k_new.stride(1)
    pos = positions.reshape(-1)
    if pos.dtype != torch.int64 or not pos.is_cuda or \
            pos.numel() not in (1, B):
        raise ValueError("decode_attention: positions must be a device "
                         "int64 tensor with 1 or B elements")
    pos = pos.contiguous()
    pos_stride = 1 if (pos.numel() == B and B > 1) else 0
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if splits is None:
        splits = decode_splits(B * Hkv, S_max, H // Hkv)
    out = torch.empty(B, H, D, dtype=BF16, device=q.device)
    ws = torch.empty(B * H * splits * (D + 2), dtype=torch.float32,
                     device=q.device) if splits > 1 else None
    ext.decode_attention(q.data_ptr(), _p(k_new), _p(v_new),
                         k_cache.data_ptr(), v_cache.data_ptr(),
                         pos.data_ptr(), pos_stride, out.data_ptr(), _p(ws),
                         B, H, Hkv, S_max, D, scale, splits,
                         rope_theta is not None, float(rope_theta or 0.0),
                         q.stride(0),
                         q.stride(1), n_bs, n_hs, k_cache.stride(0),
                         k_cache.stride(1), k_cache.stride(2), _stream())
    return out


def sample_logits(logits: torch.Tensor, temperature: float, top_k: int = 0,
                  top_p: float = 1.0, seed: int = 0,
                  step: Optional[torch.Tensor] = None,
                  u: Optional[torch.Tensor] = None,
                  vocab: Optional[int] = None,
                  out: Optional[torch.Tensor] = None,
                  return_threshold: bool = False):
    """One token per row of logits [B, Vs] (sampling.hip), the rules of
    reference.sample_logits. One launch on the current stream, no
    workspace, nothing read back: `step` stays on the device, so a captured
    launch draws a fresh uniform at every replay. fp32 and bf16 rows of any
    row stride and alignment are read in place."""
    from tepdist_amd.ops.reference import sample_check
    B, vocab = sample_check(logits, temperature, top_k, top_p, step, u,
                            vocab, out)
    if out is None:
        out = torch.empty(B, 1, dtype=torch.int64, device=logits.device)
    tau = torch.empty(B, dtype=torch.float32, device=logits.device) \
        if return_threshold else None
    ext.sample_logits(logits.data_ptr(), logits.dtype == BF16,
                      logits.stride(0), B, vocab, float(temperature),
                      int(top_k), min(float(top_p), 1.0),
                      int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step), _p(u),
                      out.data_ptr(), _p(tau), _stream())
    return (out, tau) if return_threshold else out


def _packed_dims(name: str, qkv: torch.Tensor, heads: int):
    """(B, S, D) of a packed qkv [B, S, 3*heads*D]; anything that does not
    split that way is refused (the launch would take D = d // heads and
    read past the heads)."""
    if qkv.dim() != 3 or heads < 1 or qkv.shape[-1] % (3 * heads):
        raise ValueError(f"{name}: qkv must be [B, S, 3 * heads * D], got "
                         f"{tuple(qkv.shape)} for {heads} heads")
    return qkv.shape[0], qkv.shape[1], qkv.shape[-1] // (3 * heads)


def attention_qkv_fwd(qkv: torch.Tensor, heads: int, causal: bool = True):
    """Packed-projection attention: qkv [B, S, 3*H*D] (q|k|v each [H][D]),
    out [B, S, H*D] — the flash kernels read/write the packed layout
    directly (no transpose copies)."""
    B, S, D = _packed_dims("attention_qkv_fwd", qkv, heads)
    d = heads * D
    d3 = 3 * d
    if D not in (64, 128) or _ATTN_IMPL == "composed":
        return None  # caller falls back to the split path
    if qkv.dtype != torch.bfloat16:
        raise ValueError(f"attention_qkv_fwd: qkv is {qkv.dtype}, the "
                         "flash kernels are bf16-only")
    qkv = qkv.contiguous()
    scale = 1.0 / math.sqrt(D)
    out = torch.empty(B, S, d, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B * heads, S, dtype=torch.float32, device=qkv.device)
    qs = (S * d3, D, d3)
    os_ = (S * d, D, d)
    base = qkv.data_ptr()
    esz = qkv.element_size()
    ext.attention_fwd(base, base + d * esz, base + 2 * d * esz,
                      out.data_ptr(), lse.data_ptr(), B, heads, S, D, scale,
                      causal, *qs, *os_, _stream())
    return out, (out, lse)


def attention_qkv_bwd(dout: torch.Tensor, qkv: torch.Tensor, heads: int,
                      residuals, causal: bool = True):
    B, S, d3 = qkv.shape
    d = d3 // 3
    D = d // heads
    if len(residuals) != 2:  # composed fallback (q, k, v, p)
        q, k, v, p = residuals
        dout4 = dout.reshape(B, S, heads, D).transpose(1, 2).contiguous()
        dq, dk, dv = attention_bwd(dout4, q, k, v, (p,), causal=causal)
        def back(t):
            return t.transpose(1, 2).reshape(B, S, d)
        return torch.cat([back(dq), back(dk), back(dv)], dim=-1)
    out, lse = residuals
    _packed_dims("attention_qkv_bwd", qkv, heads)
    if D not in (64, 128):
        raise ValueError(f"attention_qkv_bwd: flash residuals with head dim "
                         f"{D}; the flash kernels take 64 or 128")
    for what, t in (("qkv", qkv), ("out", out), ("dout", dout)):
        if t.dtype != torch.bfloat16 or t.device != qkv.device:
            raise ValueError(f"attention_qkv_bwd: {what} is {t.dtype} on "
                             f"{t.device}; the flash kernels take bf16 on "
                             "one device")
    for what, t in (("out", out), ("dout", dout)):
        if t.shape != (B, S, d):
            raise ValueError(f"attention_qkv_bwd: {what} is "
                             f"{tuple(t.shape)}, expected {(B, S, d)}")
    lse = _check_lse("attention_qkv_bwd", lse, B * heads, S)
    scale = 1.0 / math.sqrt(D)
    qkv, out, dout = qkv.contiguous(), out.contiguous(), dout.contiguous()
    delta = torch.empty(B * heads, S, dtype=torch.float32, device=qkv.device)
    dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
    qs = (S * d3, D, d3)
    os_ = (S * d, D, d)
    base = qkv.data_ptr()
    dbase = dqkv.data_ptr()
    esz = qkv.element_size()
    # the dQ kernel writes the packed strided layout directly (no fp32
    # workspace, no scatter pass)
    ext.attention_bwd(base, base + d * esz, base + 2 * d * esz,
                      out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                      delta.data_ptr(), dbase, dbase + d * esz,
                      dbase + 2 * d * esz, B, heads, S, D, scale, causal,
                      *qs, *os_, _stream())
    return dqkv


# --------------------------------------------------------------------------
# Embedding
# --------------------------------------------------------------------------

def embedding_fwd(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    ids_flat = ids.reshape(-1).contiguous()
    if ids_flat.dtype != torch.int64:
        ids_flat = ids_flat.long()
    dim = table.shape[1]
    out = torch.empty(ids_flat.numel(), dim, dtype=BF16, device=table.device)
    ext.embedding_fwd(ids_flat.data_ptr(), table.data_ptr(), out.data_ptr(),
                      ids_flat.numel(), dim, _stream())
    return out.reshape(*ids.shape, dim)


def embedding_bwd(dy: torch.Tensor, ids: torch.Tensor,
                  vocab: int) -> torch.Tensor:
    dim = dy.shape[-1]
    dy_flat = dy.reshape(-1, dim).contiguous()
    ids_flat = ids.reshape(-1).contiguous()
    if ids_flat.dtype != torch.int64:
        ids_flat = ids_flat.long()
    grad_f32 = torch.zeros(vocab, dim, dtype=torch.float32, device=dy.device)
    grad = torch.empty(vocab, dim, dtype=BF16, device=dy.device)
    ext.embedding_bwd(dy_flat.data_ptr(), ids_flat.data_ptr(),
                      grad_f32.data_ptr(), grad.data_ptr(),
                      ids_flat.numel(), vocab, dim, _stream())
    return grad


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------

def cross_entropy_fwd(logits: torch.Tensor, targets: torch.Tensor,
                      ignore_index: int = -1):
    logits = logits.contiguous()
    rows, cols = logits.shape
    targets = targets.contiguous()
    if targets.dtype != torch.int64:
        targets = targets.long()
    nll = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    ext.cross_entropy_fwd(logits.data_ptr(), targets.data_ptr(),
                          nll.data_ptr(), lse.data_ptr(), rows, cols,
                          ignore_index, _stream())
    n = (targets != ignore_index).sum().clamp_min(1)
    return nll.sum() / n, lse


def cross_entropy_bwd(dloss: torch.Tensor, logits: torch.Tensor,
                      targets: torch.Tensor, lse: torch.Tensor,
                      ignore_index: int = -1) -> torch.Tensor:
    rows, cols = logits.shape
    targets = targets.contiguous()
    if targets.dtype != torch.int64:
        targets = targets.long()
    # scale stays on device (graph-capturable: no host readback)
    n = (targets != ignore_index).sum().clamp_min(1)
    dscale = (dloss.to(logits.device).float() / n).contiguous()
    dlogits = torch.empty_like(logits)
    ext.cross_entropy_bwd(logits.data_ptr(), targets.data_ptr(),
                          lse.data_ptr(), dscale.data_ptr(),
                          dlogits.data_ptr(), rows, cols, ignore_index,
                          _stream())
    return dlogits


# --------------------------------------------------------------------------
# Dropout
# --------------------------------------------------------------------------

def dropout_fwd(x: torch.Tensor, p: float, seed: int, offset: int):
    if p == 0.0:
        return x, None
    x = x.contiguous()
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ext.dropout_fwd(x.data_ptr(), y.data_ptr(), mask.data_ptr(), x.numel(), p,
                    seed, offset, _stream())
    return y, mask


def dropout_bwd(dy: torch.Tensor, mask: Optional[torch.Tensor], p: float):
    if p == 0.0 or mask is None:
        return dy
    dx = torch.empty_like(dy)
    ext.dropout_bwd(dy.data_ptr(), mask.data_ptr(), dx.data_ptr(), dy.numel(),
                    p, _stream())
    return dx


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

class AdamWMT:
    """Multi-tensor fused AdamW context: static pointer/chunk tables on
    device; only the gradient pointer table refreshes per step."""

    CHUNK = 16384

    def __init__(self, params, states, wds):
        dev = params[0].device
        self.nt = len(params)
        # per-tensor storage type: 0 = bf16 param+grad, 1 = fp32 (e.g.
        # Wide-ResNet batch-norm affines)
        self.ptypes = torch.tensor(
            [1 if p.dtype == torch.float32 else 0 for p in params],
            dtype=torch.uint8, device=dev)
        ptrs = ([p.data_ptr() for p in params] +
                [s["master"].data_ptr() for s in states] +
                [0] * self.nt +
                [s["exp_avg"].data_ptr() for s in states] +
                [s["exp_avg_sq"].data_ptr() for s in states])
        self.tabs = torch.tensor(ptrs, dtype=torch.int64, device=dev)
        self.numel = torch.tensor([p.numel() for p in params],
                                  dtype=torch.int64, device=dev)
        self.wds = torch.tensor(wds, dtype=torch.float32, device=dev)
        chunks = []
        for ti, p in enumerate(params):
            for c in range((p.numel() + self.CHUNK - 1) // self.CHUNK):
                chunks.extend((ti, c))
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self.nchunks = len(chunks) // 2
        self._gslot = self.tabs[2 * self.nt:3 * self.nt]

    def step(self, grads, lr, beta1, beta2, eps, step_no):
        gp = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        self._gslot.copy_(gp, non_blocking=True)
        bc1 = 1.0 - beta1 ** step_no
        bc2 = 1.0 - beta2 ** step_no
        ext.adamw_mt(self.tabs.data_ptr(), self.numel.data_ptr(),
                     self.wds.data_ptr(), self.ptypes.data_ptr(),
                     self.chunks.data_ptr(),
                     self.nchunks, self.nt, lr, beta1, beta2, eps, bc1, bc2,
                     0, _stream())

    # -- hipGraph-capture path: the kernel reads step-dependent scalars
    # from a persistent device buffer the host updates before each replay
    # (kernel args would be frozen inside the captured graph) ------------

    def prepare_graph(self, grads):
        gp = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        self._gslot.copy_(gp)
        self.hyper = torch.zeros(4, dtype=torch.float32,
                                 device=self.tabs.device)

    def step_graph(self, beta1, beta2, eps):
        ext.adamw_mt(self.tabs.data_ptr(), self.numel.data_ptr(),
                     self.wds.data_ptr(), self.ptypes.data_ptr(),
                     self.chunks.data_ptr(),
                     self.nchunks, self.nt, 0.0, beta1, beta2, eps, 1.0,
                     1.0, self.hyper.data_ptr(), _stream())

    def set_hyper(self, lr, beta1, beta2, step_no):
        # the eager launcher rounds bc1/bc2 to fp32 and then forms
        # 1.0f / bc; do the same here (not fp32(1 / bc) from a double
        # quotient, which differs in the last bit, e.g. at bc2 = 0.001) so
        # a replayed step equals the eager one bit for bit
        vals = torch.tensor([lr, 1.0 - beta1 ** step_no,
                             1.0 - beta2 ** step_no, 0.0],
                            dtype=torch.float32)
        vals[1:3] = torch.ones(2, dtype=torch.float32) / vals[1:3]
        self.hyper.copy_(vals, non_blocking=True)


def adamw_step(param_bf16: torch.Tensor, master: torch.Tensor,
               grad: torch.Tensor, exp_avg: torch.Tensor,
               exp_avg_sq: torch.Tensor, lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    g = grad.contiguous()
    gb = g.data_ptr() if g.dtype == BF16 else 0
    gf = g.data_ptr() if g.dtype == torch.float32 else 0
    assert gb or gf, f"grad dtype {g.dtype}"
    ext.adamw(param_bf16.data_ptr(), master.data_ptr(), gb, gf,
              exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param_bf16.numel(),
              lr, beta1, beta2, eps, weight_decay, bc1, bc2, _stream())


# --------------------------------------------------------------------------
# Llama-family ops (RMSNorm / RoPE / SwiGLU)
# --------------------------------------------------------------------------

def rmsnorm_fwd(x: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-6):
    x = x.contiguous()
    rows, cols = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    ext.rmsnorm_fwd(x.data_ptr(), gamma.contiguous().data_ptr(), y.data_ptr(),
                    rstd.data_ptr(), rows, cols, eps, _stream())
    return y, rstd


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor,
                rstd: torch.Tensor):
    rows, cols = x.shape
    dy = dy.contiguous()
    part_rows = min((rows + 3) // 4 * 4, 2048 * 4)
    dg_part = torch.zeros(part_rows, cols, dtype=torch.float32,
                          device=x.device)
    dx = torch.empty_like(x)
    dg = torch.empty_like(gamma)
    ext.rmsnorm_bwd(dy.data_ptr(), x.data_ptr(),
                    gamma.contiguous().data_ptr(), rstd.data_ptr(),
                    dx.data_ptr(), dg.data_ptr(), dg_part.data_ptr(),
                    part_rows, rows, cols, _stream())
    return dx, dg


def rope_fwd(x: torch.Tensor, seq_len: int, theta: float = 10000.0):
    T, H, D = x.shape
    y = torch.empty_like(x)
    ext.rope(x.data_ptr(), y.data_ptr(), T, H, D, seq_len, theta, False,
             _stream())
    return y


def rope_bwd(dy: torch.Tensor, seq_len: int, theta: float = 10000.0):
    T, H, D = dy.shape
    dx = torch.empty_like(dy)
    ext.rope(dy.data_ptr(), dx.data_ptr(), T, H, D, seq_len, theta, True,
             _stream())
    return dx


def swiglu_fwd(a: torch.Tensor, b: torch.Tensor):
    y = torch.empty_like(a)
    ext.swiglu_fwd(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(),
                   _stream())
    return y


def swiglu_bwd(dy: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    da = torch.empty_like(a)
    db = torch.empty_like(b)
    ext.swiglu_bwd(dy.data_ptr(), a.data_ptr(), b.data_ptr(), da.data_ptr(),
                   db.data_ptr(), a.numel(), _stream())
    return da, db


# --------------------------------------------------------------------------
# MoE routing / dispatch / combine (csrc/moe_route.hip)
# --------------------------------------------------------------------------

_I32 = torch.int32


def _moe_rows(name: str, t: torch.Tensor, what: str):
    if t.dim() != 2 or t.dtype != BF16 or not t.is_cuda:
        raise ValueError(f"{name}: {what} must be a 2-D bf16 device tensor")
    if t.shape[1] < 8 or t.shape[1] % 8:
        raise ValueError(f"{name}: row width {t.shape[1]} is not a positive "
                         "multiple of 8")
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{name}: {what} must be contiguous and 16-byte "
                         "aligned")


def _moe_map(name: str, t: torch.Tensor, shape, what: str,
             dtype=_I32):
    if t.dtype != dtype or not t.is_cuda or tuple(t.shape) != tuple(shape) \
            or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} "
                         f"device tensor of shape {tuple(shape)}, got "
                         f"{t.dtype} {tuple(t.shape)}")


def _moe_k(name: str, T: int, k: int, EC: int):
    if not 1 <= k <= 4 or T < 1 or T * k >= 2 ** 31 or \
            not 1 <= EC < 2 ** 31:
        raise ValueError(f"{name}: need 1 <= k <= 4, T*k < 2^31 and "
                         f"1 <= E*C < 2^31 (T={T}, k={k}, E*C={EC})")


def moe_route(gates: torch.Tensor, k: int, capacity: int):
    """Same contract as reference.moe_route; every output element is
    written by the kernels (three launches, no atomics, no host sync)."""
    if gates.dim() != 2 or not gates.is_cuda:
        raise ValueError("moe_route: gates must be a [T, E] device tensor")
    if gates.dtype not in (BF16, torch.float32):
        raise ValueError("moe_route: gates must be bf16 or fp32")
    if not gates.is_contiguous():
        raise ValueError("moe_route: gates must be contiguous")
    T, E = gates.shape
    k, C = int(k), int(capacity)
    if not 2 <= E <= 64:
        raise ValueError(f"moe_route: E={E} not in [2, 64]")
    if not 1 <= k <= min(4, E):
        raise ValueError(f"moe_route: k={k} not in [1, min(4, E)]")
    if C < 1:
        raise ValueError("moe_route: capacity must be >= 1")
    _moe_k("moe_route", T, k, E * C)
    dev = gates.device
    topi = torch.empty(T, k, dtype=_I32, device=dev)
    slot = torch.empty(T, k, dtype=_I32, device=dev)
    src = torch.empty(E * C, dtype=_I32, device=dev)
    counts = torch.empty(E, dtype=_I32, device=dev)
    ws = torch.empty(ext.moe_route_ws_ints(T, E), dtype=_I32, device=dev)
    ext.moe_route(gates.data_ptr(), gates.dtype == torch.float32,
                  topi.data_ptr(), slot.data_ptr(), src.data_ptr(),
                  counts.data_ptr(), ws.data_ptr(), T, E, k, C, _stream())
    return topi, slot, src, counts


def moe_dispatch_fwd(x: torch.Tensor, src: torch.Tensor, k: int):
    _moe_rows("moe_dispatch", x, "x")
    T, d = x.shape
    EC = src.numel()
    _moe_k("moe_dispatch", T, k, EC)
    _moe_map("moe_dispatch", src, (EC,), "src")
    D = torch.empty(EC, d, dtype=BF16, device=x.device)
    ext.moe_gather_rows(x.data_ptr(), src.data_ptr(), 0, D.data_ptr(), T, k,
                        EC, d, _stream())
    return D


def moe_dispatch_bwd(dD: torch.Tensor, slot: torch.Tensor):
    _moe_rows("moe_dispatch backward", dD, "dD")
    EC, d = dD.shape
    if slot.dim() != 2:
        raise ValueError("moe_dispatch backward: slot must be [T, k]")
    T, k = slot.shape
    _moe_k("moe_dispatch backward", T, k, EC)
    _moe_map("moe_dispatch backward", slot, (T, k), "slot")
    dx = torch.empty(T, d, dtype=BF16, device=dD.device)
    ext.moe_reduce_rows(dD.data_ptr(), slot.data_ptr(), 0, dx.data_ptr(), T,
                        k, EC, d, _stream())
    return dx


def moe_combine_fwd(y: torch.Tensor, w: torch.Tensor, slot: torch.Tensor):
    _moe_rows("moe_combine", y, "y")
    EC, d = y.shape
    if slot.dim() != 2:
        raise ValueError("moe_combine: slot must be [T, k]")
    T, k = slot.shape
    _moe_k("moe_combine", T, k, EC)
    _moe_map("moe_combine", slot, (T, k), "slot")
    _moe_map("moe_combine", w, (T, k), "weights", torch.float32)
    out = torch.empty(T, d, dtype=BF16, device=y.device)
    ext.moe_reduce_rows(y.data_ptr(), slot.data_ptr(), w.data_ptr(),
                        out.data_ptr(), T, k, EC, d, _stream())
    return out


def moe_combine_bwd(dout: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                    slot: torch.Tensor, src: torch.Tensor):
    _moe_rows("moe_combine backward", y, "y")
    _moe_rows("moe_combine backward", dout, "dout")
    EC, d = y.shape
    if slot.dim() != 2:
        raise ValueError("moe_combine backward: slot must be [T, k]")
    T, k = slot.shape
    _moe_k("moe_combine backward", T, k, EC)
    if tuple(dout.shape) != (T, d):
        raise ValueError("moe_combine backward: dout must be [T, d]")
    _moe_map("moe_combine backward", slot, (T, k), "slot")
    _moe_map("moe_combine backward", src, (EC,), "src")
    _moe_map("moe_combine backward", w, (T, k), "weights", torch.float32)
    dy = torch.empty(EC, d, dtype=BF16, device=y.device)
    dw = torch.empty(T, k, dtype=torch.float32, device=y.device)
    ext.moe_gather_rows(dout.data_ptr(), src.data_ptr(), w.data_ptr(),
                        dy.data_ptr(), T, k, EC, d, _stream())
    ext.moe_combine_dw(y.data_ptr(), dout.data_ptr(), slot.data_ptr(),
                       dw.data_ptr(), T, k, EC, d, _stream())
    return dy, dw
