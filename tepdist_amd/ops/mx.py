"""OCP Microscaling (MX) weight formats for the decode linears: storage,
quantizer and the reference dequantizer. Plain torch; runs once at load.

Storage of a weight [N, K] (K a multiple of 32), as in the OCP MX spec. It
is both the interchange layout and the kernel's layout (csrc/
skinny_mx_gemm.hip reads it as it lies):

- a block is 32 consecutive k of one row and shares one e8m0 scale byte:
  scales [N, K / 32] uint8, value 2^(byte - 127);
- "mxfp8": elements e4m3 (OCP `fn` encoding, no infinities, NaN = 0x7f /
  0xff), codes [N, K] uint8;
- "mxfp4": elements e2m1, codes [N, K / 2] uint8, even k in the low nibble.

Quantizer (mx_quantize), the spec's rule: the block's scale is
2^(floor(log2 amax) - emax_elem), emax_elem = 2 (e2m1) or 8 (e4m3); elements
are w / scale rounded to nearest, ties to the even code, saturated to +-6 or
+-448; the e4m3 NaN codes are never emitted. An all-zero block gets scale
byte 127.

Scale clamp: the exponent is clamped so that every nonzero dequantized value
is a finite, normal bf16 (an element times a power of two is then exact in
bf16, which is what makes the kernels testable to the bit). The smallest
nonzero elements are 2^-9 (e4m3) and 2^-1 (e2m1), the largest 1.75 * 2^8 and
1.5 * 2^2; bf16 normals span 2^-126 .. 1.99 * 2^127. Hence

    mxfp8: scale byte in [10, 246]   (exponent -117 .. 119)
    mxfp4: scale byte in [2, 252]    (exponent -125 .. 125)

Bytes 0 and 255 (the e8m0 NaN) never occur, so a kernel may form the fp32
scale as `byte << 23`. For finite fp32 / bf16 input only the lower clamp can
bind (a block whose amax lies below 2^-109 or 2^-123): its small elements
then round to zero or to the lowest codes, still to nearest."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import torch

BLOCK = 32
FORMATS = ("mxfp8", "mxfp4")
# (bits, emax_elem, element max, lowest and highest scale byte)
_SPEC = {"mxfp8": (8, 8, 448.0, 10, 246), "mxfp4": (4, 2, 6.0, 2, 252)}
_ROWS = 8192
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _spec(fmt: str):
    if fmt not in _SPEC:
        raise ValueError(f"weight format must be one of {FORMATS}, "
                         f"got {fmt!r}")
    return _SPEC[fmt]


def bits(fmt: str) -> int:
    return _spec(fmt)[0]


def scale_byte_range(fmt: str) -> Tuple[int, int]:
    return _spec(fmt)[3:]


def table(fmt: str) -> torch.Tensor:
    """fp32 value of every element code: 16 (e2m1) or 256 (e4m3, NaN at
    0x7f and 0xff)."""
    if bits(fmt) == 4:
        t = torch.tensor(E2M1)
        return torch.cat([t, -t])
    return torch.arange(256, dtype=torch.uint8).view(
        torch.float8_e4m3fn).float()


@dataclass
class MXWeight:
    """A quantized weight: codes and scales in the layout above, fmt
    "mxfp8" | "mxfp4", shape the logical (N, K)."""
    codes: torch.Tensor
    scales: torch.Tensor
    fmt: str
    shape: Tuple[int, int]

    def to(self, device) -> "MXWeight":
        return MXWeight(self.codes.to(device), self.scales.to(device),
                        self.fmt, self.shape)

    def cuda(self) -> "MXWeight":
        return self.to("cuda")

    @property
    def nbytes(self) -> int:
        return self.codes.numel() + self.scales.numel()


def mx_quantize(w: torch.Tensor, fmt: str) -> MXWeight:
    """Quantize w [N, K] (any float dtype, K % 32 == 0) by the rule above."""
    nbits, emax, vmax, lo, hi = _spec(fmt)
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(f"mx_quantize: w must be [N, K] with K a multiple "
                         f"of {BLOCK}, got {tuple(w.shape)}")
    N, K = w.shape
    if N > _ROWS:           # bounds the float64 temporaries of a big head
        parts = [mx_quantize(w[r:r + _ROWS], fmt) for r in range(0, N, _ROWS)]
        return MXWeight(torch.cat([p.codes for p in parts]),
                        torch.cat([p.scales for p in parts]), fmt, (N, K))
    # float64 holds every fp32 / bf16 value over every power-of-two scale
    # exactly, so the only rounding below is the element rounding
    blk = w.detach().double().reshape(N, K // BLOCK, BLOCK)
    amax = blk.abs().amax(dim=-1)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    byte = (torch.frexp(amax)[1] - 1 - emax + 127).clamp(lo, hi)
    byte = torch.where(amax == 0, torch.full_like(byte, 127), byte)
    q = torch.ldexp(blk, (127 - byte)[..., None]).clamp(-vmax, vmax)
    q = q.reshape(N, K)
    if nbits == 8:
        # torch's cast rounds to nearest even (subnormals included) and
        # would return NaN above 448: q is already clamped
        codes = q.float().to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        a = q.abs()
        step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
        v = torch.round(a / step) * step        # half to even = even code
        c = torch.where(v < 2, v * 2, torch.where(v < 4, v + 2, v / 2 + 4))
        c = c.to(torch.uint8) | ((q < 0).to(torch.uint8) << 3)
        codes = c[:, 0::2] | (c[:, 1::2] << 4)
    return MXWeight(codes.contiguous(), byte.to(torch.uint8).contiguous(),
                    fmt, (N, K))


def check(mw: MXWeight) -> Tuple[int, int]:
    """(N, K) of a well-formed MXWeight, else ValueError."""
    nbits = bits(mw.fmt)
    N, K = mw.shape
    if K % BLOCK or mw.codes.dtype != torch.uint8 or \
            mw.scales.dtype != torch.uint8 or \
            tuple(mw.codes.shape) != (N, K * nbits // 8) or \
            tuple(mw.scales.shape) != (N, K // BLOCK):
        raise ValueError(
            f"MXWeight {mw.fmt} of shape {(N, K)}: codes must be uint8 "
            f"[N, K * {nbits} / 8] and scales uint8 [N, K / 32], got "
            f"{tuple(mw.codes.shape)} and {tuple(mw.scales.shape)}")
    return N, K


def dequantize_ref(mw: MXWeight) -> torch.Tensor:
    """bf16 [N, K]: the table value of every code times its block's scale.
    Exact for every code and every scale byte in the format's range."""
    N, K = check(mw)
    codes = mw.codes
    if bits(mw.fmt) == 4:
        codes = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N, K)
    v = table(mw.fmt).to(codes.device)[codes.long()]
    e = mw.scales.to(torch.int32) - 127
    return torch.ldexp(v.reshape(N, K // BLOCK, BLOCK),
                       e[..., None]).reshape(N, K).to(torch.bfloat16)


# --------------------------------------------------------------------------
# MXFP8 KV cache
# --------------------------------------------------------------------------

@dataclass
class MXCache:
    """A K or V cache held as MXFP8: codes uint8 [B, Hkv, S_max, D] (e4m3,
    `fn` encoding) and scales uint8 [B, Hkv, S_max, D / 32] (e8m0), fmt
    "mxfp8" only. Every (b, h) plane is an MXWeight [S_max, D] in the layout
    above: a block is 32 consecutive d of one row, scale bytes lie in
    [10, 246] and the NaN codes are never written. Views are allowed (a batch
    slice, an S_max slice of a larger buffer) as long as D is contiguous and
    code rows are 8-byte aligned; codes and scales carry their own strides."""
    codes: torch.Tensor
    scales: torch.Tensor
    fmt: str = "mxfp8"

    @property
    def shape(self):
        return tuple(self.codes.shape)

    def to(self, device) -> "MXCache":
        return MXCache(self.codes.to(device), self.scales.to(device),
                       self.fmt)

    def clone(self) -> "MXCache":
        return MXCache(self.codes.clone(), self.scales.clone(), self.fmt)

    @property
    def nbytes(self) -> int:
        return self.codes.numel() + self.scales.numel()


def kv_cache(B: int, Hkv: int, S_max: int, D: int, device=None) -> MXCache:
    """A zero-filled MXFP8 cache: every code 0, every scale byte 127."""
    if D % BLOCK:
        raise ValueError(f"kv_cache: head dim {D} is no multiple of {BLOCK}")
    return MXCache(
        torch.zeros(B, Hkv, S_max, D, dtype=torch.uint8, device=device),
        torch.full((B, Hkv, S_max, D // BLOCK), 127, dtype=torch.uint8,
                   device=device))


def check_cache(c: MXCache) -> Tuple[int, int, int, int]:
    """(B, Hkv, S_max, D) of a well-formed MXCache, else ValueError."""
    if c.fmt != "mxfp8":
        raise ValueError(f"MXCache: fmt must be 'mxfp8', got {c.fmt!r}")
    if c.codes.dim() != 4 or c.codes.shape[3] % BLOCK:
        raise ValueError(f"MXCache: codes must be [B, Hkv, S_max, D] with D "
                         f"a multiple of {BLOCK}, got {tuple(c.codes.shape)}")
    B, Hkv, S_max, D = c.codes.shape
    if c.codes.dtype != torch.uint8 or c.scales.dtype != torch.uint8 or \
            tuple(c.scales.shape) != (B, Hkv, S_max, D // BLOCK) or \
            c.scales.device != c.codes.device:
        raise ValueError(
            f"MXCache of shape {(B, Hkv, S_max, D)}: codes and scales must "
            f"be uint8 on one device, scales [B, Hkv, S_max, D / 32], got "
            f"{tuple(c.scales.shape)}")
    return B, Hkv, S_max, D


def cache_dequantize(c: MXCache) -> torch.Tensor:
    """bf16 [B, Hkv, S_max, D] by dequantize_ref's rule: exact for every code
    and every in-range scale byte."""
    B, Hkv, S_max, D = check_cache(c)
    v = table(c.fmt).to(c.codes.device)[c.codes.long()]
    e = c.scales.to(torch.int32) - 127
    return torch.ldexp(v.reshape(B, Hkv, S_max, D // BLOCK, BLOCK),
                       e[..., None]).reshape(B, Hkv, S_max, D) \
        .to(torch.bfloat16)


def cache_write(c: MXCache, bidx: torch.Tensor, rows: torch.Tensor,
                x: torch.Tensor) -> None:
    """c[bidx, :, rows] = mx_quantize(x rounded to bf16): x [..., Hkv, D]
    with leading dims those of the broadcast (bidx, rows)."""
    _, Hkv, _, D = check_cache(c)
    q = mx_quantize(x.to(torch.bfloat16).reshape(-1, D), "mxfp8")
    lead = tuple(x.shape[:-2])
    c.codes[bidx, :, rows] = q.codes.to(c.codes.device).reshape(
        *lead, Hkv, D)
    c.scales[bidx, :, rows] = q.scales.to(c.codes.device).reshape(
        *lead, Hkv, D // BLOCK)
