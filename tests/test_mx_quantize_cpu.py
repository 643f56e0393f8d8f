"""ops/mx.py on the CPU: the decode tables, the quantizer against a
brute-force nearest-value search under the spec's scale rule, and the CPU
backend of the MX ops."""

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import mx
from tepdist_amd.ops import reference as ref

FMTS = ["mxfp8", "mxfp4"]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
        -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
EMAX = {"mxfp8": 8, "mxfp4": 2}


def test_decode_tables():
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)          # k = 0..31
    packed = (codes[0::2] | (codes[1::2] << 4))[None]
    one = torch.full((1, 1), 127, dtype=torch.uint8)
    got = mx.dequantize_ref(mx.MXWeight(packed, one, "mxfp4", (1, 32)))
    assert got.dtype == torch.bfloat16
    assert torch.equal(got[0].double(), torch.tensor(E2M1 * 2).double())
    c8 = torch.arange(256, dtype=torch.uint8)
    want = c8.view(torch.float8_e4m3fn).float()
    ok = ~want.isnan()
    assert int((~ok).sum()) == 2                                   # 7f, ff
    c8 = torch.where(ok, c8, torch.zeros_like(c8))[None]
    got = mx.dequantize_ref(mx.MXWeight(
        c8, one.expand(1, 8).contiguous(), "mxfp8", (1, 256)))
    assert torch.equal(got[0].float()[ok], want[ok])


def _weights(fmt):
    """Random rows plus the edge blocks: an outlier, all zeros, magnitudes
    under the scale clamp, values above the element maximum, exact ties."""
    lo, _ = mx.scale_byte_range(fmt)
    vmax = mx.table(fmt).nan_to_num(0).max().item()
    w = torch.randn(6, 128, generator=torch.Generator().manual_seed(1))
    w[0, 5] = 3.0e30                      # outlier: the rest of the block -> 0
    w[1, 32:64] = 0.0                     # all-zero block
    w[2, 64:96] *= 2.0 ** (lo - 127 - 2)  # amax below the clamped scale's grid
    w[3, 0:32] = w[3, 0:32].clamp(-1, 1)
    w[3, 3] = 1.1 * vmax                  # same exponent as vmax: saturates
    t = mx.table(fmt)[:mx.table(fmt).numel() // 2]
    t = t[~t.isnan()]
    mids = ((t[:-1] + t[1:]) / 2)[-31:]   # ties at scale 2^0 (amax = vmax)
    w[4, 96:128] = 0.0
    w[4, 96:96 + mids.numel() + 1] = torch.cat([mids, t[-1:]])
    w[5, 96:128] = -w[4, 96:128]
    return w


@pytest.mark.parametrize("fmt", FMTS)
def test_round_trip_is_nearest_even(fmt):
    w = _weights(fmt)
    mw = mx.mx_quantize(w, fmt)
    lo, hi = mx.scale_byte_range(fmt)
    # the spec's scale, clamped to the documented range
    blk = w.double().reshape(6, 4, 32)
    amax = blk.abs().amax(-1)
    e = (torch.floor(torch.log2(amax.clamp_min(1e-300))) - EMAX[fmt]).clamp(
        lo - 127, hi - 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    assert torch.equal(mw.scales.double() - 127, e)
    assert lo <= int(mw.scales.min()) and int(mw.scales.max()) <= hi
    assert int(mw.scales[2, 2]) == lo and int(mw.scales[1, 1]) == 127
    # brute force: the nearest table value, of two equally near the one with
    # the even code; beyond the largest value the nearest is the largest
    t = mx.table(fmt).double()
    finite = ~t.isnan()
    odd = (torch.arange(t.numel()) & 1).bool()
    d = (blk[..., None] / torch.exp2(e)[..., None, None] - t).abs()
    d = torch.where(finite, d, torch.full_like(d, float("inf")))
    d_even = torch.where(odd, torch.full_like(d, float("inf")), d)
    pick = torch.where(d_even.amin(-1) == d.amin(-1), d_even.argmin(-1),
                       d.argmin(-1))
    want = (t[pick] * torch.exp2(e)[..., None]).reshape(6, 128)
    got = mx.dequantize_ref(mw)
    assert torch.equal(got.double(), want)
    assert torch.equal(got.double().abs().amax(1)[3:4],
                       mx.table(fmt).nan_to_num(0).max().double()[None])
    if fmt == "mxfp8":
        assert not ((mw.codes & 0x7F) == 0x7F).any()
    nz = got[got != 0].float().abs()
    assert nz.min() >= 2.0 ** -126 and torch.isfinite(nz).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_cpu_ops_are_the_reference_composition(fmt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 128, generator=g).bfloat16()
    b = torch.randn(24, generator=g).bfloat16()
    r = torch.randn(5, 24, generator=g).bfloat16()
    mw = ops.mx_quantize(torch.randn(24, 128, generator=g), fmt)
    mu = ops.mx_quantize(torch.randn(24, 128, generator=g), fmt)
    w, u = mx.dequantize_ref(mw), mx.dequantize_ref(mu)
    assert isinstance(mw, ops.MXWeight) and mw.shape == (24, 128)
    assert torch.equal(ops.mx_dequantize(mw), w)
    out = torch.empty(24, 128, dtype=torch.bfloat16)
    assert ops.mx_dequantize(mw, out=out) is out and torch.equal(out, w)
    assert torch.equal(ops.linear_decode_mx(x, mw, b, residual=r),
                       ref.linear_decode(x, w, b, residual=r))
    assert torch.equal(ops.linear_decode_mx(x, mw, b, act="gelu"),
                       ref.linear_decode(x, w, b, act="gelu"))
    assert torch.equal(ops.swiglu_linear_decode_mx(x, mw, mu),
                       ref.swiglu_linear_decode(x, w, u))
    with pytest.raises(ValueError, match="weight format"):
        ops.mx_quantize(torch.zeros(4, 32), "int4")
