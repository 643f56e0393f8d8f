"""MXFP4 activations on the host: the e2m1 rule of csrc/mx_gemm_a8_plan.h (the
lines the quantizer kernel runs) through ext.mx_act_quant_block(row, 4)
against mx.mx_quantize, the plan's x_bits argument, and the reference ops."""

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import _tepdist_hip as ext
from tepdist_amd.ops import mx

BF16 = torch.bfloat16


def _plan(x_bits=4, M=128, N=256, K=384, bits=4, ldxc=None, ldxs=None, epi=0,
          tile=0):
    args = (M, N, K, bits, K * bits // 8, K // 32,
            K * (x_bits or 8) // 8 if ldxc is None else ldxc,
            K // 32 if ldxs is None else ldxs, epi, tile)
    return ext.mx_gemm_a8_plan(*args) if x_bits is None else \
        ext.mx_gemm_a8_plan(*args, x_bits)


def test_quantizer_rule_every_finite_bf16():
    """All 65 280 finite patterns in bit order as [510, 128]: ties,
    saturation, subnormals, both zeros, zero blocks and both scale clamps."""
    pat = torch.arange(1 << 16, dtype=torch.int32)
    pat = pat[(pat & 0x7f80) != 0x7f80].reshape(510, 128)
    want = mx.mx_quantize(pat.to(torch.int16).view(BF16), "mxfp4")
    assert {2, 127, 252} <= set(want.scales.unique().tolist())
    for r, row in enumerate(pat.reshape(-1, 32).tolist()):
        byte, codes = ext.mx_act_quant_block(row, 4)
        assert byte == int(want.scales.reshape(-1)[r]), (r, byte)
        assert codes == want.codes.reshape(-1, 16)[r].tolist(), r


@pytest.mark.parametrize("kw", [
    dict(), dict(ldxc=208, ldxs=16), dict(M=1024, N=4096, K=2048),
    dict(tile=64, epi=4)])
def test_plan_accepts_and_matches_a8_tiles(kw):
    """e2m1 code rows of K / 2 bytes or more, 16-byte aligned; the tile rule
    and grid are those of x_bits = 8, and the argument left out is 8."""
    p = _plan(**kw)
    assert p[3] == "" and p[1] == 3
    kw8 = {k: v for k, v in kw.items() if k != "ldxc"}
    assert _plan(8, **kw8) == _plan(None, **kw8) == p


@pytest.mark.parametrize("kw,why", [
    (dict(ldxc=176), "mxfp4 activation code rows must be 16-byte aligned"),
    (dict(ldxc=200), "mxfp4 activation code rows must be 16-byte aligned"),
    (dict(ldxs=13), "activation scale rows must be 4-byte aligned"),
    (dict(bits=8), "mxfp4 activations need mxfp4 weights"),
    (dict(x_bits=6), "x_bits must be 8 (mxfp8) or 4 (mxfp4)"),
    (dict(K=192), "multiple of 128"),
    (dict(x_bits=8, ldxc=192), "activation code rows must be 16-byte")])
def test_plan_refusals(kw, why):
    p = _plan(**kw)
    assert p[:3] == (0, 0, 0) and why in p[3], p


def test_reference_ops():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 256, generator=g).to(BF16)
    mw = ops.mx_quantize(torch.randn(40, 256, generator=g), "mxfp4")
    b = torch.randn(40, generator=g).to(BF16)
    q = ops.mx_quantize_act(x, fmt="mxfp4")
    want = mx.mx_quantize(x.reshape(15, 256), "mxfp4")
    assert q.shape == (15, 256) and q.fmt == "mxfp4"
    assert torch.equal(q.codes, want.codes)
    assert torch.equal(q.scales, want.scales)
    xr = ops.mx_quantize_act(x, roundtrip=True, fmt="mxfp4")
    assert torch.equal(xr, mx.dequantize_ref(want).reshape(x.shape))
    y = ops.linear_mx(xr, mw, b, "gelu")
    assert torch.equal(ops.linear_mx_a8(x, mw, b, "gelu",
                                        act_format="mxfp4"), y)
    assert torch.equal(ops.linear_mx_a8(q, mw, b, "gelu"), y.reshape(15, 40))
    with pytest.raises(ValueError, match="W8A4"):
        ops.linear_mx_a8(q, ops.mx_quantize(torch.randn(40, 256), "mxfp8"))
