"""The fused SwiGLU gate/up GEMM on the host: ext.mx_swiglu_a8_plan (csrc/
mx_swiglu_a8_plan.h) by hand, mx_gemm_a8_plan untouched by it, and the
reference ops.linear_mx_a8(act="swiglu") against a direct fp64 computation."""

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import _tepdist_hip as ext
from tepdist_amd.ops import mx

BF16 = torch.bfloat16


def _plan(M=128, I=256, K=384, bits=4, x_bits=8, out_bits=0, epi=0, tile=0,
          up=None, ldoc=None, ldos=None):
    ldc, lds = K * bits // 8, K // 32
    return ext.mx_swiglu_a8_plan(
        M, I, K, bits, ldc, lds, *(up or (I, K, bits, ldc, lds)),
        K * x_bits // 8, K // 32, epi, tile, x_bits, out_bits,
        I * out_bits // 8 if ldoc is None else ldoc,
        I // 32 if ldos is None else ldos)


@pytest.mark.parametrize("kw,want", [
    (dict(), (64, 3, 2 * 8)),                  # 1 x 4 large tiles: no fill
    (dict(M=4096, I=6144, K=2048), (128, 3, 32 * 96)),
    (dict(M=2048, I=1024), (128, 3, 16 * 16)),  # exactly 256 large tiles
    (dict(M=129, I=96, tile=128, out_bits=8), (128, 3, 2 * 2)),
    (dict(M=65, I=503, tile=64, bits=8), (64, 3, 2 * 16)),
    (dict(M=1, I=32, K=128, x_bits=4, out_bits=4, ldoc=24), (64, 3, 1))])
def test_plan_tiles_and_blocks(kw, want):
    assert _plan(**kw) == want + ("",)


@pytest.mark.parametrize("kw,why", [
    (dict(epi=1), "no bias, no residual and no gelu"),
    (dict(up=(128, 384, 4, 192, 12)), "one format and one shape"),
    (dict(up=(256, 384, 8, 192, 12)), "one format and one shape"),
    (dict(up=(256, 384, 4, 208, 12)), "same code and scale row strides"),
    (dict(I=503, out_bits=8), "I to be a multiple of 32"),
    (dict(out_bits=8, ldoc=252), "output code rows must be 8-byte aligned"),
    (dict(out_bits=8, ldos=7), "output scale rows must hold I / 32 bytes"),
    (dict(out_bits=6), "out_bits must be 0"),
    (dict(bits=8, x_bits=4), "W8A4 is not built"),
    (dict(K=192), "multiple of 128")])
def test_plan_refusals(kw, why):
    p = _plan(**kw)
    assert p[:3] == (0, 0, 0) and why in p[3], p


def test_a8_plan_is_unaffected():
    assert ext.mx_gemm_a8_plan(128, 512, 384, 4, 192, 12, 384, 12) == \
        (64, 3, 16, "")
    assert ext.mx_gemm_a8_plan(4096, 6144, 2048, 8, 2048, 64, 2048, 64, 4) \
        == (128, 3, 32 * 48, "")


@pytest.mark.parametrize("fmt,xfmt", [("mxfp4", "mxfp8"), ("mxfp8", "mxfp8"),
                                      ("mxfp4", "mxfp4")])
def test_reference_op(fmt, xfmt):
    M, I, K = 5, 64, 128
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(BF16)
    mg, mu = (ops.mx_quantize(torch.randn(I, K, generator=g) * K ** -0.5, fmt)
              for _ in range(2))
    xq = mx.mx_quantize(x, xfmt)
    G, U = (mx.dequantize_ref(xq).double() @ mx.dequantize_ref(w).double().t()
            for w in (mg, mu))
    h = (G / (1 + torch.exp(-G)) * U).to(BF16)
    got = ops.linear_mx_a8(x, mg, act="swiglu", up=mu, act_format=xfmt)
    assert torch.equal(got, h)
    for out in mx.FORMATS:
        q = ops.linear_mx_a8(xq, mg, act="swiglu", up=mu, out_format=out)
        want = mx.mx_quantize(h, out)
        assert q.fmt == out and q.shape == (M, I)
        assert torch.equal(q.codes, want.codes)
        assert torch.equal(q.scales, want.scales)
    for kw in (dict(act="swiglu"), dict(up=mu), dict(out_format="mxfp8"),
               dict(act="swiglu", up=mu, bias=x[0, :I]),
               dict(act="swiglu", up=mu, residual=x[:, :I])):
        with pytest.raises(ValueError):
            ops.linear_mx_a8(xq, mg, **kw)
