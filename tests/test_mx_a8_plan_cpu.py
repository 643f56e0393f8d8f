"""csrc/mx_gemm_a8_plan.h on the host: the plan through ext.mx_gemm_a8_plan,
the activation quantizer's integer rule (the lines the kernel runs) through
ext.mx_act_quant_block against mx.mx_quantize, and the reference ops."""

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.ops import _tepdist_hip as ext
from tepdist_amd.ops import mx

BF16 = torch.bfloat16


def _plan(M=128, N=256, K=384, bits=4, ldc=None, lds=None, ldxc=None,
          ldxs=None, epi=0, tile=0):
    return ext.mx_gemm_a8_plan(
        M, N, K, bits, K * bits // 8 if ldc is None else ldc,
        K // 32 if lds is None else lds, K if ldxc is None else ldxc,
        K // 32 if ldxs is None else ldxs, epi, tile)


@pytest.mark.parametrize("M,N,K,tile,blocks", [
    (1024, 4096, 2048, 128, 256), (1024, 3968, 2048, 64, 16 * 62),
    (129, 503, 1152, 64, 3 * 8), (1, 1, 128, 64, 1)])
def test_tile_rule_and_override(M, N, K, tile, blocks):
    assert _plan(M, N, K, 8) == (tile, 3, blocks, "")
    assert _plan(M, N, K, 4, tile=192 - tile)[0] == 192 - tile


@pytest.mark.parametrize("kw,why", [
    (dict(K=192), "multiple of 128"), (dict(bits=6), "bits must be"),
    (dict(epi=5), "epi must be 0..4"), (dict(tile=32), "tile must be"),
    (dict(ldc=200), "code rows must be 16-byte aligned"),
    (dict(lds=14), "scale rows must be 4-byte aligned"),
    (dict(ldxc=392), "activation code rows must be 16-byte aligned"),
    (dict(ldxc=256), "activation code rows must be 16-byte aligned"),
    (dict(ldxs=13), "activation scale rows must be 4-byte aligned")])
def test_refusals(kw, why):
    p = _plan(**kw)
    assert p[:3] == (0, 0, 0) and why in p[3], p
    assert _plan(ldxc=400, ldxs=16)[3] == ""


def test_quantizer_rule_every_finite_bf16():
    """All 65 280 finite patterns in bit order as [510, 128]: ties,
    saturation, subnormals, zero blocks and both scale clamps."""
    pat = torch.arange(1 << 16, dtype=torch.int32)
    pat = pat[(pat & 0x7f80) != 0x7f80].reshape(510, 128)
    want = mx.mx_quantize(pat.to(torch.int16).view(BF16), "mxfp8")
    assert {10, 127, 246} <= set(want.scales.unique().tolist())
    for r, row in enumerate(pat.reshape(-1, 32).tolist()):
        byte, codes = ext.mx_act_quant_block(row)
        assert byte == int(want.scales.reshape(-1)[r]), (r, byte)
        assert codes == want.codes.reshape(-1, 32)[r].tolist(), r


def test_reference_ops():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 256, generator=g).to(BF16)
    mw = ops.mx_quantize(torch.randn(40, 256, generator=g), "mxfp4")
    b = torch.randn(40, generator=g).to(BF16)
    q = ops.mx_quantize_act(x)
    assert q.shape == (15, 256) and q.fmt == "mxfp8"
    xr = ops.mx_quantize_act(x, roundtrip=True)
    assert torch.equal(xr, mx.dequantize_ref(q).reshape(x.shape))
    want = ops.linear_mx(xr, mw, b, "gelu")
    assert torch.equal(ops.linear_mx_a8(x, mw, b, "gelu"), want)
    assert torch.equal(ops.linear_mx_a8(q, mw, b, "gelu"),
                       want.reshape(15, 40))
