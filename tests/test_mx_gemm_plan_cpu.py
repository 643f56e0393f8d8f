"""csrc/mx_gemm_plan.h through ext.mx_gemm_plan: the tile every shape gets,
the refusals and the override. Host only."""

import pytest

from tepdist_amd.ops import _tepdist_hip as ext


def _plan(M, N, K, bits=4, ldc=None, lds=None, epi=0, tile=0):
    ldc = K * bits // 8 if ldc is None else ldc
    lds = K // 32 if lds is None else lds
    return ext.mx_gemm_plan(M, N, K, bits, ldc, lds, epi, tile)


# (M, N, K) -> tile, blocks: 128 where its grid has at least 256 blocks
@pytest.mark.parametrize("M,N,K,tile,blocks", [
    (128, 3072, 2048, 64, 2 * 48),        # batch decode: 24 blocks at 128
    (512, 3072, 2048, 64, 8 * 48),        # 96 blocks at 128
    (1024, 4096, 2048, 128, 8 * 32),      # exactly 256
    (1024, 3968, 2048, 64, 16 * 62),      # 248 at 128
    (2048, 2048, 8192, 128, 256),
    (65, 128256, 2048, 128, 1002),        # a head: N alone fills the chip
    (1, 1, 128, 64, 1),
    (129, 503, 1152, 64, 3 * 8),          # ragged both ways
])
@pytest.mark.parametrize("bits", [4, 8])
def test_tile_rule(M, N, K, tile, blocks, bits):
    assert _plan(M, N, K, bits) == (tile, 3, blocks, "")


@pytest.mark.parametrize("tile,blocks", [(64, 3 * 8), (128, 2 * 4)])
def test_override(tile, blocks):
    assert _plan(129, 503, 1152, tile=tile) == (tile, 3, blocks, "")
    assert _plan(4096, 4096, 128, tile=tile)[0] == tile


@pytest.mark.parametrize("kw,why", [
    (dict(K=192), "multiple of 128"),
    (dict(K=0), "multiple of 128"),
    (dict(M=0), "positive"),
    (dict(bits=6), "bits must be"),
    (dict(epi=5), "epi must be 0..4"),
    (dict(epi=-1), "epi must be 0..4"),
    (dict(tile=32), "tile must be"),
    (dict(bits=4, ldc=200), "code rows must be 16-byte aligned"),
    (dict(bits=8, ldc=256), "code rows must be 16-byte aligned"),
    (dict(lds=14), "scale rows must be 4-byte aligned"),
    (dict(lds=8), "scale rows must be 4-byte aligned"),
])
def test_refusals(kw, why):
    args = dict(M=128, N=256, K=384)
    args.update(kw)
    p = _plan(**args)
    assert p[:3] == (0, 0, 0) and why in p[3], p


def test_padded_rows_are_covered():
    assert _plan(128, 256, 384, bits=4, ldc=208, lds=16)[3] == ""
