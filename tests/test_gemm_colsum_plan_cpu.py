"""Workspace sizing of the hand GEMM with and without column sums
(gemm_ws_floats in ops/csrc/gemm_plan.h, the only place that knows it),
against values worked out by hand, and the refusal of a column-sum request
wherever the plan is not the 256 kernel on two k-outer operands. Host code
only: needs the built extension but no GPU."""

import pytest

try:
    from tepdist_amd.ops import _tepdist_hip as ext
except ImportError:
    ext = None

pytestmark = pytest.mark.skipif(ext is None, reason="HIP extension not built")


def ws_ko(M, N, K, colsum, lda=None, ldb=None):
    return ext.gemm_ws_floats(M, N, K, M if lda is None else lda,
                              N if ldb is None else ldb, False, False, 0, 1,
                              colsum)


def test_split_plan_one_n_tile():
    M, N, K = 256, 256, 2048
    assert ext.gemm_plan(M, N, K, M, N, False, False, 0, 1)[:3] == \
        (256, 16, 128)
    assert ws_ko(M, N, K, False) == 16 * 65536
    # 16 chunks x 1 n-tile parts of 256 floats after the product partials
    assert ws_ko(M, N, K, True) == 16 * 65536 + 16 * 1 * 256


def test_unsplit_plan():
    M, N, K = 512, 512, 320
    assert ext.gemm_plan(M, N, K, M, N, False, False, 0, 1)[:3] == \
        (256, 1, 0)
    assert ws_ko(M, N, K, False) == 0
    assert ws_ko(M, N, K, True) == 2 * 512      # 2 n-tiles x M


def test_flagship_out_wgrad():
    M, N, K = 1024, 4096, 65536
    kernel, split_k, _, _ = ext.gemm_plan(M, N, K, M, N, False, False, 0, 1)
    assert (kernel, split_k) == (256, 8)
    assert ws_ko(M, N, K, False) == split_k * M * N
    assert ws_ko(M, N, K, True) == split_k * M * N + split_k * 16 * 1024


def test_canonical_sizes_are_unchanged():
    # k-contiguous calls: split_k * M * N or nothing, as _gemm_raw computed
    for (M, N, K) in [(256, 256, 2048), (512, 512, 320), (100, 60, 4096),
                      (1024, 1024, 1024)]:
        split_k = ext.gemm_plan(M, N, K, K, K, True, True, 0, 1)[1]
        want = split_k * M * N if split_k > 1 else 0
        assert ext.gemm_ws_floats(M, N, K, K, K, True, True, 0, 1,
                                  False) == want


@pytest.mark.parametrize("args", [
    # two k-contiguous operands, 256 kernel
    (512, 512, 320, 320, 320, True, True, 0, 1),
    # mixed layouts
    (512, 512, 320, 512, 320, False, True, 0, 1),
    # two k-outer operands that the plan gives the 128 kernel: partial
    # tiles, unaligned rows, a single K-tile
    (128, 128, 2048, 128, 128, False, False, 0, 1),
    (256, 256, 192, 260, 256, False, False, 0, 1),
    (256, 256, 64, 256, 256, False, False, 0, 1),
    # batched
    (256, 256, 128, 256, 256, False, False, 0, 2),
])
def test_colsum_refused(args):
    assert ext.gemm_ws_floats(*args, False) >= 0    # sized without colsum
    with pytest.raises(RuntimeError, match="colsum_out needs the 256 kernel"):
        ext.gemm_ws_floats(*args, True)
