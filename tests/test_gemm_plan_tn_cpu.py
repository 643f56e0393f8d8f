"""Planner (ops/csrc/gemm_plan.h) for two k-outer operands, wgrad's layout
(A stored [K][M], B stored [K][N]): a pinned table, the invariants of
test_gemm_plan_cpu.py over a k-outer grid, and a sample of canonical, mixed
and non-qualifying k-outer calls whose plans must be what they were before
the 256 kernel learnt this layout. Host code only: needs the built
extension but no GPU."""

import itertools

import pytest

try:
    from tepdist_amd.ops import _tepdist_hip as ext
except ImportError:
    ext = None

pytestmark = pytest.mark.skipif(ext is None, reason="HIP extension not built")


def plan_ko(M, N, K, lda=None, ldb=None, epi=0, batch=1):
    return ext.gemm_plan(M, N, K, M if lda is None else lda,
                         N if ldb is None else ldb, False, False, epi, batch)


# (M, N, K) -> (kernel, split_k, k_chunk): block count, split trigger and
# split count of the canonical case at the same shape
KO_PLANS = [
    ((256, 256, 128), (256, 1, 0)),
    ((512, 256, 192), (256, 1, 0)),
    ((256, 512, 320), (256, 1, 0)),
    ((256, 256, 1984), (256, 1, 0)),
    ((256, 256, 2048), (256, 16, 128)),
    ((512, 256, 8192), (256, 16, 512)),
    ((768, 768, 2048), (256, 16, 128)),
    ((3072, 768, 2048), (256, 11, 192)),
    ((4096, 4096, 4096), (256, 2, 2048)),
    ((5120, 5120, 4096), (256, 1, 0)),
    # the flagship wgrads: proj, qkv, fc, out at 65536 tokens
    ((1024, 1024, 65536), (256, 16, 4096)),
    ((3072, 1024, 65536), (256, 16, 4096)),
    ((4096, 1024, 65536), (256, 8, 8192)),
    ((1024, 4096, 65536), (256, 8, 8192)),
]


@pytest.mark.parametrize("shape,want", KO_PLANS)
def test_ko_plan_table(shape, want):
    kernel, split_k, k_chunk, why_not = plan_ko(*shape)
    assert (kernel, split_k, k_chunk) == want
    assert why_not == ""
    # same as the canonical plan of the shape
    M, N, K = shape
    assert ext.gemm_plan(M, N, K, K, K, True, True, 0, 1)[:3] == want


def test_ko_plan_wider_rows_and_batches():
    # column slices of wider tensors: any ld that keeps 16-byte rows
    assert plan_ko(256, 256, 2048, lda=264, ldb=512)[:3] == (256, 16, 128)
    assert plan_ko(256, 256, 128, batch=2)[:3] == (256, 1, 0)
    assert plan_ko(256, 256, 4096, batch=2)[:3] == (256, 1, 0)


def _check(M, N, K, max_split):
    kernel, s, kc, why_not = p = plan_ko(M, N, K)
    ctx = (M, N, K, p)
    assert kernel in (128, 256) and why_not == "", ctx
    if s == 1:
        assert kc == 0, ctx
    else:
        assert 2 <= s <= max_split, ctx
        assert kc % 64 == 0, ctx
        assert (s - 1) * kc < K <= s * kc, ctx      # no empty chunk
    if kernel == 256:
        assert K >= 128, ctx
        if s > 1:
            assert kc >= 128 and K - (s - 1) * kc >= 128, ctx
    return kernel, s


def test_ko_plan_invariants_grid():
    # M, N multiples of 256 up to 17 x 17 tiles, K = 64 .. 65536 in steps of
    # 64, thinned: every 5th K per (M, N) with a shifting start
    tiles = range(1, 18)
    n256 = n_split = n128 = 0
    for i, (mt, nt) in enumerate(itertools.product(tiles, tiles)):
        for K in range(64 + 64 * (i % 5), 65536 + 1, 64 * 5):
            kernel, s = _check(256 * mt, 256 * nt, K, 16)
            n256 += kernel == 256
            n128 += kernel == 128
            n_split += kernel == 256 and s > 1
            if kernel == 256:   # then it is the canonical call's plan
                assert plan_ko(256 * mt, 256 * nt, K)[:3] == ext.gemm_plan(
                    256 * mt, 256 * nt, K, K, K, True, True, 0, 1)[:3]
    assert n_split > 10000 and n256 > n128 > 0


# (M, N, K, lda, ldb, a_kc, b_kc, epi, batch) -> plan, as returned by the
# build of the commit before the k-outer path
UNCHANGED = [
    # canonical
    ((256, 256, 2048, 2048, 2048, True, True, 0, 1), (256, 16, 128)),
    ((256, 256, 2176, 2176, 2176, True, True, 0, 1), (128, 12, 192)),
    ((1024, 1024, 65536, 65536, 65536, True, True, 0, 1), (256, 16, 4096)),
    ((3072, 1024, 65536, 65536, 65536, True, True, 0, 1), (256, 16, 4096)),
    ((4096, 1024, 65536, 65536, 65536, True, True, 0, 1), (256, 8, 8192)),
    ((65536, 1024, 1024, 1024, 1024, True, True, 1, 1), (256, 1, 0)),
    ((65536, 4096, 1024, 1024, 1024, True, True, 2, 1), (256, 1, 0)),
    ((65536, 1024, 4096, 4096, 4096, True, True, 4, 1), (256, 1, 0)),
    ((512, 256, 128, 128, 128, True, True, 0, 4), (256, 1, 0)),
    ((256, 256, 4096, 4100, 4096, True, True, 0, 1), (128, 16, 256)),
    ((200, 136, 4096, 4096, 4096, True, True, 0, 1), (128, 16, 256)),
    # mixed layouts stay on the 128 kernel
    ((256, 256, 4096, 256, 4096, False, True, 0, 1), (128, 16, 256)),
    ((256, 256, 4096, 4096, 256, True, False, 0, 1), (128, 16, 256)),
    ((65536, 1024, 1024, 1024, 1024, True, False, 0, 1), (128, 1, 0)),
    ((1024, 1024, 65536, 1024, 65536, False, True, 0, 1), (128, 8, 8192)),
    ((512, 512, 128, 512, 128, False, True, 0, 1), (128, 1, 0)),
    ((200, 136, 4096, 4096, 136, True, False, 0, 1), (128, 16, 256)),
    ((256, 256, 4096, 256, 4096, False, True, 1, 1), (128, 1, 0)),
    # k-outer calls that miss one of the 256 kernel's conditions: partial
    # tiles, unaligned rows, one K-tile, a one-tile last chunk, an
    # epilogue, K no multiple of 64
    ((128, 128, 2048, 128, 128, False, False, 0, 1), (128, 16, 128)),
    ((200, 136, 4096, 200, 136, False, False, 0, 1), (128, 16, 256)),
    ((256, 256, 4096, 260, 256, False, False, 0, 1), (128, 16, 256)),
    ((256, 256, 4096, 256, 260, False, False, 0, 1), (128, 16, 256)),
    ((256, 256, 64, 256, 256, False, False, 0, 1), (128, 1, 0)),
    ((256, 256, 2176, 256, 256, False, False, 0, 1), (128, 12, 192)),
    ((256, 256, 4096, 256, 256, False, False, 1, 1), (128, 1, 0)),
    ((96, 144, 80, 96, 144, False, False, 0, 6), (128, 1, 0)),
    ((256, 384, 2048, 256, 384, False, False, 0, 1), (128, 16, 128)),
    ((256, 256, 2056, 256, 256, False, False, 0, 1), (128, 17, 128)),
]


@pytest.mark.parametrize("call,want", UNCHANGED)
def test_other_plans_unchanged(call, want):
    kernel, split_k, k_chunk, why_not = ext.gemm_plan(*call)
    assert (kernel, split_k, k_chunk) == want
    assert why_not == ""
