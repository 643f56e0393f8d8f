"""The hand GEMM's host-side planner (ops/csrc/gemm_plan.h, bound as
ext.gemm_plan): fixed plans for representative calls, and invariants over a
canonical and a non-canonical grid. The planner is pure host code, so this
needs the built extension but no GPU."""

import itertools

import pytest

try:
    from tepdist_amd.ops import _tepdist_hip as ext
except ImportError:
    ext = None

pytestmark = pytest.mark.skipif(ext is None, reason="HIP extension not built")


def plan(M, N, K, lda=None, ldb=None, a_kc=True, b_kc=True, epi=0, batch=1):
    return ext.gemm_plan(M, N, K, K if lda is None else lda,
                         K if ldb is None else ldb, a_kc, b_kc, epi, batch)


# (M, N, K, other arguments) -> (kernel, split_k, k_chunk)
PLANS = [
    ((256, 256, 2048, {}), (256, 16, 128)),
    ((256, 256, 2176, {}), (128, 12, 192)),
    ((256, 256, 1984, {}), (256, 1, 0)),
    ((256, 256, 128, {}), (256, 1, 0)),
    ((256, 256, 64, {}), (128, 1, 0)),
    ((512, 256, 8192, {}), (256, 16, 512)),
    ((3072, 768, 2048, {}), (256, 11, 192)),
    ((2304, 768, 2048, {}), (256, 16, 128)),
    ((4096, 4096, 4096, {}), (256, 2, 2048)),
    ((5120, 5120, 4096, {}), (256, 1, 0)),
    ((256, 256, 4096, dict(lda=4100)), (128, 16, 256)),
    ((256, 256, 4096, dict(a_kc=False, lda=256)), (128, 16, 256)),
    ((200, 136, 4096, dict(b_kc=False, ldb=136)), (128, 16, 256)),
    ((128, 128, 2048, {}), (128, 16, 128)),
    ((120, 136, 2056, {}), (128, 17, 128)),
    ((123, 125, 18440, {}), (128, 17, 1088)),
    ((256, 256, 4096, dict(epi=1)), (256, 1, 0)),
    ((256, 256, 4096, dict(batch=2)), (256, 1, 0)),
]


@pytest.mark.parametrize("call,want", PLANS)
def test_plan_table(call, want):
    M, N, K, kw = call
    kernel, split_k, k_chunk, why_not = plan(M, N, K, **kw)
    assert (kernel, split_k, k_chunk) == want
    assert why_not == ""


def test_plan_dgelu_needs_the_256_kernel():
    assert plan(512, 256, 128, epi=4)[0] == 256
    for M, N, K in [(500, 256, 128), (512, 256, 64)]:
        kernel, split_k, k_chunk, why_not = plan(M, N, K, epi=4)
        assert kernel == 0 and why_not
        assert (split_k, k_chunk) == (1, 0)


def _check(M, N, K, kw, max_split):
    kernel, s, kc, why_not = p = plan(M, N, K, **kw)
    ctx = (M, N, K, kw, p)
    assert kernel in (128, 256) and why_not == "", ctx
    if s == 1:
        assert kc == 0, ctx
    else:
        assert kw.get("epi", 0) == 0 and kw.get("batch", 1) == 1, ctx
        assert 2 <= s <= max_split, ctx
        assert kc % 64 == 0, ctx
        assert (s - 1) * kc < K <= s * kc, ctx      # no empty chunk
    if kernel == 256:
        assert K >= 128, ctx
        if s > 1:
            assert kc >= 128 and K - (s - 1) * kc >= 128, ctx
    return s


def test_plan_invariants_canonical_grid():
    # M, N multiples of 256 up to 23 x 23 tiles, K = 2048 .. 65536 in steps
    # of 64, thinned: every 3rd K per (M, N) with a shifting start
    tiles = range(1, 24)
    n_split = 0
    for i, (mt, nt) in enumerate(itertools.product(tiles, tiles)):
        for K in range(2048 + 64 * (i % 3), 65536 + 1, 64 * 3):
            n_split += _check(256 * mt, 256 * nt, K, {}, 16) > 1
    assert n_split > 100000     # the grid does exercise the split plans


def test_plan_invariants_noncanonical_grid():
    # M = 128 i - 5, N = 128 j - 3, K = 2048 .. 20000 in steps of 8 plus a
    # few odd K, thinned: every 5th K per (M, N) with a shifting start
    tiles = range(1, 20)
    seen17 = 0
    for i, (mt, nt) in enumerate(itertools.product(tiles, tiles)):
        ks = list(range(2048 + 8 * (i % 5), 20000, 8 * 5))
        for K in ks + [2049, 2051, 2056, 4097, 5001, 18440]:
            seen17 += _check(128 * mt - 5, 128 * nt - 3, K, {}, 17) == 17
    assert seen17 > 0           # the 17-chunk plans are on the grid


def test_plan_never_splits_epilogues_or_batches():
    for (M, N), K in itertools.product([(256, 256), (120, 136), (768, 512)],
                                       [2048, 2056, 4096, 16384]):
        for kw in [dict(epi=1), dict(epi=2), dict(epi=3), dict(batch=2),
                   dict(batch=6, epi=1)]:
            assert _check(M, N, K, kw, 17) == 1, (M, N, K, kw)
