"""Column sums of the k-outer A operand (wgrad's bias gradient) formed
inside the 256-tile GEMM: exact integer sums over the tile-count, split-K
and n-tile sharing edges, which element is counted where, a rounding bound
on random data, bit-identical repeats, and the call sites that use it."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tepdist_amd.ops import hip

BF16 = torch.bfloat16


def _randn(*shape, seed=0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def _assert_close_bf16(ours, ref32, rtol=2e-2, scale=None):
    """Compare a bf16 kernel output against an fp32 reference with a
    tolerance scaled to the reference magnitude."""
    err = (ours.float() - ref32).abs()
    denom = scale if scale is not None else ref32.abs().max().clamp_min(1.0)
    rel = (err / denom).max().item()
    assert rel < rtol, f"max scaled err {rel} (atol ref {err.max().item()})"


@pytest.fixture
def hand_gemm():
    """Pin the GEMM sites to the hand kernels (in "auto" mode the faster of
    the hand kernel and hipBLASLt answers)."""
    old = hip._GEMM_BACKEND
    hip._GEMM_BACKEND = "hip"
    yield
    hip._GEMM_BACKEND = old


def _plan_ko(M, N, K, lda, ldb):
    return hip.ext.gemm_plan(M, N, K, lda, ldb, False, False, 0, 1)[:3]


def _tn(a_st, b_st, colsum=True):
    """(a_st^T @ b_st, column sums of a_st or None) for a_st [K, M] and
    b_st [K, N] as they lie, in one hand call."""
    K, M = a_st.shape
    N = b_st.shape[1]
    db = torch.empty(M, dtype=BF16, device="cuda") if colsum else None
    c = hip._gemm_raw(a_st, b_st, False, False, M, N, K, a_st.stride(0),
                      b_st.stride(0), 0, 0, 1, colsum_out=db)[0]
    torch.cuda.synchronize()
    return c, db


def _ints(K, M, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (K, M), generator=g)


# (K, M, N, seed) -> plan
EXACT = [
    ((128, 256, 256, 81), (256, 1, 0)),      # two K-tiles, the minimum
    ((320, 512, 256, 82), (256, 1, 0)),      # five tiles, two m-tiles
    ((2048, 256, 256, 83), (256, 16, 128)),  # split-K 16
    ((2048, 512, 512, 84), (256, 16, 128)),  # split-K, two n-tiles share A
]


@pytest.mark.parametrize("case,plan", EXACT)
def test_colsum_integers_are_exact(case, plan):
    # entries in {-1, 0, 1}: every partial sum is a small integer, exact in
    # fp32 and (|sum| <= 117 < 256) in bf16. No tolerance.
    K, M, N, seed = case
    assert _plan_ko(M, N, K, M, N) == plan
    a64 = _ints(K, M, seed)
    want = a64.sum(0)
    assert want.abs().max().item() <= 117
    a_st = a64.to(BF16).cuda()
    b_st = _randn(K, N, seed=seed + 100)
    c, db = _tn(a_st, b_st)
    assert torch.equal(db.cpu().to(torch.int64), want)
    # the product is the one the kernel gives without the column sums
    assert torch.equal(c, _tn(a_st, b_st, colsum=False)[0])


# (K, M, N): unsplit one and two n-tiles, split one and two n-tiles
WHICH = [(256, 256, 256), (512, 256, 512), (2048, 256, 256),
         (2048, 512, 512)]


@pytest.mark.parametrize("K,M,N", WHICH)
def test_colsum_counts_each_row_once(K, M, N):
    assert _plan_ko(M, N, K, M, N)[0] == 256
    b_st = _randn(K, N, seed=85)
    # one 1.0 per row r, at column r % M: every column sums to K / M
    a_st = torch.zeros(K, M, dtype=BF16, device="cuda")
    r = torch.arange(K, device="cuda")
    a_st[r, r % M] = 1.0
    db = _tn(a_st, b_st)[1]
    assert torch.equal(db.float(), torch.full((M,), float(K // M),
                                              device="cuda"))
    # a single nonzero row in the last K-tile of the last chunk, a distinct
    # small integer per column: counted once, in its own column
    a_st = torch.zeros(K, M, dtype=BF16, device="cuda")
    row = (torch.arange(M, device="cuda") % 7 + 1).to(BF16)
    a_st[K - 3] = row
    db = _tn(a_st, b_st)[1]
    assert torch.equal(db, row)


@pytest.mark.parametrize("K,M", [(320, 512), (2048, 256)])
def test_colsum_random_within_rounding(K, M):
    N = 256
    assert _plan_ko(M, N, K, M, N)[0] == 256
    a_st = _randn(K, M, seed=86)
    b_st = _randn(K, N, seed=87)
    db = _tn(a_st, b_st)[1]
    a64 = a_st.double()
    s64 = a64.sum(0)
    # one bf16 rounding of the result + fp32 accumulation in any order
    bound = 2.0 ** -8 * s64.abs() + K * 2.0 ** -23 * a64.abs().sum(0)
    err = (db.double() - s64).abs()
    print(f"colsum K={K} M={M}: max err/bound "
          f"{(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    # no atomics: the same bits on every call
    c2, db2 = _tn(a_st, b_st)
    assert torch.equal(db2, db)
    assert torch.equal(c2, _tn(a_st, b_st)[0])


def test_colsum_column_slices_of_wider_tensors():
    # ld > F: both operands are column slices, 16-byte rows and offsets
    M, N, K = 256, 256, 192
    a_w = _ints(K, M + 72, 88).to(BF16).cuda()
    b_w = _randn(K, N + 256, seed=89)
    a_st, b_st = a_w[:, 8:8 + M], b_w[:, 128:128 + N]
    assert _plan_ko(M, N, K, a_w.shape[1], b_w.shape[1]) == (256, 1, 0)
    c, db = _tn(a_st, b_st)
    assert torch.equal(db.float(), a_st.float().sum(0))
    _assert_close_bf16(c, a_st.float().t() @ b_st.float(), rtol=3e-2,
                       scale=math.sqrt(K))


def test_colsum_refused_off_the_256_k_outer_plan():
    M, N, K = 256, 256, 128
    a = _randn(M, K, seed=90)
    b = _randn(N, K, seed=91)
    db = torch.empty(M, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="colsum_out needs the 256 kernel"):
        hip._gemm_raw(a, b, True, True, M, N, K, K, K, 0, 0, 1,
                      colsum_out=db)


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_linear_bwd_fused_bias_grad(act, has_bias):
    T, N, K = 192, 256, 256      # tokens, out features, in features
    assert _plan_ko(N, K, T, N, K) == (256, 1, 0)
    x = _randn(T, K, seed=92)
    w = _randn(N, K, seed=93)
    dy = _randn(T, N, seed=94)
    pre = _randn(T, N, seed=95) if act == "gelu" else None
    dx, dw, db = hip.linear_bwd(dy, x, w, has_bias, act, pre)
    torch.cuda.synchronize()
    dy32 = dy.float()
    if act == "gelu":
        p32 = pre.float().requires_grad_(True)
        torch.nn.functional.gelu(p32, approximate="tanh").backward(dy32)
        dy32 = p32.grad
    _assert_close_bf16(dx, dy32 @ w.float(), rtol=3e-2, scale=math.sqrt(N))
    _assert_close_bf16(dw, dy32.t() @ x.float(), rtol=3e-2,
                       scale=math.sqrt(T))
    if has_bias:
        _assert_close_bf16(db, dy32.sum(0), rtol=3e-2, scale=math.sqrt(T))
    else:
        assert db is None


@pytest.mark.usefixtures("hand_gemm")
def test_mlp_bwd_fused_bias_grad():
    # hand dgelu backward: dw2 and db2 come from one wgrad call
    T, d, hid = 256, 256, 512
    assert _plan_ko(d, hid, T, d, hid) == (256, 1, 0)
    x = _randn(T, d, seed=96) * 0.5
    w1, b1 = _randn(hid, d, seed=97) * 0.05, _randn(hid, seed=98) * 0.05
    w2, b2 = _randn(d, hid, seed=99) * 0.05, _randn(d, seed=100) * 0.05
    dy = _randn(T, d, seed=101)
    old = hip._MLP_FUSED
    hip._MLP_FUSED = "0"
    try:
        _, (h, pre) = hip.mlp_fwd(x, w1, b1, w2, b2)
        dx, dw1, db1, dw2, db2 = hip.mlp_bwd(dy, x, w1, w2, h, pre)
        torch.cuda.synchronize()
    finally:
        hip._MLP_FUSED = old
    xf, w1f, b1f, w2f, b2f = (t.float().clone().requires_grad_()
                              for t in (x, w1, b1, w2, b2))
    hf = torch.nn.functional.gelu(xf @ w1f.t() + b1f, approximate="tanh")
    (hf @ w2f.t() + b2f).backward(dy.float())
    for got, want, name in ((dx, xf.grad, "dx"), (dw1, w1f.grad, "dw1"),
                            (db1, b1f.grad, "db1"), (dw2, w2f.grad, "dw2"),
                            (db2, b2f.grad, "db2")):
        torch.testing.assert_close(got.float(), want, rtol=5e-2, atol=5e-2,
                                   msg=name)
    # db2 is the column sum of dy, to one bf16 rounding of the fp32 sum
    s64 = dy.double().sum(0)
    bound = 2.0 ** -8 * s64.abs() + T * 2.0 ** -23 * dy.double().abs().sum(0)
    assert bool(((db2.double() - s64).abs() <= bound).all())
