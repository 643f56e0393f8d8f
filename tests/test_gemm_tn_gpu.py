"""The 256-tile GEMM on two k-outer operands (A stored [K][M], B stored
[K][N], wgrad's layout) read in place through transposed LDS fragment reads:
an exact check of the fragment maps, fp32 references over the tile-count
edges, split-K, the fallbacks, and the call sites that use it."""

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


def _assert_close_bf16(ours, ref32, atol=2e-2, rtol=2e-2, scale=None):
    """Compare a bf16 kernel output against an fp32 reference with a
    tolerance scaled to the reference magnitude."""
    ours32 = ours.float()
    err = (ours32 - ref32).abs()
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


def _plan_ko(M, N, K, lda, ldb, batch=1):
    return hip.ext.gemm_plan(M, N, K, lda, ldb, False, False, 0, batch)[:3]


def _tn(a_st, b_st):
    """C[M,N] = a_st^T @ b_st for a_st [K, M], b_st [K, N] as they lie."""
    c = hip.matmul(a_st.t(), b_st)
    torch.cuda.synchronize()
    return c


@pytest.mark.usefixtures("hand_gemm")
def test_tn_identity_a_is_exact():
    # A = I: C[m][n] = B[m][n], every product exact and every other term
    # zero, so any k-order mismatch between the operands or any m/n
    # fragment-map error shows as a wrong element. No tolerance.
    M, N, K = 256, 512, 256
    assert _plan_ko(M, N, K, M, N) == (256, 1, 0)
    a_st = torch.eye(K, M, dtype=BF16, device="cuda")
    b_st = _randn(K, N, seed=51)
    assert torch.equal(_tn(a_st, b_st), b_st)


@pytest.mark.usefixtures("hand_gemm")
def test_tn_identity_b_is_exact():
    M, N, K = 512, 256, 256
    assert _plan_ko(M, N, K, M, N) == (256, 1, 0)
    a_st = _randn(K, M, seed=52)
    b_st = torch.eye(K, N, dtype=BF16, device="cuda")
    assert torch.equal(_tn(a_st, b_st), a_st.t())


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", [
    (256, 256, 128),    # two K-tiles, the minimum
    (512, 256, 192),    # odd tile count, M != N
    (256, 512, 320)])   # five tiles: the slot cycle wraps
def test_tn_against_fp32(M, N, K):
    assert _plan_ko(M, N, K, M, N) == (256, 1, 0)
    a_st = _randn(K, M, seed=53)
    b_st = _randn(K, N, seed=54)
    _assert_close_bf16(_tn(a_st, b_st), a_st.float().t() @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_tn_column_slices_of_wider_tensors():
    # ld > F: both operands are column slices, 16-byte rows and offsets
    M, N, K = 256, 256, 192
    a_w = _randn(K, M + 72, seed=55)
    b_w = _randn(K, N + 256, seed=56)
    a_st, b_st = a_w[:, 8:8 + M], b_w[:, 128:128 + N]
    assert _plan_ko(M, N, K, a_w.shape[1], b_w.shape[1]) == (256, 1, 0)
    _assert_close_bf16(_tn(a_st, b_st), a_st.float().t() @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_tn_batched():
    B, M, N, K = 2, 256, 256, 128
    assert _plan_ko(M, N, K, M, N, batch=B) == (256, 1, 0)
    a_st = _randn(B, K, M, seed=57)
    b_st = _randn(B, K, N, seed=58)
    c = hip.matmul(a_st.transpose(1, 2), b_st)
    torch.cuda.synchronize()
    _assert_close_bf16(c, a_st.float().transpose(1, 2) @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_tn_splitk():
    M, N, K = 256, 256, 2048
    assert _plan_ko(M, N, K, M, N) == (256, 16, 128)
    a_st = _randn(K, M, seed=59)
    b_st = _randn(K, N, seed=60)
    _assert_close_bf16(_tn(a_st, b_st), a_st.float().t() @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_tn_unaligned_rows_fall_back_to_128():
    M, N, K = 256, 256, 192
    a_w = _randn(K, M + 4, seed=61)
    a_st, b_st = a_w[:, :M], _randn(K, N, seed=62)
    assert _plan_ko(M, N, K, M + 4, N) == (128, 1, 0)
    _assert_close_bf16(_tn(a_st, b_st), a_st.float().t() @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_tn_partial_tiles_stay_on_128():
    M, N, K = 128, 128, 2048
    assert _plan_ko(M, N, K, M, N) == (128, 16, 128)
    a_st = _randn(K, M, seed=63)
    b_st = _randn(K, N, seed=64)
    _assert_close_bf16(_tn(a_st, b_st), a_st.float().t() @ b_st.float(),
                       rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_linear_bwd_wgrad_in_place(act):
    T, N, K = 192, 256, 256      # tokens, out features, in features
    assert _plan_ko(N, K, T, N, K) == (256, 1, 0)
    x = _randn(T, K, seed=65)
    w = _randn(N, K, seed=66)
    dy = _randn(T, N, seed=67)
    pre = _randn(T, N, seed=68) if act == "gelu" else None
    dx, dw, db = hip.linear_bwd(dy, x, w, True, act, pre)
    torch.cuda.synchronize()
    dy32 = dy.float()
    if act == "gelu":
        p32 = pre.float().requires_grad_(True)
        torch.nn.functional.gelu(p32, approximate="tanh").backward(dy32)
        dy32 = p32.grad
    _assert_close_bf16(dx, dy32 @ w.float(), rtol=3e-2, scale=math.sqrt(N))
    _assert_close_bf16(dw, dy32.t() @ x.float(), rtol=3e-2,
                       scale=math.sqrt(T))
    _assert_close_bf16(db, dy32.sum(0), rtol=3e-2, scale=math.sqrt(T))


@pytest.mark.usefixtures("hand_gemm")
def test_matmul_dy_t_x():
    T, N, K = 192, 256, 256
    assert _plan_ko(N, K, T, N, K) == (256, 1, 0)
    dy = _randn(T, N, seed=69)
    x = _randn(T, K, seed=70)
    dw = hip.matmul(dy.t(), x)
    torch.cuda.synchronize()
    _assert_close_bf16(dw, dy.float().t() @ x.float(), rtol=3e-2,
                       scale=math.sqrt(T))
