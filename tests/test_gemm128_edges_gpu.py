"""The 128-tile GEMM (ops/csrc/gemm.hip) at the edges of each of its data
paths, against exact and per-element float64 oracles.

The kernel runs every hand GEMM call the planner does not give the 256
kernel: partial tiles, K tails, mixed layouts, unaligned leading dimensions,
batches, and every split-K plan of such a shape. Cases, inputs and the three
criteria (integer-exact, selection-exact, 1 ulp + K * 2^-23 * |a| @ |b| per
element) are in tests/gemm_checks.py; tests/test_gemm_oracle_cpu.py proves on
the CPU that a correct implementation passes them and that eight kinds of
wrong ones do not. Here the same checks drive the kernel through
hip._gemm_raw, where no library can take the call, and the callers that map
torch views to layout flags through hip.matmul / hip.linear_fwd pinned to the
hand path.

The unmarked plan test keeps every case on the kernel (and split) it is here
for, so a planner change cannot empty this file silently."""

import pytest
import torch

import gemm_checks as gc
from tepdist_amd.ops import _tepdist_hip as ext

if torch.cuda.is_available():
    from tepdist_amd.ops import hip

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
_ids = dict(ids=lambda c: c.name)


@pytest.mark.parametrize("case", gc.ALL_CASES, **_ids)
def test_plan_keeps_the_case_on_its_kernel(case):
    gc.check_plan(ext, case)


def test_plan_split_cases_reach_the_short_last_chunk_and_scalar_tail():
    c = gc.BY_NAME["split-130x67x2056-kc,kc"]
    s, chunk = c.split
    assert c.K - (s - 1) * chunk == 8 and (c.M * c.N) % 4 == 2


def test_dgelu_is_still_refused_off_the_256_kernel():
    kernel, _, _, why = ext.gemm_plan(200, 136, 72, 72, 72, True, True, 4, 1)
    assert kernel == 0
    assert "epi 4 (dgelu) runs only on the 256 kernel" in why
    # batch 0 is an empty grid: nothing could run even without the refusal
    with pytest.raises(RuntimeError, match="runs only on the 256 kernel"):
        ext.gemm(1 << 20, 1 << 20, 1 << 20, 1 << 20, 0, 200, 136, 72, 72, 72,
                 136, 0, 0, 0, 0, True, True, 4, 0, 0)


class HipGemm:
    def gemm(self, a, b, a_kc, b_kc, M, N, K, lda, ldb, sa, sb, batch, bias,
             epi, out, out_pre, ws_fill=None):
        if ws_fill is None:
            hip._gemm_raw(a, b, a_kc, b_kc, M, N, K, lda, ldb, sa, sb, batch,
                          bias=bias, epi=epi, out=out, out_pre=out_pre)
        else:   # the same call with a workspace that holds ws_fill
            n = ext.gemm_ws_floats(M, N, K, lda, ldb, a_kc, b_kc, epi, batch)
            assert n > 0
            ws = torch.full((n,), ws_fill, dtype=torch.float32, device=DEV)
            ext.gemm(a.data_ptr(), b.data_ptr(), out.data_ptr(), 0, 0, M, N,
                     K, lda, ldb, N, sa, sb, M * N, batch, a_kc, b_kc, epi,
                     ws.data_ptr(), hip._stream())
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def be():
    yield HipGemm()
    # the figures of docs/KERNELS.md (shown with pytest -s)
    print("\nlargest error / (1 ulp + floor):")
    print("\n".join(gc.measured_lines()))


@gpu
@pytest.mark.parametrize("case", gc.CASES, **_ids)
def test_case(be, case):
    gc.check_all(be, DEV, case)


@gpu
@pytest.mark.parametrize("case", gc.SEL_CASES, **_ids)
def test_selection_is_a_bit_exact_copy(be, case):
    gc.check_all(be, DEV, case)


@gpu
@pytest.mark.parametrize("case", gc.EPI256_CASES, **_ids)
def test_gelu_epilogues_of_the_256_kernel_per_element(be, case):
    gc.check_all(be, DEV, case)


@gpu
@pytest.mark.parametrize("fill", [float("nan"), 3.0e38, -3.0e38])
def test_split_workspace_needs_no_zeroing(be, fill):
    for lay in ("kc,kc", "ko,kc"):
        gc.check_int(be, DEV, gc.BY_NAME[f"split-130x67x2056-{lay}"],
                     ws_fill=fill)


# --------------------------------------------------------------------------
# the callers' mapping of torch views to layout flags
# --------------------------------------------------------------------------

@pytest.fixture
def hand_gemm():
    """Pin the GEMM sites to the hand kernels (test_gemm_tn_gpu.py)."""
    old = hip._GEMM_BACKEND
    hip._GEMM_BACKEND = "hip"
    yield
    hip._GEMM_BACKEND = old


def _ints(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(BF16)


def _exact(a, b):
    """bf16 bits of the float64 a @ b (exact: integers, 64 K < 2^24)."""
    return (a.double() @ b.double()).to(BF16)


def _matmul(a, b):
    c = hip.matmul(a, b)
    torch.cuda.synchronize()
    return c.cpu()


SHAPES = [(129, 136, 72), (128, 128, 64)]


@gpu
@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("a_t,b_t", [(False, False), (True, False),
                                     (False, True), (True, True)])
def test_matmul_2d_views(M, N, K, a_t, b_t):
    a, b = _ints(M, K, seed=M + 2 * a_t), _ints(K, N, seed=N + 3 * b_t)
    da = a.t().contiguous().to(DEV).t() if a_t else a.to(DEV)
    db = b.t().contiguous().to(DEV).t() if b_t else b.to(DEV)
    assert da.shape == a.shape and da.is_contiguous() != a_t
    assert db.shape == b.shape and db.is_contiguous() != b_t
    assert torch.equal(_matmul(da, db), _exact(a, b))


@gpu
@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_matmul_4d_with_transposed_b(M, N, K):
    a, b = _ints(2, 3, M, K, seed=K), _ints(2, 3, K, N, seed=K + 1)
    db = b.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)
    assert db.stride(-2) == 1
    assert torch.equal(_matmul(a.to(DEV), db), _exact(a, b))


@gpu
@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_matmul_broadcasts_a_batch_of_one(M, N, K):
    a, b = _ints(3, M, K, seed=K + 2), _ints(1, K, N, seed=K + 3)
    assert torch.equal(_matmul(a.to(DEV), b.to(DEV)), _exact(a, b))
    a1 = a[:1]
    b3 = _ints(3, K, N, seed=K + 4)
    assert torch.equal(_matmul(a1.to(DEV), b3.to(DEV)), _exact(a1, b3))


@gpu
@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_matmul_copies_what_no_layout_flag_describes(M, N, K):
    b = _ints(K, N, seed=K + 5)
    # neither dim has unit stride
    wide = _ints(M, 2 * K, seed=K + 6)
    a = wide.to(DEV)[:, ::2]
    assert a.stride() == (2 * K, 2)
    assert torch.equal(_matmul(a, b.to(DEV)), _exact(wide[:, ::2], b))
    # 16-byte rows that start 6 bytes off a 16-byte boundary: the kernel
    # would take them for aligned, so the caller copies (never launched
    # misaligned: ext.gemm refuses such an operand, test_gemm_oracle_cpu.py)
    wide = _ints(M, K + 8, seed=K + 7)
    a = wide.to(DEV)[:, 3:3 + K]
    assert a.stride(0) % 8 == 0 and a.data_ptr() % 16 == 6
    assert torch.equal(_matmul(a, b.to(DEV)), _exact(wide[:, 3:3 + K], b))
    # the same as a k-outer operand: 4-byte rows, 2 bytes off
    wide = _ints(K, M + 5 + (M % 2 == 0), seed=K + 8)
    a = wide.to(DEV)[:, 1:1 + M].t()
    assert a.stride(1) % 2 == 0 and a.data_ptr() % 4 == 2
    assert torch.equal(_matmul(a, b.to(DEV)), _exact(wide[:, 1:1 + M].t(), b))


@gpu
@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("pad,off", [(16, 8), (3, 8), (5, 3)])
def test_linear_fwd_weight_slice_of_a_wider_tensor(pad, off):
    M, N, K = 200, 136, 72
    x, wide = _ints(M, K, seed=1), _ints(N, K + pad + off, seed=2)
    bias = (torch.arange(N) * 5 % 127 - 63).to(BF16)
    w = wide.to(DEV)[:, off:off + K]
    assert w.stride(0) != K
    y, _ = hip.linear_fwd(x.to(DEV), w, bias.to(DEV))
    torch.cuda.synchronize()
    want = x.double() @ wide[:, off:off + K].double().t() + bias.double()
    assert torch.equal(y.cpu(), want.to(BF16))
