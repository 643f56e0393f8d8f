"""The criteria of tests/gemm_checks.py, proved on the CPU before the
128-tile GEMM kernel is held to them (test_gemm128_edges_gpu.py).

A stand-in backend (the fp32 torch.matmul of the bf16 inputs, bias added in
fp32, rounded once; gelu of the rounded pre-activation) passes every oracle on
every case, so the inputs are ones a correct implementation stays inside the
bounds with. Then eight deliberately wrong stand-ins, each the kind of bug the
kernel's data paths can have, must each be rejected by the oracle named next
to it, on the case named next to it.

Also here, because it launches nothing: the host side's decision about
operands whose base address is off the alignment their ld promises."""

import pytest
import torch

import gemm_checks as gc
from tepdist_amd.ops import _tepdist_hip as ext
from tepdist_amd.ops import fp64_reference as o

BF16 = torch.bfloat16


class CpuGemm:
    """hip._gemm_raw's contract on CPU tensors. The hooks are where the
    wrong variants below go wrong."""

    def operands(self, A, B, K):          # fp32 [Bt, M, K], [Bt, N, K]
        return A, B

    def product(self, A, B, K, plan):
        return A @ B.transpose(-1, -2)

    def bias(self, bias):
        return bias

    def finish(self, acc):                # fp32 [batch, M, N], bias added
        return acc

    def stray(self, out):
        pass

    def gemm(self, a, b, a_kc, b_kc, M, N, K, lda, ldb, sa, sb, batch, bias,
             epi, out, out_pre, ws_fill=None):
        A = (a if a_kc else a.transpose(-1, -2)).float()
        B = (b if b_kc else b.transpose(-1, -2)).float()
        assert A.shape[-2:] == (M, K) and B.shape[-2:] == (N, K)
        plan = ext.gemm_plan(M, N, K, lda, ldb, a_kc, b_kc, epi, batch)
        A, B = self.operands(A, B, K)
        acc = self.product(A, B, K, plan).expand(batch, M, N).clone()
        if epi in (1, 2):
            acc = acc + self.bias(bias).float()
        acc = self.finish(acc)
        if epi >= 2:
            pre = acc.to(BF16)
            out_pre.copy_(pre)
            acc = o.gelu_fwd(pre)         # float64, then one rounding
        out.copy_(acc.to(BF16))
        self.stray(out)


@pytest.mark.parametrize("case", gc.ALL_CASES, ids=lambda c: c.name)
def test_stand_in_passes_every_oracle(case):
    gc.check_all(CpuGemm(), "cpu", case)


# --------------------------------------------------------------------------
# wrong on purpose
# --------------------------------------------------------------------------

class DropsLastK(CpuGemm):
    def operands(self, A, B, K):
        A = A.clone()
        A[..., K - 1] = 0
        return A, B


class DropsEightOfOneTile(CpuGemm):       # k in [64, 72): one 16-byte vector
    def operands(self, A, B, K):
        A = A.clone()
        A[..., 64:72] = 0
        return A, B


class BiasFromNextColumn(CpuGemm):
    def bias(self, bias):
        return torch.roll(bias, -1)


class RoundsEachKTile(CpuGemm):           # bf16 partial sums per K-tile
    def product(self, A, B, K, plan):
        acc = 0
        for k in range(0, K, 64):
            acc = acc + (A[..., k:k + 64] @ B[..., k:k + 64]
                         .transpose(-1, -2)).to(BF16).float()
        return acc


class SwapsTwoRowsOfAPartialTile(CpuGemm):
    def finish(self, acc):                # rows 1, 2 of the last m-tile
        m0 = (acc.shape[1] - 1) // 128 * 128
        assert acc.shape[1] % 128 >= 3
        acc[:, [m0 + 1, m0 + 2]] = acc[:, [m0 + 2, m0 + 1]]
        return acc


class ZeroesLowMantissaBits(CpuGemm):
    # of operand A. The low byte of a bf16 is its seven mantissa bits and the
    # last exponent bit; small integers use only the top two mantissa bits,
    # so what they cannot see is modelled by clearing the other five.
    def operands(self, A, B, K):
        bits = A.to(BF16).view(torch.int16) & -32
        return bits.view(BF16).float(), B


class SkipsOneSplitChunk(CpuGemm):
    def product(self, A, B, K, plan):
        if plan[1] > 1:
            A = A.clone()
            A[..., plan[2]:2 * plan[2]] = 0
        return super().product(A, B, K, plan)


class WritesOnePastN(CpuGemm):            # of the last row
    def stray(self, out):
        torch.as_strided(out, (1,), (1,),
                         out.storage_offset() + out.numel())[0] = 1.0


# (wrong backend, the oracle that must reject it, on which case)
REJECTED = [
    (DropsLastK, "int", "ktail-128x128x65-kc,kc"),
    (DropsLastK, "int", "ktail-128x128x1-kc,ko"),
    (DropsLastK, "sel_a", "sel-128x128x65-kc,kc-a"),
    (DropsEightOfOneTile, "int", "pipe-128x128x128-kc,kc"),
    (DropsEightOfOneTile, "int", "ktail-128x128x72-ko,kc"),
    (BiasFromNextColumn, "int", "epi1-200x136x72-kc,kc"),
    (BiasFromNextColumn, "int", "epi2-128x128x64-kc,ko"),
    (BiasFromNextColumn, "rand", "epi1-257x255x200-kc,ko"),
    (RoundsEachKTile, "rand", "pipe-128x128x320-kc,kc"),
    (RoundsEachKTile, "rand", "edge-257x255x200-kc,ko"),
    (SwapsTwoRowsOfAPartialTile, "int", "edge-200x136x72-ko,ko"),
    (SwapsTwoRowsOfAPartialTile, "sel_b", "sel-127x130x136-kc,kc-b"),
    (ZeroesLowMantissaBits, "sel_b", "sel-128x128x192-ko,kc-b"),
    (ZeroesLowMantissaBits, "rand", "pipe-128x128x64-kc,kc"),
    (SkipsOneSplitChunk, "int", "split-128x128x2048-kc,kc"),
    (SkipsOneSplitChunk, "int", "split-130x67x2056-ko,kc"),
    (WritesOnePastN, "int", "edge-130x67x64-kc,kc"),
    (WritesOnePastN, "rand", "epi3-200x136x72-kc,kc"),
]


@pytest.mark.parametrize("wrong,oracle,name", REJECTED,
                         ids=lambda v: getattr(v, "__name__", v))
def test_wrong_backend_is_rejected(wrong, oracle, name):
    case = gc.BY_NAME[name]
    assert oracle in case.oracles
    with pytest.raises(AssertionError):
        gc.check(wrong(), "cpu", case, oracle)
    gc.check(CpuGemm(), "cpu", case, oracle)      # and only the wrong one


def test_small_integers_cannot_see_lost_low_mantissa_bits():
    # why the selection oracle exists: integers in [-8, 8] have the low
    # five mantissa bits zero already
    gc.check(ZeroesLowMantissaBits(), "cpu",
             gc.BY_NAME["pipe-128x128x64-kc,kc"], "int")


# --------------------------------------------------------------------------
# operand base addresses (csrc/gemm_plan.h operand_why_not)
# --------------------------------------------------------------------------

def _why(base, ld, kc, M=200, N=136, K=72, stride=0, batch=1, other_ld=None):
    ldb = other_ld if other_ld is not None else K
    return ext.gemm_operand_why_not(M, N, K, ld, ldb, kc, True, 0, batch,
                                    True, base, stride)


def test_operand_base_must_match_what_its_ld_selects():
    base = 1 << 20
    # 16-byte rows of a k-contiguous operand: 16-byte loads and the DMA
    assert _why(base, 72, True) == ""
    for off in (2, 4, 8, 14):
        assert "not 16-byte aligned" in _why(base + off, 72, True)
    # rows off 16 bytes go by element loads: any bf16 address
    for off in (0, 2, 6):
        assert _why(base + off, 75, True) == ""
        assert _why(base + off, 203, False) == ""
    # k-outer on the 128 kernel: 4-byte pairs when ld is even
    assert _why(base + 4, 208, False) == ""
    assert "not 4-byte aligned" in _why(base + 2, 208, False)
    assert "not 4-byte aligned" in _why(base + 6, 202, False)
    # two k-outer operands on the 256 kernel read 16-byte rows
    assert ext.gemm_plan(256, 256, 128, 256, 256, False, False, 0, 1)[0] == 256
    assert "not 16-byte aligned" in ext.gemm_operand_why_not(
        256, 256, 128, 256, 256, False, False, 0, 1, True, base + 4, 0)
    # every batch element starts on the same boundary
    assert _why(base, 72, True, stride=200 * 72 + 8, batch=3) == ""
    assert "batch stride" in _why(base, 72, True, stride=200 * 72 + 4,
                                  batch=3)
    assert _why(base, 72, True, stride=200 * 72 + 4, batch=1) == ""


def test_gemm_refuses_a_misaligned_operand_before_launching():
    # batch 0 is an empty grid: even if the refusal were lost, nothing runs
    base = 1 << 20
    args = dict(C=base, Cpre=0, bias=0, M=200, N=136, K=72, lda=72, ldb=72,
                ldc=136, sa=0, sb=0, sc=0, batch=0, a_kc=True, b_kc=True,
                epi=0, splitk_ws=0, stream=0)
    with pytest.raises(RuntimeError, match="A: .*not 16-byte aligned"):
        ext.gemm(A=base + 2, B=base, **args)
    with pytest.raises(RuntimeError, match="B: .*not 16-byte aligned"):
        ext.gemm(A=base, B=base + 6, **args)


def test_callers_copy_a_view_that_starts_off_its_alignment():
    from tepdist_amd.ops.hip import _base_suits_ld
    wide = torch.zeros(16, 80, dtype=BF16)
    assert wide.data_ptr() % 16 == 0
    assert _base_suits_ld(wide[:, 8:72], 80)
    assert not _base_suits_ld(wide[:, 3:67], 80)      # 6 bytes in, 16 B rows
    assert not _base_suits_ld(wide[:, 1:65], 82)      # 2 bytes in, 4 B rows
    assert _base_suits_ld(wide[:, 2:66], 82)
    assert _base_suits_ld(wide[:, 1:65], 81)          # element loads
    assert not _base_suits_ld(wide, 80, batch_stride=16 * 80 + 4)


def test_matmul_refuses_a_batch_that_broadcasts_in_part():
    # flattened batches broadcast as a whole or not at all; raised before
    # anything is launched, so CPU tensors do
    from tepdist_amd.ops.hip import _matmul_hip
    a = torch.zeros(2, 1, 8, 8, dtype=BF16)
    b = torch.zeros(2, 3, 8, 8, dtype=BF16)
    with pytest.raises(ValueError, match="batch dims"):
        _matmul_hip(a, b)
