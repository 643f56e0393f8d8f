"""The 256-tile GEMM with its two wave halves staggered by one barrier.

Exact oracle: operands are integers in [-8, 8], so every K-tile is distinct
and every fp32 sum is exact (|sum| <= 64 K < 2^24); the expected result is the
fp64 product rounded once to bf16, and the kernel must give those bits. A tile
read before its DMA landed, or restaged before its last read retired, changes
an integer sum. Shapes reach each edge of the schedule: two and three K-tiles,
the slot wraps, blocks that share panels, a split plan with a short last
chunk, and a screen of repeated calls at sizes that fill the chip."""

import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tepdist_amd.ops import _tepdist_hip as ext

if torch.cuda.is_available():
    from tepdist_amd.ops import hip

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
ROOT = Path(__file__).resolve().parent.parent

# (M, N, K) of C[M,N]; canonical operands are A [M,K], B [N,K], k-outer ones
# A [K,M], B [K,N]
SMALL = [(256, 256, 128), (256, 256, 192), (256, 256, 256), (256, 256, 320),
         (256, 256, 576), (512, 512, 256)]
SPLIT = (256, 256, 2432)          # 13 chunks of 192, the last one 128
BIG_KC = (4096, 4096, 1024)       # 256 blocks
BIG_KO = (4096, 1024, 4096)       # 64 tiles (the plan splits K over them)
EPI_SHAPES = [(256, 256, 128), (512, 256, 320)]


def _plan(M, N, K, ko, epi=0):
    lda, ldb = (M, N) if ko else (K, K)
    return ext.gemm_plan(M, N, K, lda, ldb, not ko, not ko, epi, 1)


def test_plan_gives_every_shape_the_256_kernel():
    for ko in (False, True):
        for M, N, K in SMALL:
            kernel, split_k, k_chunk, why_not = _plan(M, N, K, ko)
            assert (kernel, split_k, k_chunk) == (256, 1, 0), (M, N, K, ko)
            assert why_not == ""
        kernel, s, kc, why_not = _plan(*SPLIT, ko)
        assert kernel == 256 and s > 1 and why_not == "", (SPLIT, ko)
        last = SPLIT[2] - (s - 1) * kc
        assert 128 <= last < kc, (s, kc, last)        # a short last chunk
    for M, N, K in SMALL:
        assert _plan(M, N, K, False, epi=1)[:3] == (256, 1, 0)
    assert _plan(*BIG_KC, False)[:3] == (256, 1, 0)
    kernel, s, kc, why_not = _plan(*BIG_KO, True)
    assert kernel == 256 and why_not == ""
    assert (s - 1) * kc < BIG_KO[2] <= s * kc
    for epi in (2, 3, 4):
        for M, N, K in EPI_SHAPES:
            assert _plan(M, N, K, False, epi)[:3] == (256, 1, 0)


def _ints(*shape, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(BF16).to(dev)


def _operands(M, N, K, ko, seed):
    """(a, b, exact fp64 product rounded once to bf16, fp64 column sums of a
    k-outer a rounded once to bf16)."""
    if ko:
        a, b = _ints(K, M, seed=seed), _ints(K, N, seed=seed + 1)
        want = a.double().t() @ b.double()
        cs = a.double().sum(0).to(BF16)
    else:
        a, b = _ints(M, K, seed=seed), _ints(N, K, seed=seed + 1)
        want = a.double() @ b.double().t()
        cs = None
    assert want.abs().max().item() < 2 ** 24
    return a, b, want, cs


def _run(a, b, M, N, K, ko, bias=None, colsum=False):
    db = torch.empty(M, dtype=BF16, device="cuda") if colsum else None
    lda, ldb = (M, N) if ko else (K, K)
    c = hip._gemm_raw(a, b, not ko, not ko, M, N, K, lda, ldb, 0, 0, 1,
                      bias=bias, epi=1 if bias is not None else 0,
                      colsum_out=db)[0]
    return c, db


@gpu
@pytest.mark.parametrize("M,N,K", SMALL + [SPLIT])
def test_canonical_exact(M, N, K):
    a, b, want, _ = _operands(M, N, K, False, seed=K + M)
    c, _ = _run(a, b, M, N, K, False)
    assert torch.equal(c, want.to(BF16))
    if (M, N, K) != SPLIT:        # the plan splits no epilogue
        bias = _ints(N, seed=7 * K)
        c, _ = _run(a, b, M, N, K, False, bias=bias)
        assert torch.equal(c, (want + bias.double()).to(BF16))


@gpu
@pytest.mark.parametrize("M,N,K", SMALL + [SPLIT])
def test_k_outer_exact(M, N, K):
    a, b, want, cs = _operands(M, N, K, True, seed=3 * K + M)
    c, _ = _run(a, b, M, N, K, True)
    assert torch.equal(c, want.to(BF16))
    c, db = _run(a, b, M, N, K, True, colsum=True)
    assert torch.equal(c, want.to(BF16))
    assert torch.equal(db, cs)


@gpu
@pytest.mark.parametrize("epi", [2, 3, 4])
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_gelu_epilogues(M, N, K, epi):
    g = torch.Generator().manual_seed(100 * epi + K)
    a = torch.randn(M, K, generator=g).to(BF16).cuda()
    b = torch.randn(N, K, generator=g).to(BF16).cuda()
    bias = torch.randn(N, generator=g).to(BF16).cuda() if epi == 2 else None
    pre_in = torch.randn(M, N, generator=g).to(BF16).cuda()
    c, pre = hip._gemm_raw(a, b, True, True, M, N, K, K, K, 0, 0, 1,
                           bias=bias, epi=epi,
                           out_pre=pre_in if epi == 4 else None)
    torch.cuda.synchronize()
    up = a.double() @ b.double().t()
    if bias is not None:
        up = up + bias.double()
    if epi == 4:
        p64 = pre_in.double().requires_grad_()
        torch.nn.functional.gelu(p64, approximate="tanh").backward(up)
        want = p64.grad
    else:
        want = torch.nn.functional.gelu(up, approximate="tanh")
        err = (pre.double() - up).abs().max().item() / math.sqrt(K)
        assert err < 3e-2, err
    # the bound tests/test_kernels_gpu.py holds these epilogues to
    err = (c.double() - want).abs().max().item() / math.sqrt(K)
    print(f"epi {epi} {M}x{N}x{K}: scaled err {err:.2e}")
    assert err < 3e-2, err


@gpu
@pytest.mark.parametrize("shape,ko", [(BIG_KC, False), (BIG_KO, True)])
def test_race_screen_under_load(shape, ko):
    M, N, K = shape
    sets = []
    for s in range(4):
        a, b, want, cs = _operands(M, N, K, ko, seed=1000 + 10 * s + ko)
        sets.append((a, b, want.to(BF16), cs))
    bad = []
    for call in range(20):
        a, b, want, cs = sets[call % 4]
        c, db = _run(a, b, M, N, K, ko, colsum=ko and call % 2 == 1)
        if not torch.equal(c, want):
            bad.append((call, int((c != want).sum().item())))
        if db is not None and not torch.equal(db, cs):
            bad.append((call, "colsum"))
    assert not bad, bad


_MLP_CHILD = r"""
import json, torch
from tepdist_amd.ops import hip
assert hip._GEMM_BACKEND == "hip"
T, d = 512, 256
g = torch.Generator().manual_seed(5)
mk = lambda *s, k=0.05: (torch.randn(*s, generator=g) * k).to(torch.bfloat16).cuda()
x, w1, b1, w2, b2 = mk(T, d, k=0.5), mk(4 * d, d), mk(4 * d), mk(d, 4 * d), mk(d)
dy = mk(T, d, k=1.0)
_, (h, pre) = hip.mlp_fwd(x, w1, b1, w2, b2)
dx, dw1, db1, dw2, db2 = hip.mlp_bwd(dy, x, w1, w2, h, pre)
# dh as mlp_bwd's hand path forms it (the same call, so the same bits)
dh = hip._gemm_raw(dy, hip.transpose2d(w2), True, True, T, 4 * d, d, d, d,
                   0, 0, 1, epi=4, out_pre=pre)[0]
db = torch.empty(4 * d, dtype=torch.bfloat16, device="cuda")
hip._gemm_raw(dh, x, False, False, 4 * d, d, T, 4 * d, d, 0, 0, 1, colsum_out=db)
torch.cuda.synchronize()
s64 = dh.double().sum(0)
bound = 2.0 ** -8 * s64.abs() + T * 2.0 ** -23 * dh.double().abs().sum(0)
err = (db1.double() - s64).abs()
print(json.dumps({"in_place": bool(hip._wgrad_in_place(dh, x)),
                  "worst": (err / bound).max().item(),
                  "ok": bool((err <= bound).all()),
                  "from_wgrad": bool(torch.equal(db1, db)),
                  "nonzero": bool(s64.abs().max().item() > 0)}))
"""


@gpu
def test_mlp_bwd_db1_from_the_wgrad():
    # TEPDIST_MLP_FUSED=0 keeps the library's fused dgelu out of the way, so
    # that the pinned hand path is the one with the dgelu epilogue
    env = dict(os.environ, TEPDIST_GEMM_BACKEND="hip", TEPDIST_MLP_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _MLP_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["in_place"] and res["nonzero"] and res["from_wgrad"]
    assert res["ok"], res
