"""skinny_plan (csrc/skinny_plan.h, bound host-only) against plans worked
out by hand, and the CPU reference decode linears against fp64."""

import pytest
import torch

from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import reference as ref

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def plan():
    from tepdist_amd.ops import _tepdist_hip as ext
    return lambda M, N, K, ldx=None, ldw=None, epi=0, dual=False: \
        ext.skinny_plan(M, N, K, ldx or K, ldw or K, epi, dual)


# (M, N, K, dual) -> (mt, rows, waves, k_per_wave): blocks = ceil(N / rows),
# waves = the power of two that brings blocks * waves to 1024 (at most 8),
# capped by the K / 64 steps; k_per_wave = ceil(steps / waves) * 64
PLANS = [
    ((1, 2048, 2048, False), (1, 16, 8, 256)),     # 128 blocks, 32 steps
    ((16, 3072, 2048, False), (1, 16, 8, 256)),    # 192 blocks
    ((17, 2048, 6144, False), (2, 16, 8, 768)),    # 96 steps over 8 waves
    ((32, 16, 64, False), (2, 16, 1, 64)),         # one step: one wave
    ((33, 16, 192, False), (4, 16, 3, 64)),        # 3 steps cap the waves
    ((64, 40, 1088, False), (4, 16, 8, 192)),      # 17 steps: 3, 2, 2, ...
    ((64, 32000, 2048, False), (4, 32, 2, 1024)),  # 2000 tiles: 32 rows
    ((32, 6144, 2048, True), (2, 16, 4, 512)),     # dual stays at 16 rows
    ((8, 16384, 1024, True), (1, 16, 1, 1024)),    # 1024 blocks: 1 wave
]


@pytest.mark.parametrize("args,want", PLANS)
def test_plan_table(plan, args, want):
    M, N, K, dual = args
    mt, rows, waves, kpw, split_k, why = plan(M, N, K, dual=dual)
    assert (mt, rows, waves, kpw) == want and split_k == 1 and why == ""
    # wave w owns steps w, w + waves, ...: every wave has one, none is
    # owned twice, all are owned
    steps = [list(range(w, K // 64, waves)) for w in range(waves)]
    assert all(steps) and max(map(len, steps)) * 64 == kpw
    assert sorted(sum(steps, [])) == list(range(K // 64))


@pytest.mark.parametrize("kw,word", [
    (dict(M=65, N=16, K=64), "1..64"),
    (dict(M=0, N=16, K=64), "1..64"),
    (dict(M=4, N=16, K=96), "multiple of 64"),
    (dict(M=4, N=16, K=0), "multiple of 64"),
    (dict(M=4, N=16, K=64, ldw=68), "16-byte"),
    (dict(M=4, N=16, K=64, ldx=60), "16-byte"),
    (dict(M=4, N=16, K=64, epi=5), "epi"),
    (dict(M=4, N=16, K=64, epi=1, dual=True), "dual"),
])
def test_plan_refuses(plan, kw, word):
    got = plan(**kw)
    assert got[:4] == (0, 0, 0, 0) and word in got[5], got


@pytest.mark.parametrize("act,bias,res", [("none", False, False),
                                          ("none", True, True),
                                          ("gelu", True, False)])
def test_reference_linear_decode(act, bias, res):
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(5, 64, generator=g).to(BF16), \
        torch.randn(24, 64, generator=g).to(BF16)
    b = torch.randn(24, generator=g).to(BF16) if bias else None
    r = torch.randn(5, 24, generator=g).to(BF16) if res else None
    a = o.f64(x) @ o.f64(w).t() + (o.f64(b) if bias else 0.0)
    want = (o.gelu_fwd(a) if act == "gelu" else a) + (o.f64(r) if res else 0)
    # fp32 math: K 2^-24 sum|x||w| for the sum, 2^-20 max(1, |a|) for gelu
    floor = 64 * 2.0 ** -24 * (o.f64(x).abs() @ o.f64(w).abs().t()) \
        + 2.0 ** -20 * a.abs().clamp_min(1.0)
    o.assert_within_ulp(ref.linear_decode(x, w, b, act, r), want, floor, act)


def test_reference_swiglu_linear_decode():
    g = torch.Generator().manual_seed(2)
    x, wg, wu = (torch.randn(*s, generator=g).to(BF16)
                 for s in ((5, 64), (24, 64), (24, 64)))
    gt, up = o.f64(x) @ o.f64(wg).t(), o.f64(x) @ o.f64(wu).t()
    acc = 64 * 2.0 ** -24
    floor = (acc * (o.f64(x).abs() @ o.f64(wg).abs().t()) * 1.1 * up.abs()
             + acc * (o.f64(x).abs() @ o.f64(wu).abs().t()) * gt.abs()
             + 2.0 ** -20 * gt.abs().clamp_min(1.0) * up.abs())
    o.assert_within_ulp(ref.swiglu_linear_decode(x, wg, wu),
                        o.swiglu_fwd(gt, up), floor, "swiglu")
