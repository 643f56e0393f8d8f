"""The flash attention kernels (ops/csrc/attention.hip: forward, dK/dV, dQ,
delta) at their mask and tile edges, against the float64 oracles of
tepdist_amd/ops/fp64_reference.py under the per-element bound
|got - fp64| <= 1 ulp + floor, every element asserted.

Inputs, shapes, floors and their derivations live in tests/flash_checks.py;
tests/test_flash_oracle_cpu.py runs the same checks with an emulation of
the kernels' arithmetic on the CPU and shows that wrong variants fail them.
"""

import pytest
import torch

import flash_checks as fc
import rowwise_checks as rc
from tepdist_amd import ops

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from tepdist_amd.ops import hip as be
    yield be
    # the figures of docs/KERNELS.md (shown with pytest -s)
    print("\noutput: largest error in ulps where the floor is under 1/8 ulp"
          " / anywhere / as a fraction of 1 ulp + floor")
    for key, (plain, anywhere, frac) in rc.MEASURED.items():
        if key.startswith("flash_"):
            print(f"{key:20s} {plain:6.3f} {anywhere:10.1f} {frac:6.3f}")


@pytest.mark.parametrize("D,S,causal,kind", list(fc.cases_4d()))
def test_flash_4d(hip, D, S, causal, kind):
    fc.check_flash(hip, DEV, 1, 1, S, D, causal, kind)


@pytest.mark.parametrize("B,H,D,S,causal,kind,layout",
                         list(fc.cases_layout()))
def test_flash_layouts(hip, B, H, D, S, causal, kind, layout):
    fc.check_flash(hip, DEV, B, H, S, D, causal, kind, layout)


@pytest.mark.parametrize("sentinel", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_flash_bwd_global_lse(hip, D, sentinel):
    fc.check_flash_bwd_global_lse(hip, DEV, D, sentinel=sentinel)


def test_attention_rejects_mismatched_operands(hip):
    """S, H and D are taken from q alone: an operand of another shape or
    dtype would be misread (a shorter k out of bounds), so it must raise
    before any launch. The composed path for other head dims stays."""
    B, H, S, D = 2, 3, 72, 64

    def t(*shape, dtype=BF16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)
    q = t(B, H, S, D)
    out, res = hip.attention_fwd(q, q, q, causal=True)
    for bad in (t(B, H, S - 8, D), t(B, H - 1, S, D), t(B, H, S, 128),
                t(B, H, S, D, dtype=torch.float16),
                t(B, H, S, D, dtype=torch.float32)):
        for args in ((q, bad, q), (q, q, bad), (bad, q, q)):
            with pytest.raises(ValueError, match="attention_fwd"):
                hip.attention_fwd(*args, causal=True)
        # (dout, q, k, v, (out, lse)), each in turn
        for i in range(5):
            a = [q, q, q, q, out]
            a[i] = bad
            with pytest.raises(ValueError, match="attention_bwd"):
                hip.attention_bwd(*a[:4], (a[4], res[1]), causal=True)
    with pytest.raises(ValueError, match="lse"):
        hip.attention_bwd(q, q, q, q, (out, res[1][:, :S - 1]), causal=True)
    with pytest.raises(ValueError, match="lse"):
        hip.attention_bwd(q, q, q, q, (out, res[1].to(BF16)), causal=True)

    # packed: what does not split into 3 * heads * D, another dtype, and
    # flash residuals with a head dim the kernels do not have
    qkv = t(B, S, 3 * H * D)
    pout, pres = hip.attention_qkv_fwd(qkv, H, causal=True)
    with pytest.raises(ValueError, match="attention_qkv_fwd"):
        hip.attention_qkv_fwd(t(B, S, 3 * H * D + 8), H, causal=True)
    with pytest.raises(ValueError, match="attention_qkv_fwd"):
        hip.attention_qkv_fwd(qkv.to(torch.float16), H, causal=True)
    with pytest.raises(ValueError, match="attention_qkv_bwd"):
        hip.attention_qkv_bwd(pout.float(), qkv, H, pres, causal=True)
    with pytest.raises(ValueError, match="attention_qkv_bwd"):
        hip.attention_qkv_bwd(pout[:, :S - 8], qkv, H, pres, causal=True)
    with pytest.raises(ValueError, match="lse"):
        hip.attention_qkv_bwd(pout, qkv, H, (pout, pres[1][:1]), causal=True)
    qkv96 = t(B, S, 3 * H * 96)
    with pytest.raises(ValueError, match="head dim 96"):
        hip.attention_qkv_bwd(t(B, S, H * 96), qkv96, H,
                              (t(B, S, H * 96), pres[1]), causal=True)
    # the documented composed path for D = 96 stays
    assert hip.attention_qkv_fwd(qkv96, H, causal=True) is None
    g = rc.gen(96)
    x = rc.randn(g, B, S, 3 * H * 96).to(DEV).requires_grad_()
    y = ops.attention_qkv(x, H, causal=True)
    y.backward(torch.ones_like(y))
    ry = ops.attention_qkv(x.detach().cpu().float(), H, causal=True)
    assert (y.detach().cpu().float() - ry).abs().max() < 3e-2
    assert torch.isfinite(x.grad).all()
