"""Flash attention after the masked-slice skip, balanced q-pair ownership,
single-image transposed LDS reads and constant folding: the transposed
fragment helper against its stated lane/element map, and forward + backward
(+ LSE) against fp32 SDPA at the smallest shapes that reach each path."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tepdist_amd.ops import hip
from tepdist_amd import ops

BF16 = torch.bfloat16

# (B, H, S, D): single tile; ragged single block; second fwd/dq block of 8
# rows + third kv block; both 512-row blocks full (every skip and every
# remapped pair live); D=128 ragged and multi-block.
SHAPES = [(1, 2, 64, 64), (1, 2, 200, 64), (2, 2, 520, 64),
          (1, 2, 1024, 64), (1, 2, 328, 128), (1, 1, 640, 128)]


def _randn(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16).cuda()


def _scaled_err(ours, ref32, scale=None):
    err = (ours.float() - ref32).abs()
    denom = scale if scale is not None else ref32.abs().max().clamp_min(1.0)
    return (err / denom).max().item()


@pytest.mark.parametrize("C", [64, 128])
def test_tr_frag_lane_element_map(C):
    """tr_frag<C> (lds_frag.h) over a [64][C] image written through loff<C>
    with the bf16 bit pattern row*128 + col: lane 16g+i, element e of
    fragment (c, df) must hold image[32c + 16*(e>>2) + 4g + (e&3)][16df + i].
    Checks every lane and element, so a swapped 8-byte half behind the XOR
    swizzle cannot pass."""
    from tepdist_amd.ops import _tepdist_hip as ext
    DF = C // 16
    out = torch.full((2, DF, 64, 8), -1, dtype=torch.int32, device="cuda")
    ext.tr16_frag_probe(out.data_ptr(), C,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = torch.arange(2).view(2, 1, 1, 1)
    df = torch.arange(DF).view(1, DF, 1, 1)
    lane = torch.arange(64).view(1, 1, 64, 1)
    e = torch.arange(8).view(1, 1, 1, 8)
    row = 32 * c + 16 * (e // 4) + 4 * (lane // 16) + (e % 4)
    col = 16 * df + (lane % 16)
    expect = (row * 128 + col).to(torch.int32)
    got = out.cpu()
    bad = (got != expect).nonzero()
    assert bad.numel() == 0, (
        f"{bad.shape[0]} wrong elements, first (c, df, lane, e) = "
        f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()} "
        f"expected {expect[tuple(bad[0])].item()}")


def _reference(q, k, v, dout, causal):
    """fp32 SDPA forward/backward and the fp32 logsumexp of the scaled,
    masked scores."""
    q2, k2, v2 = (t.float().requires_grad_() for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(
        q2, k2, v2, is_causal=causal)
    ref.backward(dout.float())
    S, D = q.shape[-2], q.shape[-1]
    s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    return ref.detach(), q2.grad, k2.grad, v2.grad, torch.logsumexp(s, -1)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,S,D", SHAPES)
def test_flash_fwd_bwd_vs_sdpa(B, H, S, D, causal):
    q = _randn(B, H, S, D, seed=70)
    k = _randn(B, H, S, D, seed=71)
    v = _randn(B, H, S, D, seed=72)
    dout = _randn(B, H, S, D, seed=73)
    ref, rdq, rdk, rdv, rlse = _reference(q, k, v, dout, causal)

    # 4-D entry points
    out, res = hip.attention_fwd(q, k, v, causal=causal)
    assert len(res) == 2, "flash path should save (out, lse)"
    dq, dk, dv = hip.attention_bwd(dout, q, k, v, res, causal=causal)
    torch.cuda.synchronize()
    lse = res[1].reshape(B, H, S)
    errs = {
        "out": _scaled_err(out, ref),
        "dq": _scaled_err(dq, rdq, rdq.abs().max()),
        "dk": _scaled_err(dk, rdk, rdk.abs().max()),
        "dv": _scaled_err(dv, rdv, rdv.abs().max()),
        "lse": (lse - rlse).abs().max().item(),
    }

    # packed-qkv entry point (strided kernels) on the same data
    d = H * D
    def pack(t):
        return t.transpose(1, 2).reshape(B, S, d)
    qkv = torch.cat([pack(q), pack(k), pack(v)], dim=-1).contiguous()
    qkv.requires_grad_()
    pout = ops.attention_qkv(qkv, H, causal=causal)
    pout.backward(pack(dout).contiguous())
    torch.cuda.synchronize()
    rgrad = torch.cat([pack(rdq), pack(rdk), pack(rdv)], dim=-1)
    errs["packed_out"] = _scaled_err(pout.detach(), pack(ref))
    for name, sl in (("packed_dq", slice(0, d)), ("packed_dk", slice(d, 2 * d)),
                     ("packed_dv", slice(2 * d, 3 * d))):
        r = rgrad[..., sl]
        errs[name] = _scaled_err(qkv.grad[..., sl], r, r.abs().max())

    print(f"flash_trim {(B, H, S, D)} causal={causal}: " +
          " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    assert errs["out"] < 3e-2 and errs["packed_out"] < 3e-2, errs
    for n in ("dq", "dk", "dv", "packed_dq", "packed_dk", "packed_dv"):
        assert errs[n] < 5e-2, errs
    assert errs["lse"] < 1e-2, errs
