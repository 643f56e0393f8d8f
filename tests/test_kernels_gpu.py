"""GPU numerics tests: every hand-written gfx950 kernel vs a plain PyTorch
fp32 reference of the same op (SURVEY.md §4 test strategy)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tepdist_amd.ops import hip
from tepdist_amd import ops

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


# --------------------------------------------------------------------------


@pytest.fixture
def hand_gemm():
    """Pin the GEMM sites to the hand kernels: in the default "auto" mode
    _pick_backend returns the output of whichever of the hand kernel and
    hipBLASLt was faster, which need not be the hand kernel's."""
    old = hip._GEMM_BACKEND
    hip._GEMM_BACKEND = "hip"
    yield
    hip._GEMM_BACKEND = old


def _plan(M, N, K, lda, ldb, a_kc=True, b_kc=True, epi=0, batch=1):
    return hip.ext.gemm_plan(M, N, K, lda, ldb, a_kc, b_kc, epi, batch)


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 72),
                                   (256, 512, 1024), (33, 17, 9)])
def test_gemm_nt_layout(M, N, K):
    # asymmetric inputs (catches transposed-output bugs)
    a = _randn(M, K, seed=1)
    w = _randn(N, K, seed=2)
    y, _ = hip.linear_fwd(a, w, None, "none")
    torch.cuda.synchronize()
    ref = a.float() @ w.float().t()
    _assert_close_bf16(y, ref, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True),
                                   (True, False)])
def test_gemm_transposes(ta, tb):
    M, N, K = 96, 144, 80
    a_base = _randn(K, M, seed=3) if ta else _randn(M, K, seed=3)
    b_base = _randn(N, K, seed=4) if tb else _randn(K, N, seed=4)
    a = a_base.t() if ta else a_base
    b = b_base.t() if tb else b_base
    c = hip.matmul(a, b)
    torch.cuda.synchronize()
    ref = a.float() @ b.float()
    _assert_close_bf16(c, ref, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("M,N,K", [(512, 256, 8192), (256, 256, 4096),
                                   (768, 512, 16384), (3072, 768, 2048),
                                   (768, 768, 2048), (2304, 768, 2048)])
def test_gemm_splitk_256(M, N, K):
    # canonical KCxKC shapes deep enough to trigger the split-K path of the
    # 256-tile kernel (fp32 partials + reduce)
    a = _randn(M, K, seed=11)
    b = _randn(N, K, seed=12)
    y = hip.matmul(a, b.t())
    torch.cuda.synchronize()
    ref = a.float() @ b.float().t()
    _assert_close_bf16(y, ref, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_gemm_batched():
    B, M, N, K = 6, 64, 96, 32
    a = _randn(B, M, K, seed=5)
    b = _randn(B, K, N, seed=6)
    c = hip.matmul(a, b)
    torch.cuda.synchronize()
    ref = a.float() @ b.float()
    _assert_close_bf16(c, ref, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_linear_bias_gelu():
    M, N, K = 128, 96, 64
    x = _randn(M, K, seed=7)
    w = _randn(N, K, seed=8)
    b = _randn(N, seed=9)
    y, pre = hip.linear_fwd(x, w, b, "gelu")
    torch.cuda.synchronize()
    pre_ref = (x.float() @ w.float().t() + b.float())
    y_ref = torch.nn.functional.gelu(pre_ref, approximate="tanh")
    _assert_close_bf16(pre, pre_ref, rtol=3e-2, scale=math.sqrt(K))
    _assert_close_bf16(y, y_ref, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_linear_bwd():
    M, N, K = 192, 80, 112
    x = _randn(M, K, seed=10)
    w = _randn(N, K, seed=11)
    dy = _randn(M, N, seed=12)
    dx, dw, db = hip.linear_bwd(dy, x, w, True, "none", None)
    torch.cuda.synchronize()
    _assert_close_bf16(dx, dy.float() @ w.float(), rtol=3e-2,
                       scale=math.sqrt(N))
    _assert_close_bf16(dw, dy.float().t() @ x.float(), rtol=3e-2,
                       scale=math.sqrt(M))
    _assert_close_bf16(db, dy.float().sum(0), rtol=3e-2, scale=math.sqrt(M))


# Plan branches (csrc/gemm_plan.h) that the shapes above do not reach. Each
# test first asserts the plan, so that it keeps covering its branch.

@pytest.mark.usefixtures("hand_gemm")
def test_gemm_splitk_128_by_layout():
    # k-outermost operands: split-K on the 128 kernel's register-transpose
    # staging
    M, N, K = 128, 128, 2048
    assert _plan(M, N, K, M, N, False, False)[:3] == (128, 16, 128)
    a = _randn(K, M, seed=41).t()
    b = _randn(K, N, seed=42)
    c = hip.matmul(a, b)
    torch.cuda.synchronize()
    _assert_close_bf16(c, a.float() @ b.float(), rtol=3e-2,
                       scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
@pytest.mark.parametrize("K,plan", [
    (2176, (128, 12, 192)),   # last chunk is one K-tile: 256 kernel refuses
    (2048, (256, 16, 128))])  # the smallest split the 256 kernel runs
def test_gemm_splitk_canonical_edges(K, plan):
    M, N = 256, 256
    assert _plan(M, N, K, K, K)[:3] == plan
    a = _randn(M, K, seed=43)
    b = _randn(N, K, seed=44)
    y = hip.matmul(a, b.t())
    torch.cuda.synchronize()
    _assert_close_bf16(y, a.float() @ b.float().t(), rtol=3e-2,
                       scale=math.sqrt(K))


@pytest.mark.usefixtures("hand_gemm")
def test_gemm_splitk_k_tail_17_chunks():
    # K is no multiple of 64: 17 chunks of 128, the last one 8 long
    M, N, K = 120, 136, 2056
    assert _plan(M, N, K, K, K)[:3] == (128, 17, 128)
    x = _randn(M, K, seed=45)
    w = _randn(N, K, seed=46)
    y, _ = hip.linear_fwd(x, w, None, "none")
    torch.cuda.synchronize()
    _assert_close_bf16(y, x.float() @ w.float().t(), rtol=3e-2,
                       scale=math.sqrt(K))


def test_gemm_dgelu_rejected_with_plan_reason():
    # epi 4 exists on the 256 kernel only; nothing is launched
    M, N, K = 500, 256, 128
    kernel, _, _, why = _plan(M, N, K, K, K, epi=4)
    assert kernel == 0 and why
    a = _randn(M, K, seed=47)
    b = _randn(N, K, seed=48)
    pre = _randn(M, N, seed=49)
    with pytest.raises(RuntimeError) as exc:
        hip._gemm_raw(a, b, True, True, M, N, K, K, K, 0, 0, 1, epi=4,
                      out_pre=pre)
    assert why in str(exc.value)


# --------------------------------------------------------------------------


def test_layernorm_fwd_bwd():
    rows, cols = 512, 1024
    x = _randn(rows, cols, seed=13)
    g = _randn(cols, seed=14)
    b = _randn(cols, seed=15)
    y, mean, rstd = hip.layernorm_fwd(x, g, b, 1e-5)
    dy = _randn(rows, cols, seed=16)
    dx, dg, db = hip.layernorm_bwd(dy, x, g, mean, rstd)
    torch.cuda.synchronize()

    x32 = x.float().requires_grad_()
    g32 = g.float().requires_grad_()
    b32 = b.float().requires_grad_()
    y32 = torch.nn.functional.layer_norm(x32, (cols,), g32, b32, 1e-5)
    y32.backward(dy.float())
    _assert_close_bf16(y, y32.detach(), rtol=2e-2)
    _assert_close_bf16(dx, x32.grad, rtol=3e-2)
    _assert_close_bf16(dg, g32.grad, rtol=3e-2, scale=math.sqrt(rows))
    _assert_close_bf16(db, b32.grad, rtol=3e-2, scale=math.sqrt(rows))


def test_softmax_causal_fwd_bwd():
    B, H, S = 2, 3, 256
    s = _randn(B, H, S, S, seed=17)
    scale = 0.125
    p = hip.softmax_fwd(s, scale=scale, causal=True)
    dp = _randn(B, H, S, S, seed=18)
    ds = hip.softmax_bwd(dp, p, scale=scale)
    torch.cuda.synchronize()

    s32 = (s.float() * scale).requires_grad_()
    mask = torch.ones(S, S, dtype=torch.bool, device="cuda").tril()
    sm = s32.masked_fill(~mask, float("-inf"))
    # recompute graph for grads wrt pre-scale scores
    s2 = s.float().requires_grad_()
    p_ref = torch.softmax((s2 * scale).masked_fill(~mask, float("-inf")), -1)
    p_ref.backward(dp.float())
    _assert_close_bf16(p, p_ref.detach(), rtol=2e-2)
    _assert_close_bf16(ds, s2.grad, rtol=2e-2)


def test_attention_fwd_bwd():
    B, H, S, D = 2, 4, 128, 64
    q = _randn(B, H, S, D, seed=19)
    k = _randn(B, H, S, D, seed=20)
    v = _randn(B, H, S, D, seed=21)
    out, p = hip.attention_fwd(q, k, v, causal=True)
    dout = _randn(B, H, S, D, seed=22)
    dq, dk, dv = hip.attention_bwd(dout, q, k, v, p, causal=True)
    torch.cuda.synchronize()

    q2, k2, v2 = (t.float().requires_grad_() for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2,
                                                           is_causal=True)
    ref.backward(dout.float())
    _assert_close_bf16(out, ref.detach(), rtol=3e-2)
    _assert_close_bf16(dq, q2.grad, rtol=4e-2)
    _assert_close_bf16(dk, k2.grad, rtol=4e-2)
    _assert_close_bf16(dv, v2.grad, rtol=4e-2)


def test_embedding_fwd_bwd():
    V, D, n = 1000, 256, 4096
    table = _randn(V, D, seed=23)
    ids = torch.randint(0, V, (n,), device="cuda")
    out = hip.embedding_fwd(ids, table)
    dy = _randn(n, D, seed=24)
    grad = hip.embedding_bwd(dy, ids, V)
    torch.cuda.synchronize()

    t32 = table.float().requires_grad_()
    out_ref = torch.nn.functional.embedding(ids, t32)
    out_ref.backward(dy.float())
    assert torch.equal(out.float(), table[ids].float())
    _assert_close_bf16(grad, t32.grad, rtol=3e-2,
                       scale=torch.tensor(4.0, device="cuda"))


def test_cross_entropy_fwd_bwd():
    M, V = 512, 50304
    logits = _randn(M, V, seed=25)
    targets = torch.randint(0, 50257, (M,), device="cuda")
    targets[5] = -1
    loss, lse = hip.cross_entropy_fwd(logits, targets, -1)
    dlogits = hip.cross_entropy_bwd(torch.ones((), device="cuda"), logits,
                                    targets, lse, -1)
    torch.cuda.synchronize()

    l32 = logits.float().requires_grad_()
    loss_ref = torch.nn.functional.cross_entropy(l32, targets,
                                                 ignore_index=-1)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * loss_ref.item()
    _assert_close_bf16(dlogits, l32.grad, rtol=5e-2,
                       scale=l32.grad.abs().max())


def test_dropout():
    x = torch.ones(1 << 20, dtype=BF16, device="cuda")
    y, mask = hip.dropout_fwd(x, 0.3, seed=7, offset=3)
    y2, mask2 = hip.dropout_fwd(x, 0.3, seed=7, offset=3)
    torch.cuda.synchronize()
    assert torch.equal(mask, mask2), "philox mask not deterministic"
    keep = mask.float().mean().item()
    assert abs(keep - 0.7) < 0.01
    kept_vals = y.float()[mask.bool()]
    assert torch.allclose(kept_vals,
                          torch.full_like(kept_vals, 1 / 0.7), atol=1e-2)
    dy = _randn(1 << 20, seed=26)
    dx = hip.dropout_bwd(dy, mask, 0.3)
    torch.cuda.synchronize()
    ref = dy.float() * mask.float() / 0.7
    _assert_close_bf16(dx, ref, rtol=2e-2)


def test_adamw_matches_torch():
    n = 10007
    g0 = torch.Generator().manual_seed(0)
    p32 = torch.randn(n, generator=g0).cuda()
    p_ref = torch.nn.Parameter(p32.clone())
    opt_ref = torch.optim.AdamW([p_ref], lr=1e-2, betas=(0.9, 0.999),
                                eps=1e-8, weight_decay=0.01)
    param = p32.to(BF16)
    master = p32.clone()
    m = torch.zeros_like(master)
    v = torch.zeros_like(master)
    for step in range(1, 6):
        g = torch.randn(n, generator=torch.Generator().manual_seed(step)).cuda()
        p_ref.grad = g.clone()
        opt_ref.step()
        hip.adamw_step(param, master, g, m, v, lr=1e-2, beta1=0.9,
                       beta2=0.999, eps=1e-8, weight_decay=0.01, step=step)
    torch.cuda.synchronize()
    assert (master - p_ref.detach()).abs().max().item() < 1e-5


# --------------------------------------------------------------------------


def test_gpt2_tiny_gpu_trains():
    from tepdist_amd.models import GPT2, GPT2_CONFIGS
    from tepdist_amd.train import AdamW, Trainer
    cfg = GPT2_CONFIGS["gpt2-test"]
    torch.manual_seed(0)
    model = GPT2(cfg, dtype=BF16).cuda()
    opt = AdamW(model.parameters(), lr=1e-3)
    trainer = Trainer(model, opt)
    g = torch.Generator().manual_seed(42)
    ids = torch.randint(0, cfg.vocab_size, (4, 33), generator=g).cuda()
    batch = (ids[:, :-1], ids[:, 1:])
    losses = [trainer.train_step(lambda i: batch) for _ in range(12)]
    assert losses[-1] < losses[0] * 0.9, losses
    assert all(math.isfinite(l) for l in losses)


def test_tr16_probe_mapping():
    """Documents the MEASURED semantics of ds_read_b64_tr_b16 on gfx950:
    within each 16-lane group, the four QUAD LEADERS' addresses (lanes
    16g+4j) define 4 row bases; lane l reads the (l&3)-th bf16 of each row
    (so data is duplicated across the 4 quads of a group). This is why the
    GEMM's transposed-operand path uses a v_perm register transpose instead
    (see gemm.hip header)."""
    from tepdist_amd.ops import _tepdist_hip as ext
    pat = torch.zeros(256, device="cuda")
    uni = torch.zeros(256, device="cuda")
    ext.tr16_probe(pat.data_ptr(), uni.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pat = pat.reshape(64, 4).cpu().int()
    uni = uni.reshape(64, 4).cpu().int()
    # probe addresses: lane l at element (l&15) + (l>>4)*64
    expect_pat = torch.tensor(
        [[(l >> 4) * 64 + 4 * j + (l & 3) for j in range(4)]
         for l in range(64)], dtype=torch.int32)
    expect_uni = torch.tensor(
        [[l & 3 for _ in range(4)] for l in range(64)], dtype=torch.int32)
    assert torch.equal(pat, expect_pat), f"tr16 pattern mapping:\n{pat}"
    assert torch.equal(uni, expect_uni), f"tr16 uniform mapping:\n{uni}"


@pytest.mark.parametrize("D", [64, 128])
def test_flash_attention_large_vs_sdpa(D):
    """Flash fwd+bwd at benchmark shape (S=1024) vs fp32 SDPA; D=128
    covers the wide-head template (llama-class models)."""
    B, H, S = 4, 8, 1024
    q = _randn(B, H, S, D, seed=40)
    k = _randn(B, H, S, D, seed=41)
    v = _randn(B, H, S, D, seed=42)
    out, res = hip.attention_fwd(q, k, v, causal=True)
    assert len(res) == 2, "flash path should save (out, lse)"
    dout = _randn(B, H, S, D, seed=43)
    dq, dk, dv = hip.attention_bwd(dout, q, k, v, res, causal=True)
    torch.cuda.synchronize()

    q2, k2, v2 = (t.float().requires_grad_() for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2,
                                                           is_causal=True)
    ref.backward(dout.float())
    _assert_close_bf16(out, ref.detach(), rtol=3e-2)
    _assert_close_bf16(dq, q2.grad, rtol=5e-2, scale=q2.grad.abs().max())
    _assert_close_bf16(dk, k2.grad, rtol=5e-2, scale=k2.grad.abs().max())
    _assert_close_bf16(dv, v2.grad, rtol=5e-2, scale=v2.grad.abs().max())


def test_flash_attention_ragged_seq():
    """Non-multiple-of-tile sequence lengths."""
    B, H, S, D = 2, 2, 200, 64
    q = _randn(B, H, S, D, seed=50)
    k = _randn(B, H, S, D, seed=51)
    v = _randn(B, H, S, D, seed=52)
    out, res = hip.attention_fwd(q, k, v, causal=True)
    torch.cuda.synchronize()
    q2, k2, v2 = (t.float() for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2,
                                                           is_causal=True)
    _assert_close_bf16(out, ref, rtol=3e-2)


def test_attention_qkv_packed_matches_split():
    """Packed-qkv flash path (strided kernels, no transposes) vs the 4-D
    API and torch SDPA, fwd+bwd."""
    B, S, H, D = 2, 256, 4, 64
    d = H * D
    g = torch.Generator().manual_seed(60)
    qkv = (torch.randn(B, S, 3 * d, generator=g) * 0.5).to(BF16).cuda()
    qkv.requires_grad_()
    out = ops.attention_qkv(qkv, H, causal=True)
    dout = _randn(B, S, d, seed=61)
    out.backward(dout)
    torch.cuda.synchronize()

    qkv2 = qkv.detach().float().requires_grad_()
    q, k, v = (t.reshape(B, S, H, D).transpose(1, 2)
               for t in qkv2.split(d, dim=-1))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v,
                                                           is_causal=True)
    ref = ref.transpose(1, 2).reshape(B, S, d)
    ref.backward(dout.float())
    _assert_close_bf16(out, ref.detach(), rtol=3e-2)
    _assert_close_bf16(qkv.grad, qkv2.grad, rtol=5e-2,
                       scale=qkv2.grad.abs().max())


def test_transpose_kernel():
    for R, C in ((128, 256), (200, 72), (64, 64), (1000, 1024)):
        x = _randn(R, C, seed=R + C)
        y = hip.transpose2d(x)
        torch.cuda.synchronize()
        assert torch.equal(y.float(), x.float().t())
    xb = _randn(6, 96, 160, seed=70)
    yb = hip.transpose2d(xb)
    torch.cuda.synchronize()
    assert torch.equal(yb.float(), xb.float().transpose(-1, -2))


def test_adamw_multi_tensor_matches_single():
    from tepdist_amd.train import AdamW
    torch.manual_seed(0)
    shapes = [(100, 64), (37,), (513, 16), (1000,), (64, 64), (20000,)]
    params_a = [torch.nn.Parameter(torch.randn(*s).bfloat16().cuda())
                for s in shapes]
    params_b = [torch.nn.Parameter(p.detach().clone()) for p in params_a]
    oa = AdamW(params_a, lr=1e-2)
    ob = AdamW(params_b, lr=1e-2)
    for step in range(3):
        for pa, pb in zip(params_a, params_b):
            g = torch.randn(pa.shape).bfloat16().cuda()
            pa.grad = g.clone()
            pb.grad = g.clone()
        oa.step()                         # multi-tensor path (>=4 cuda bf16)
        ob._mt_key = object()             # poison cache
        saved, ob._try_mt = ob._try_mt, lambda: None  # force per-tensor
        ob.step()
        ob._try_mt = saved
    torch.cuda.synchronize()
    for pa, pb in zip(params_a, params_b):
        torch.testing.assert_close(pa.data.float(), pb.data.float())
        torch.testing.assert_close(oa.state[pa]["master"],
                                   ob.state[pb]["master"], rtol=1e-6,
                                   atol=1e-7)


@pytest.mark.gpu
def test_mlp_fused_epilogue():
    """hipBLASLt fused-epilogue MLP (GELU_AUX_BIAS fwd, DGELU_BGRAD
    dgrad) vs the fp32 tanh-gelu reference: values and all five grads."""
    from tepdist_amd.ops import hip
    if hip._blt is None:
        pytest.skip("blaslt extension not built")
    if hip._blt.probe_epilogues(256, 256, 256)["gelu_aux_bias_bf16"] <= 0:
        # measured: hipBLASLt 1.2.7 offers no algos for ANY aux epilogue
        # on gfx950 (profiles/blaslt_epilogue_probe.md) — ops.mlp then
        # permanently falls back to the composed path, which the rest of
        # the GPU suite covers
        pytest.skip("hipblaslt lacks aux epilogues on this stack")
    torch.manual_seed(0)
    T, d = 1024, 256
    mk = lambda *s: (torch.randn(*s, device="cuda", dtype=torch.bfloat16)
                     * 0.05).requires_grad_()
    x, w1, b1 = mk(T, d), mk(4 * d, d), mk(4 * d)
    w2, b2 = mk(d, 4 * d), mk(d)
    dy = torch.randn(T, d, device="cuda", dtype=torch.bfloat16)

    old = hip._MLP_FUSED
    hip._MLP_FUSED = "1"
    try:
        from tepdist_amd import ops
        y = ops.mlp(x, w1, b1, w2, b2)
        y.backward(dy)
    finally:
        hip._MLP_FUSED = old

    xf, w1f, b1f, w2f, b2f = (t.detach().float().clone().requires_grad_()
                              for t in (x, w1, b1, w2, b2))
    h = torch.nn.functional.gelu(xf @ w1f.t() + b1f, approximate="tanh")
    ref = h @ w2f.t() + b2f
    ref.backward(dy.float())

    torch.testing.assert_close(y.float(), ref, rtol=3e-2, atol=3e-2)
    for got, want, name in ((x.grad, xf.grad, "dx"),
                            (w1.grad, w1f.grad, "dw1"),
                            (b1.grad, b1f.grad, "db1"),
                            (w2.grad, w2f.grad, "dw2"),
                            (b2.grad, b2f.grad, "db2")):
        torch.testing.assert_close(got.float(), want, rtol=5e-2,
                                   atol=5e-2, msg=name)


@pytest.mark.gpu
def test_add_layernorm_fused():
    """Fused residual add + layernorm vs fp32 composed reference:
    forward sum + normed output, and x/res/gamma/beta grads with the sum
    consumed by a second path (exercises the fused dsum accumulation)."""
    from tepdist_amd import ops
    torch.manual_seed(0)
    R, C = 512, 1024
    x = torch.randn(R, C, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    r = torch.randn(R, C, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    g = (1 + 0.1 * torch.randn(C, device="cuda")).bfloat16() \
        .requires_grad_()
    b = (0.1 * torch.randn(C, device="cuda")).bfloat16().requires_grad_()
    s, y = ops.add_layernorm(x, r, g, b)
    (y.float().sum() + (s.float() ** 2).sum()).backward()

    xf, rf, gf, bf = (t.detach().float().clone().requires_grad_()
                      for t in (x, r, g, b))
    sf = xf + rf
    yf = torch.nn.functional.layer_norm(sf, (C,), gf, bf, 1e-5)
    (yf.sum() + (sf ** 2).sum()).backward()

    torch.testing.assert_close(s.float(), sf, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(y.float(), yf, rtol=2e-2, atol=3e-2)
    torch.testing.assert_close(x.grad.float(), xf.grad, rtol=5e-2,
                               atol=2e-1)
    torch.testing.assert_close(r.grad.float(), rf.grad, rtol=5e-2,
                               atol=2e-1)
    torch.testing.assert_close(g.grad.float(), gf.grad, rtol=5e-2,
                               atol=5e-1)
    torch.testing.assert_close(b.grad.float(), bf.grad, rtol=5e-2,
                               atol=5e-1)


@pytest.mark.gpu
def test_add_layernorm_sum_only_grad():
    """When the normalized output is unused, backward routes the sum
    gradient straight through (the None-dy branch)."""
    from tepdist_amd import ops
    x = torch.randn(64, 128, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    r = torch.randn(64, 128, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    g = torch.ones(128, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(128, device="cuda", dtype=torch.bfloat16)
    s, _y = ops.add_layernorm(x, r, g, b)
    s.float().sum().backward()
    torch.testing.assert_close(x.grad.float(),
                               torch.ones(64, 128, device="cuda"))


@pytest.mark.gpu
def test_gemm_dgelu_epilogue():
    """256-schedule GEMM with the dgelu epilogue: C = (A@B) * gelu'(aux)
    vs fp32 autograd through tanh-gelu."""
    M, N, K = 512, 256, 128
    a = _randn(M, K, seed=31)
    b = _randn(N, K, seed=32)
    pre = _randn(M, N, seed=33)
    dh, _ = hip._gemm_raw(a, b, True, True, M, N, K, K, K, 0, 0, 1,
                          epi=4, out_pre=pre)
    torch.cuda.synchronize()
    up = a.float() @ b.float().t()
    p32 = pre.float().requires_grad_()
    torch.nn.functional.gelu(p32, approximate="tanh").backward(up)
    _assert_close_bf16(dh, p32.grad, rtol=3e-2, scale=math.sqrt(K))


@pytest.mark.gpu
def test_mlp_hand_dgelu_backward():
    """ops.mlp backward with the hand dgelu-epilogue dgrad (pinned via
    TEPDIST_GEMM_BACKEND=hip) vs the fp32 reference."""
    torch.manual_seed(0)
    T, d = 512, 256
    mk = lambda *s: (torch.randn(*s, device="cuda", dtype=torch.bfloat16)
                     * 0.05).requires_grad_()
    x, w1, b1 = mk(T, d), mk(4 * d, d), mk(4 * d)
    w2, b2 = mk(d, 4 * d), mk(d)
    dy = torch.randn(T, d, device="cuda", dtype=torch.bfloat16)
    old = hip._GEMM_BACKEND
    hip._GEMM_BACKEND = "hip"
    try:
        from tepdist_amd import ops
        y = ops.mlp(x, w1, b1, w2, b2)
        y.backward(dy)
    finally:
        hip._GEMM_BACKEND = old
    xf, w1f, b1f, w2f, b2f = (t.detach().float().clone().requires_grad_()
                              for t in (x, w1, b1, w2, b2))
    h = torch.nn.functional.gelu(xf @ w1f.t() + b1f, approximate="tanh")
    ref = h @ w2f.t() + b2f
    ref.backward(dy.float())
    torch.testing.assert_close(y.float(), ref, rtol=3e-2, atol=3e-2)
    for got, want, name in ((x.grad, xf.grad, "dx"),
                            (w1.grad, w1f.grad, "dw1"),
                            (b1.grad, b1f.grad, "db1"),
                            (w2.grad, w2f.grad, "dw2"),
                            (b2.grad, b2f.grad, "db2")):
        torch.testing.assert_close(got.float(), want, rtol=5e-2,
                                   atol=5e-2, msg=name)
