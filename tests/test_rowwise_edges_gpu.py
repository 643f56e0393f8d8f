"""The row and elementwise HIP kernels at their edges, against float64
oracles (tepdist_amd/ops/fp64_reference.py) under the bound
|got - fp64| <= 1 ulp + floor.

The shapes are the smallest that reach each branch of the launchers in
ops/csrc: every NV of the LayerNorm / RMSNorm (1..6) and softmax (1..4)
template dispatch with a partial last vector group, the cols % 8 tail and
cols < 8; rows past each grid cap, so the grid-stride loops and the
cross-row dgamma/dbeta accumulation run (LN bwd above 1024 waves, LN/softmax
/embedding fwd and RMSNorm bwd above 8192, CE above 2048 rows, dropout and
AdamW above 2 Mi elements, SwiGLU 4 Mi, GELU 8 Mi, RoPE 1 Mi pairs, the
embedding scatter 512 Ki); the over-limit throws. Odd cols put rows off a
16-byte boundary on purpose.

Inputs, floors and their derivations live in tests/rowwise_checks.py, which
tests/test_fp64_reference_cpu.py runs with ops/reference.py on the CPU.
"""

import pytest
import torch

import rowwise_checks as rc
from tepdist_amd.ops import fp64_reference as o

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from tepdist_amd.ops import hip as be
    yield be
    # the figures of docs/KERNELS.md (shown with pytest -s)
    print("\noutput: largest error in ulps where nothing cancels / anywhere"
          " / as a fraction of 1 ulp + floor")
    for key, (plain, anywhere, frac) in rc.MEASURED.items():
        print(f"{key:20s} {plain:6.3f} {anywhere:10.1f} {frac:6.3f}")


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


# --------------------------------------------------------------------------
# LayerNorm, add + LayerNorm, RMSNorm
# --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ln", "add", "add_dsum"])
@pytest.mark.parametrize("cols", rc.NORM_COLS)
def test_layernorm_cols(hip, cols, mode):
    rc.check_layernorm(hip, DEV, 9, cols, mode=mode)


# 1030 rows: above the 1024 backward waves, so waves 0..5 take two rows and
# the reduce kernel sums 1024 partials; 8200: above the forward's 8192
@pytest.mark.parametrize("mode", ["ln", "add", "add_dsum"])
@pytest.mark.parametrize("rows,gamma", [(1, "near1"), (9, "randn"),
                                        (1030, "near1"), (1030, "randn"),
                                        (8200, "near1")])
def test_layernorm_rows(hip, rows, gamma, mode):
    rc.check_layernorm(hip, DEV, rows, 72, gamma=gamma, mode=mode)


@pytest.mark.parametrize("cols", rc.NORM_COLS)
def test_rmsnorm_cols(hip, cols):
    rc.check_rmsnorm(hip, DEV, 9, cols)


# rmsnorm_bwd launches min(rows rounded up to 4, 8192) waves: only 8200
# rows enter its row loop
@pytest.mark.parametrize("rows,gamma", [(1, "near1"), (9, "randn"),
                                        (8200, "near1"), (8200, "randn")])
def test_rmsnorm_rows(hip, rows, gamma):
    rc.check_rmsnorm(hip, DEV, rows, 72, gamma=gamma)


def test_norm_cols_over_limit_raise(hip):
    x, res, dy = _dev(*(rc.randn(rc.gen(i), 9, 3073) for i in range(3)))
    g, b = _dev(rc.randn(rc.gen(3), 3073), rc.randn(rc.gen(4), 3073))
    mean = torch.zeros(9, device=DEV)
    rstd = torch.ones(9, device=DEV)
    with pytest.raises(RuntimeError, match="3072"):
        hip.layernorm_fwd(x, g, b)
    with pytest.raises(RuntimeError, match="3072"):
        hip.add_layernorm_fwd(x, res, g, b)
    with pytest.raises(RuntimeError, match="3072"):
        hip.layernorm_bwd(dy, x, g, mean, rstd)
    with pytest.raises(RuntimeError, match="3072"):
        hip.add_layernorm_bwd(dy, res, x, g, mean, rstd)
    with pytest.raises(RuntimeError, match="cols too large"):
        hip.rmsnorm_fwd(x, g)
    with pytest.raises(RuntimeError, match="cols too large"):
        hip.rmsnorm_bwd(dy, x, g, rstd)
    torch.cuda.synchronize()      # nothing was launched, nothing pending


# --------------------------------------------------------------------------
# Softmax
# --------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("sq,sk", rc.SOFTMAX_SHAPES)
def test_softmax_shapes(hip, sq, sk, causal):
    rc.check_softmax(hip, DEV, 3, sq, sk, causal)


# 114 * 72 = 8208 rows: above the 8192 waves of the launch, the row loop
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("kind,bh,scale", [("randn", 114, 0.125),
                                           ("pm80", 3, 1.0),
                                           ("const", 3, 0.125)])
def test_softmax_inputs(hip, kind, bh, scale, causal):
    rc.check_softmax(hip, DEV, bh, 72, 72, causal, scale=scale, kind=kind)


def test_softmax_more_queries_than_keys(hip):
    # without the mask any shape is fine ...
    rc.check_softmax(hip, DEV, 3, 9, 5, causal=False)
    # ... with it the first sq - sk queries would see no key: the wrapper
    # refuses (the kernel returned NaN rows silently)
    x = rc.softmax_scores(3, 9, 5).to(DEV)
    with pytest.raises(ValueError, match="sq <= sk"):
        hip.softmax_fwd(x, scale=1.0, causal=True)


def test_softmax_cols_over_limit_raise(hip):
    x = rc.softmax_scores(1, 3, 2049).to(DEV)
    with pytest.raises(RuntimeError, match="2048"):
        hip.softmax_fwd(x, scale=1.0, causal=False)
    with pytest.raises(RuntimeError, match="2048"):
        hip.softmax_bwd(x, x, scale=1.0)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", rc.CE_PATTERNS)
@pytest.mark.parametrize("rows,cols", rc.CE_SHAPES)
def test_cross_entropy(hip, rows, cols, pattern):
    rc.check_cross_entropy(hip, DEV, rows, cols, pattern)


def test_cross_entropy_pad_id_rows_add_no_loss(hip):
    """The defect: with ignore_index = 0 the forward added the ignored
    rows' losses while n and the backward left them out."""
    g = rc.gen(3)
    logits = rc.randn(g, 33, 520, scale=3.0)
    t = torch.randint(1, 520, (33,), generator=g)
    base, _ = hip.cross_entropy_fwd(logits.to(DEV), t.to(DEV), 0)
    # rows 5.. become padding: the loss is the mean over rows 0..4 alone
    t2 = t.clone()
    t2[5:] = 0
    loss, _ = hip.cross_entropy_fwd(logits.to(DEV), t2.to(DEV), 0)
    ref5, _, _ = o.cross_entropy_fwd(logits[:5], t[:5], 0)
    rc.judge(loss.reshape(()), ref5.reshape(()), 2.0 ** -18 * ref5.abs(),
             "ce_fwd.loss[pad rows]")
    assert float(base) != float(loss)


# --------------------------------------------------------------------------
# Embedding
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [8, 64, 100, 1026])
def test_embedding_fwd_exact(hip, dim):
    vocab, n = 300, 8200          # 8200 ids: above the 8192 waves
    g = rc.gen(dim)
    table = rc.randn(g, vocab, dim)
    ids = torch.randint(0, vocab, (n,), generator=g)
    ids[0], ids[1], ids[-1] = 0, vocab - 1, vocab - 1
    out = hip.embedding_fwd(ids.to(DEV), table.to(DEV))
    rc.assert_bits_equal(out, table[ids], f"embedding_fwd[{n}x{dim}]")


# equal: 4096 atomic adds into one row; 8200 x 64 = 524 800 elements, above
# the scatter's 512 Ki threads; 1026: dim % 8 != 0
@pytest.mark.parametrize("n,dim,vocab,pattern", [
    (4096, 8, 16, "equal"), (100, 100, 101, "distinct"),
    (8200, 64, 300, "random"), (600, 1026, 50, "random")])
def test_embedding_bwd(hip, n, dim, vocab, pattern):
    rc.check_embedding_bwd(hip, DEV, n, dim, vocab, pattern)


# --------------------------------------------------------------------------
# Dropout
# --------------------------------------------------------------------------

@pytest.mark.parametrize("seed,offset", [((5 << 32) + 17, 0),
                                         ((1 << 40) + 3, (1 << 33) + 9)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2 * 2 ** 20 + 5])
def test_dropout_is_the_philox_mask(hip, n, p, seed, offset):
    x = rc.randn(rc.gen(n), n, scale=2.0)
    y, mask = hip.dropout_fwd(x.to(DEV), p, seed, offset)
    want = rc.np_mask(n, p, seed, offset)
    assert mask.dtype == torch.uint8
    assert torch.equal(mask.cpu(), want), \
        f"{int((mask.cpu() != want).sum())} of {n} mask elements differ"
    rc.assert_bits_equal(y, o.dropout_apply(x, want, p), "dropout_fwd.y")
    dy = rc.randn(rc.gen(n + 1), n)
    dx = hip.dropout_bwd(dy.to(DEV), mask, p)
    rc.assert_bits_equal(dx, o.dropout_apply(dy, want, p), "dropout_bwd.dx")


# --------------------------------------------------------------------------
# GELU, SwiGLU, RoPE, bias sum
# --------------------------------------------------------------------------

@pytest.mark.parametrize("n", rc.ELEMWISE_N + [8 * 2 ** 20 + 3])
def test_gelu(hip, n):
    rc.check_gelu(hip, DEV, n)


@pytest.mark.parametrize("n", rc.ELEMWISE_N + [4 * 2 ** 20 + 3])
def test_swiglu(hip, n):
    rc.check_swiglu(hip, DEV, n)


@pytest.mark.parametrize("theta", [10000.0, 500000.0])
@pytest.mark.parametrize("tokens,seq_len", [(64, 64), (100, 33),
                                            (2048, 2048)])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
def test_rope(hip, D, heads, tokens, seq_len, theta):
    rc.check_rope(hip, DEV, tokens, heads, D, seq_len, theta)


def test_rope_loops(hip):
    # 8200 * 4 * 32 = 1 049 600 pairs: above the 4096 * 256 threads
    rc.check_rope(hip, DEV, 8200, 4, 64, 2048, 10000.0)


# 512 and 1024 take the streaming kernel (4099 rows over 260 waves, 1000
# over 64: neither divides), the rest the fallback: 520 has a full last
# group and 32 row slices of 1000 rows, 100 a cols % 8 tail, 8 one group
@pytest.mark.parametrize("rows,cols", rc.BIAS_SHAPES)
def test_bias_sum(hip, rows, cols):
    rc.check_bias_sum(hip._bias_sum, DEV, rows, cols)


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

STD_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


@pytest.mark.parametrize("n", [3, 10007, 2 * 2 ** 20 + 1])
def test_adamw_fp32_grad(hip, n):
    rc.check_adamw_single(hip, DEV, n)


def test_adamw_fp32_grad_usual_hyperparameters(hip):
    rc.check_adamw_single(hip, DEV, 10007, hp=STD_HP)


def _mt_params(g):
    """bf16 and fp32 parameters; 16384 = one chunk exactly, 16385 = a
    second chunk of one element, 3 = less than one vector."""
    shapes = [((128, 128), BF16), ((16385,), BF16), ((3,), BF16),
              ((10, 10), torch.float32), ((5,), torch.float32),
              ((40000,), BF16)]
    return [torch.nn.Parameter(
        torch.randn(*s, generator=g).to(dt).to(DEV)) for s, dt in shapes]


@pytest.mark.parametrize("hp", [rc.ADAMW_HP, STD_HP], ids=["dyadic", "usual"])
def test_adamw_multi_tensor_eager_and_graph_path(hip, hp):
    from tepdist_amd.train import AdamW
    kw = dict(lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
              weight_decay=hp["weight_decay"])
    pa, pb = _mt_params(rc.gen(1)), _mt_params(rc.gen(1))
    eager, graph = AdamW(pa, **kw), AdamW(pb, **kw)
    g = rc.gen(2)
    for p in pa + pb:
        p.grad = torch.zeros_like(p)
    graph.prepare_graph()
    for step in range(1, 4):
        grads = [rc.adamw_grad(g, p.numel(), p.dtype).reshape(p.shape)
                 for p in pa]
        before = [tuple(eager.state[p][k].detach().cpu().clone()
                        for k in ("master", "exp_avg", "exp_avg_sq"))
                  for p in pa]
        for p, q, gr in zip(pa, pb, grads):
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        eager.step()
        graph.refresh_hyper()
        graph.step()
        assert eager._mt is not None and graph.graph_mode
        for i, (p, q) in enumerate(zip(pa, pb)):
            st, sq = eager.state[p], graph.state[q]
            wd = 0.0 if p.dim() == 1 else hp["weight_decay"]
            rc.adamw_judge(
                (p.data, st["master"], st["exp_avg"], st["exp_avg_sq"]),
                before[i], grads[i], dict(hp, weight_decay=wd), step,
                f"[mt tensor {i} {tuple(p.shape)} step {step}]")
            # the graph path: same kernel, hyper-parameters from the
            # device buffer; must be the eager step bit for bit
            for a, b, name in [(p.data, q.data, "param")] + \
                    [(st[k], sq[k], k) for k in st]:
                assert torch.equal(a, b), \
                    f"graph != eager: tensor {i} {name} step {step}: " \
                    f"{int((a != b).sum())} of {a.numel()} differ"
