"""ops.linear_decode / ops.swiglu_linear_decode (csrc/skinny_gemm.hip) and
the engine's decode_linear modes, on the GPU.

Exact cases: x holds integers in [-8, 8], W integers in [-8, 8] times 2^-3,
bias and residual small integers times 2^-3. Every product and partial sum
is an integer multiple of 2^-3 below 64 K < 2^24 units, so every fp32 sum
is exact in any order and the output must be the fp64 result rounded once
to bf16, bit for bit. Activations use the same construction scaled to
pre-activations within about [-12, 12] (exact again) and are held to the
floors of the standalone kernels (rowwise_checks.check_gelu/check_swiglu).
Random data is held to 1 bf16 ulp + K 2^-24 sum|x||w|, the standard fp32
accumulation bound."""

import itertools

import pytest
import torch

import rowwise_checks as rc
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPIS = ["none", "bias", "residual", "bias+residual"]
# M: fragment edges, zero-filled token rows, each MT. N: one tile, ragged
# tile, N % 4 != 0, several blocks plus a ragged last one. K: one K-step,
# waves with unequal shares, several load groups per wave.
CASES = list(itertools.product([1, 15, 16, 17, 33, 64], [16, 40, 503, 2064],
                               [64, 192, 1088], EPIS))[::7]


def _ints(g, *shape, scale=1.0, lim=8):
    return (torch.randint(-lim, lim + 1, shape, generator=g) * scale).to(BF16)


def _operands(M, N, K, seed, wscale=2.0 ** -3):
    g = rc.gen(seed)
    return (_ints(g, M, K), _ints(g, N, K, scale=wscale),
            _ints(g, N, scale=2.0 ** -3, lim=40),
            _ints(g, M, N, scale=2.0 ** -3, lim=40))


def _exact(x, w, bias=None, res=None):
    y = o.f64(x) @ o.f64(w).t()
    if bias is not None:
        y = y + o.f64(bias)
    if res is not None:
        y = y + o.f64(res)
    return y


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize("M,N,K,epi", CASES)
def test_exact(M, N, K, epi):
    x, w, b, r = _operands(M, N, K, M * N + K)
    b = b if "bias" in epi else None
    r = r if "residual" in epi else None
    xd, wd, bd, rd = _cuda(x, w, b, r)
    got = ops.linear_decode(xd, wd, bd, residual=rd)
    rc.assert_bits_equal(got.cpu(), _exact(x, w, b, r).to(BF16),
                         f"linear_decode[{M},{N},{K},{epi}]")


@pytest.mark.parametrize("view", ["w", "x", "residual"])
def test_exact_strided_views(view):
    M, N, K = 17, 40, 192
    x, w, b, r = _operands(M, N, K, 5)
    xd, wd, bd, rd = _cuda(x, w, b, r)
    if view == "w":      # a column slice: row stride K + 128
        wd = torch.zeros(N, K + 128, dtype=BF16, device="cuda")[:, 64:64 + K]
        wd.copy_(w)
    elif view == "x":
        xd = torch.zeros(M, K + 16, dtype=BF16, device="cuda")[:, 8:8 + K]
        xd.copy_(x)
    else:                # a row slice: every other row of a taller tensor
        rd = torch.zeros(2 * M, N, dtype=BF16, device="cuda")[1::2]
        rd.copy_(r)
    assert not (wd.is_contiguous() and xd.is_contiguous()
                and rd.is_contiguous())
    got = ops.linear_decode(xd, wd, bd, residual=rd)
    rc.assert_bits_equal(got.cpu(), _exact(x, w, b, r).to(BF16), view)


def test_placement():
    """One-hot weight rows select single x values: a wrong k-permutation or
    a row/column mix-up moves a value. x[m, k] are distinct bf16 values
    (mantissa from k % 128, exponent from m and k // 128)."""
    M, N, K = 17, 40, 192
    k = torch.arange(K)
    x = ((1.0 + (k % 128) / 128.0)[None, :]
         * 2.0 ** (2 * torch.arange(M)[:, None] + k[None, :] // 128 - 20.0))
    assert x.unique().numel() == M * K
    sel = (torch.arange(N) * 37 + 5) % K
    w = torch.zeros(N, K)
    w[torch.arange(N), sel] = 1.0
    got = ops.linear_decode(x.to(BF16).cuda(), w.to(BF16).cuda())
    rc.assert_bits_equal(got.cpu(), x[:, sel].to(BF16), "placement")


@pytest.mark.parametrize("M,N,K", [(17, 40, 192), (64, 503, 1088)])
def test_activations(M, N, K):
    # sums of K products of integers in [-8, 8]: sigma ~ 27 sqrt(K); the
    # weight scale brings 4 sigma to about 12
    ws = 2.0 ** -7 if K == 192 else 2.0 ** -8
    x, w, b, _ = _operands(M, N, K, 3, wscale=ws)
    _, w_up, _, _ = _operands(M, N, K, 4, wscale=ws)
    xd, wd, bd, ud = _cuda(x, w, b, w_up)
    a = _exact(x, w, b)
    print(f"gelu pre-activations in [{a.min():.2f}, {a.max():.2f}]")
    o.assert_within_ulp(ops.linear_decode(xd, wd, bd, act="gelu").cpu(),
                        o.gelu_fwd(a), rc.ELEM * a.abs().clamp_min(1.0),
                        "bias+gelu")
    gt, up = _exact(x, w), _exact(x, w_up)
    o.assert_within_ulp(ops.swiglu_linear_decode(xd, wd, ud).cpu(),
                        o.swiglu_fwd(gt, up),
                        rc.ELEM * gt.abs().clamp_min(1.0) * up.abs(),
                        "swiglu")


@pytest.mark.parametrize("M,N,K", [(33, 503, 1088), (8, 2064, 192)])
def test_random(M, N, K):
    g = rc.gen(M + N)
    x, w = rc.randn(g, M, K), rc.randn(g, N, K, scale=K ** -0.5)
    floor = K * 2.0 ** -24 * (o.f64(x).abs() @ o.f64(w).abs().t())
    o.assert_within_ulp(ops.linear_decode(x.cuda(), w.cuda()).cpu(),
                        _exact(x, w), floor, "randn")


def test_repeat_and_graph_replay():
    M, N, K = 33, 503, 1088
    g = rc.gen(9)
    x, w, r = (rc.randn(g, *s).cuda() for s in ((M, K), (N, K), (M, N)))

    def call():
        return ops.linear_decode(x, w, residual=r)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc.assert_bits_equal(call(), call(), "two eager calls")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in range(3):
        for t in (x, w, r):
            t.copy_(rc.randn(g, *t.shape))
        graph.replay()
        rc.assert_bits_equal(out, call(), f"replay {i}")


# -- engine: the two-layer models of the decode-attention tests --------------

def _model(kind):
    torch.manual_seed(0)
    if kind == "llama":
        from tepdist_amd.models.llama import Llama, LlamaConfig
        cfg = LlamaConfig("decode-linear-test", n_layer=2, n_embd=256,
                          n_head=4, n_ctx=64, vocab_size=503, n_kv_head=2)
        return cfg, Llama(cfg, dtype=BF16).cuda().eval()
    from tepdist_amd.models import GPT2
    from tepdist_amd.models.configs import GPT2Config
    cfg = GPT2Config("decode-linear-test", n_layer=2, n_embd=128, n_head=2,
                     n_ctx=64, vocab_size=503)
    return cfg, GPT2(cfg, dtype=BF16).cuda().eval()


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_step_auto_matches_gemm(kind):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ga = Generator(model, decode_linear="auto")
    gg = Generator(model, decode_linear="gemm")
    S0, D = 12, cfg.n_embd // cfg.n_head
    # one sequence: at M = 1 "auto" takes every site, the ragged head too
    ids = torch.randint(0, cfg.vocab_size, (1, S0 + 1), device="cuda")
    kc = [torch.zeros(1, gg.kv_heads, 32, D, dtype=BF16, device="cuda")
          for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    with torch.no_grad():
        gg._stack(gg._embed(ids[:, :S0], torch.arange(S0, device="cuda")),
                  kc, vc, 0)
        x1 = gg._embed(ids[:, S0:], torch.tensor([S0], device="cuda"))
        ka, va = [t.clone() for t in kc], [t.clone() for t in vc]
        ha, hg = ga._stack(x1, ka, va, S0), gg._stack(x1, kc, vc, S0)
        la, lg = ga._logits(ha), gg._logits(hg)
    for got, want, what in ((ha, hg, "hidden"), (la, lg, "logits")):
        err = (got.float() - want.float()).abs().max().item()
        bound = 3e-2 * want.float().abs().max().item()
        print(f"{kind} {what}: max err {err:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_generate_graph_equals_eager(kind, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, decode_linear="auto")
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)


def test_engine_modes():
    from tepdist_amd.inference import Generator
    cfg, model = _model("gpt2")
    with pytest.raises(ValueError, match="decode_linear"):
        Generator(model, decode_linear="fast")
    x = torch.zeros(65, 1, cfg.n_embd, dtype=BF16, device="cuda")  # M = 65
    with torch.no_grad():
        with pytest.raises(ValueError, match="not covered"):
            Generator(model, decode_linear="skinny")._logits(x)
        ya = Generator(model, decode_linear="auto")._logits(x)
        yg = Generator(model, decode_linear="gemm")._logits(x)
    assert torch.equal(ya, yg)
