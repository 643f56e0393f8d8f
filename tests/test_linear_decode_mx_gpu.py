"""ops.linear_decode_mx / ops.swiglu_linear_decode_mx / ops.mx_dequantize
(csrc/skinny_mx_gemm.hip) and the engine's weight_format, on the GPU. The
reference is always fp64 on mx.dequantize_ref(mw).

Exact cases, by the method of test_linear_decode_gpu.py: x holds integers in
[-8, 8]; W codes are the table values that are multiples of 2^-3 with
|v| <= 8, under block scales 2^-2 .. 2^1, so dq(W) is a multiple of 2^-5
with |w| <= 16; bias and residual are integers times 2^-3. Every product is
an integer multiple of 2^-5 of at most 8 * 16 * 2^5 = 2^12 units, and a sum
over K <= 1152 of them stays below 1152 * 2^12 < 2^23 units (bias and
residual add 320 more), under 2^24: every fp32 partial sum is exact in any
order, and the output must be the fp64 result rounded once to bf16, bit for
bit. The activation cases use scales 2^-9 .. 2^-7 (the same count of units,
pre-activations within about [-12, 12]) and the floors of the standalone
kernels. Random data is held to 1 bf16 ulp + K 2^-24 sum|x||dq(w)|."""

import copy
import itertools

import pytest
import torch

import rowwise_checks as rc
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import mx

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FMTS = ["mxfp8", "mxfp4"]
EPIS = ["none", "bias", "residual", "bias+residual"]
# M: fragment edges, zero-filled token rows, each MT. N: one tile, a ragged
# tile, N % 4 != 0 over several blocks. K: one K-step, waves with unequal
# shares, more steps than waves.
CASES = list(itertools.product([1, 16, 17, 33, 64], [16, 40, 503],
                               [128, 384, 1152], EPIS))[::7]
# the 32-row head path (>= 1024 tiles) with a ragged last tile
CASES.append((17, 16400, 128, "bias+residual"))


def _pack(codes, scales, fmt):
    """MXWeight of unpacked codes [N, K] and scale bytes [N, K / 32]."""
    N, K = codes.shape
    if fmt == "mxfp4":
        codes = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return mx.MXWeight(codes.contiguous(), scales.to(torch.uint8), fmt, (N, K))


def _valid(fmt, eighths=False):
    """The non-NaN codes; eighths: those worth a multiple of 2^-3 <= 8."""
    t = mx.table(fmt).double()
    ok = ~t.isnan()
    if eighths:
        ok &= (t * 8 == (t * 8).round()) & (t.abs() <= 8)
    return torch.arange(t.numel(), dtype=torch.uint8)[ok]


def _int_weight(g, N, K, fmt, exps=(-2, 1)):
    pool = _valid(fmt, eighths=True)
    codes = pool[torch.randint(0, pool.numel(), (N, K), generator=g)]
    scales = 127 + torch.randint(exps[0], exps[1] + 1, (N, K // 32),
                                 generator=g)
    return _pack(codes, scales, fmt)


def _ints(g, *shape, scale=1.0, lim=8):
    return (torch.randint(-lim, lim + 1, shape, generator=g) * scale).to(BF16)


def _operands(M, N, K, fmt, seed, exps=(-2, 1)):
    g = rc.gen(seed)
    return (_ints(g, M, K), _int_weight(g, N, K, fmt, exps),
            _ints(g, N, scale=2.0 ** -3, lim=40),
            _ints(g, M, N, scale=2.0 ** -3, lim=40))


def _exact(x, mw, bias=None, res=None):
    y = o.f64(x) @ o.f64(mx.dequantize_ref(mw)).t()
    if bias is not None:
        y = y + o.f64(bias)
    if res is not None:
        y = y + o.f64(res)
    return y


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize("fmt", FMTS)
def test_dequantize_every_code(fmt):
    """Every code at scale bytes {low clamp, 120, 127, 130, high clamp} on a
    ragged shape: block b takes scale b % 5 and the next 32 codes of its
    scale's own cycle through the code list."""
    N, K = 40, 384
    lo, hi = mx.scale_byte_range(fmt)
    pool = _valid(fmt)
    b = torch.arange(N * K // 32)
    scales = torch.tensor([lo, 120, 127, 130, hi])[b % 5]
    codes = pool[(32 * (b // 5)[:, None] + torch.arange(32)) % pool.numel()]
    assert all(codes[b % 5 == s].unique().numel() == pool.numel()
               for s in range(5))
    mw = _pack(codes.reshape(N, K), scales.reshape(N, K // 32), fmt)
    want = mx.dequantize_ref(mw)
    rc.assert_bits_equal(ops.mx_dequantize(mw.cuda()).cpu(), want, fmt)
    out = torch.zeros(N, K, dtype=BF16, device="cuda")
    assert ops.mx_dequantize(mw.cuda(), out=out) is out
    rc.assert_bits_equal(out.cpu(), want, f"{fmt} out=")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K,epi", CASES)
def test_exact(M, N, K, epi, fmt):
    x, mw, b, r = _operands(M, N, K, fmt, M * N + K)
    b = b if "bias" in epi else None
    r = r if "residual" in epi else None
    xd, bd, rd = _cuda(x, b, r)
    got = ops.linear_decode_mx(xd, mw.cuda(), bd, residual=rd)
    rc.assert_bits_equal(got.cpu(), _exact(x, mw, b, r).to(BF16),
                         f"linear_decode_mx[{fmt},{M},{N},{K},{epi}]")


@pytest.mark.parametrize("fmt", FMTS)
def test_placement(fmt):
    """One-hot weight rows (the code of 1.0) under a scale that changes with
    row and block select single x values times a power of two: a wrong
    nibble order, k permutation, lane-to-block map or scale byte moves a
    value. x[m, k] are distinct bf16 values (mantissa from k % 128, exponent
    from m and k // 128)."""
    M, N, K = 17, 40, 384
    k = torch.arange(K)
    x = ((1.0 + (k % 128) / 128.0)[None, :]
         * 2.0 ** (3 * torch.arange(M)[:, None] + k[None, :] // 128 - 26.0))
    assert x.unique().numel() == M * K
    n = torch.arange(N)
    sel = (n * 37 + 5) % K
    s = (5 * n[:, None] + 3 * torch.arange(K // 32)[None, :]) % 11 - 5
    one = int((mx.table(fmt) == 1.0).nonzero()[0])
    codes = torch.zeros(N, K, dtype=torch.uint8)
    codes[n, sel] = one
    got = ops.linear_decode_mx(x.to(BF16).cuda(),
                               _pack(codes, 127 + s, fmt).cuda())
    want = x[:, sel] * 2.0 ** s[n, sel // 32].double()[None, :]
    rc.assert_bits_equal(got.cpu(), want.to(BF16), f"placement {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
def test_activations_and_dual(fmt):
    M, N, K = 17, 40, 384
    x, mw, b, _ = _operands(M, N, K, fmt, 3, exps=(-9, -7))
    _, mu, _, _ = _operands(M, N, K, fmt, 4, exps=(-9, -7))
    xd, bd = _cuda(x, b)
    a = _exact(x, mw, b)
    print(f"gelu pre-activations in [{a.min():.2f}, {a.max():.2f}]")
    o.assert_within_ulp(
        ops.linear_decode_mx(xd, mw.cuda(), bd, act="gelu").cpu(),
        o.gelu_fwd(a), rc.ELEM * a.abs().clamp_min(1.0), "bias+gelu")
    gt, up = _exact(x, mw), _exact(x, mu)
    o.assert_within_ulp(
        ops.swiglu_linear_decode_mx(xd, mw.cuda(), mu.cuda()).cpu(),
        o.swiglu_fwd(gt, up), rc.ELEM * gt.abs().clamp_min(1.0) * up.abs(),
        "swiglu")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K", [(33, 503, 1152), (8, 2064, 384)])
def test_random(M, N, K, fmt):
    g = rc.gen(M + N)
    x = rc.randn(g, M, K)
    mw = ops.mx_quantize(rc.randn(g, N, K, scale=K ** -0.5), fmt)
    w64 = o.f64(mx.dequantize_ref(mw))
    floor = K * 2.0 ** -24 * (o.f64(x).abs() @ w64.abs().t())
    o.assert_within_ulp(ops.linear_decode_mx(x.cuda(), mw.cuda()).cpu(),
                        o.f64(x) @ w64.t(), floor, f"randn {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
def test_repeat_and_graph_replay(fmt):
    M, N, K = 33, 503, 1152
    g = rc.gen(9)
    x, r = (rc.randn(g, *s).cuda() for s in ((M, K), (M, N)))
    mw = ops.mx_quantize(rc.randn(g, N, K), fmt).cuda()

    def call():
        return ops.linear_decode_mx(x, mw, residual=r)

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
        for t in (x, r):
            t.copy_(rc.randn(g, *t.shape))
        graph.replay()
        rc.assert_bits_equal(out, call(), f"replay {i}")


@pytest.mark.parametrize("fmt", FMTS)
def test_refusals(fmt):
    g = rc.gen(1)
    x = _ints(g, 65, 192).cuda()
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.linear_decode_mx(x[:4], _int_weight(g, 16, 192, fmt).cuda())
    mw = _int_weight(g, 16, 128, fmt).cuda()
    with pytest.raises(ValueError, match="M must be in 1..64"):
        ops.linear_decode_mx(x[:, :128], mw)
    kb = mw.codes.shape[1]
    shifted = torch.zeros(16, kb + 16, dtype=torch.uint8,
                          device="cuda")[:, 4:4 + kb]
    shifted.copy_(mw.codes)
    with pytest.raises(ValueError, match="16-byte-aligned base"):
        ops.linear_decode_mx(x[:4, :128], mx.MXWeight(shifted, mw.scales,
                                                      fmt, mw.shape))


# -- engine: the two-layer models of the decode-linear tests -----------------

def _model(kind):
    torch.manual_seed(0)
    if kind == "llama":
        from tepdist_amd.models.llama import Llama, LlamaConfig
        cfg = LlamaConfig("decode-mx-test", n_layer=2, n_embd=256,
                          n_head=4, n_ctx=64, vocab_size=503, n_kv_head=2)
        return cfg, Llama(cfg, dtype=BF16).cuda().eval()
    from tepdist_amd.models import GPT2
    from tepdist_amd.models.configs import GPT2Config
    cfg = GPT2Config("decode-mx-test", n_layer=2, n_embd=128, n_head=2,
                     n_ctx=64, vocab_size=503)
    return cfg, GPT2(cfg, dtype=BF16).cuda().eval()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_step_matches_dequantized_model(kind, fmt):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    deq = copy.deepcopy(model)
    with torch.no_grad():
        for w in Generator.quantized_params(deq):
            w.copy_(mx.dequantize_ref(ops.mx_quantize(w, fmt)))
    gm = Generator(model, weight_format=fmt)
    gg = Generator(deq, decode_linear="gemm")
    S0, D = 12, cfg.n_embd // cfg.n_head
    ids = torch.randint(0, cfg.vocab_size, (1, S0 + 1), device="cuda")
    kc = [torch.zeros(1, gg.kv_heads, 32, D, dtype=BF16, device="cuda")
          for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    with torch.no_grad():
        gg._stack(gg._embed(ids[:, :S0], torch.arange(S0, device="cuda")),
                  kc, vc, 0)
        x1 = gg._embed(ids[:, S0:], torch.tensor([S0], device="cuda"))
        km, vm = [t.clone() for t in kc], [t.clone() for t in vc]
        hm, hg = gm._stack(x1, km, vm, S0), gg._stack(x1, kc, vc, S0)
        lm, lg = gm._logits(hm), gg._logits(hg)
    for got, want, what in ((hm, hg, "hidden"), (lm, lg, "logits")):
        err = (got.float() - want.float()).abs().max().item()
        bound = 3e-2 * want.float().abs().max().item()
        print(f"{kind} {fmt} {what}: max err {err:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_generate_graph_equals_eager(kind, fmt, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, weight_format=fmt)
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)


def test_engine_default_format_and_modes(monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model("gpt2")
    monkeypatch.delenv("TEPDIST_WEIGHT_FORMAT", raising=False)
    with pytest.raises(ValueError, match="weight_format"):
        Generator(model, weight_format="int4")
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    a = Generator(model).generate(ids, 10)
    b = Generator(model, weight_format="bf16").generate(ids, 10)
    assert torch.equal(a, b)
