"""MXFP4 activations on the GPU: ops.mx_quantize_act(fmt="mxfp4") (csrc/
mx_act_quant.hip), ops.linear_mx_a8 on the e2m1 x e2m1 instantiations of
csrc/mx_gemm_a8.hip (both tiles through hip._mx_gemm_a8_raw) and the engine's
act_format="mxfp4". The quantizer is held to mx.mx_quantize(x, "mxfp4") in
every byte; the GEMM's reference is fp64 on mx.dequantize_ref of both
operands. Exact cases draw x as e2m1 values times 2^(-1 .. 1) per block,
which survives the MXFP4 round trip bit for bit (every block amax puts all
its elements on codes); against the mxfp4 weights of the decode tests
(multiples of 2^-3 up to 12) every partial sum is a multiple of 2^-5 below
2^18: exact in fp32, so the result is fp64 rounded once. Random data is held
to 1 bf16 ulp + K 2^-23 (|dq(Xq)| . |dq(W)|^T + |bias| + |res|), the
fp32-accumulation bound of test_linear_mx_gpu.py.

Measured on the MI355X, largest err / bound of test_random: see
docs/KERNELS.md "MX weights x MXFP4 activations"."""

import copy

import pytest
import torch

import rowwise_checks as rc
from test_linear_decode_mx_gpu import (_cuda, _exact, _int_weight, _model,
                                       _pack)
from test_linear_mx_gpu import _cases
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import mx

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TILES = [64, 128]
NAN = float("nan")
F4 = "mxfp4"


def _raw(x, mw, b=None, r=None, act="none", tile=0, out=None):
    from tepdist_amd.ops import hip
    xq = x if isinstance(x, mx.MXWeight) else ops.mx_quantize_act(x, fmt=F4)
    return hip._mx_gemm_a8_raw(xq, mw, b, r, hip.skinny_epi(b, act, r), tile,
                               out)


def _operands(M, N, K, seed, wexps=(-2, 1)):
    """x on the e2m1 grid (see above), an mxfp4 weight, bias and residual in
    eighths."""
    g = rc.gen(seed)
    x = mx.dequantize_ref(_pack(
        torch.randint(0, 16, (M, K), generator=g).to(torch.uint8),
        127 + torch.randint(-1, 2, (M, K // 32), generator=g), F4))
    eighths = [(torch.randint(-40, 41, s, generator=g) / 8).to(BF16)
               for s in ((N,), (M, N))]
    return x, _int_weight(g, N, K, F4, wexps), *eighths


def _same_bytes(got, want, what):
    assert torch.equal(got.codes.cpu(), want.codes), what + " codes"
    assert torch.equal(got.scales.cpu(), want.scales), what + " scales"


# -- the quantizer -----------------------------------------------------------

def test_quantize_every_finite_bf16():
    pat = torch.arange(1 << 16, dtype=torch.int32)
    pat = pat[(pat & 0x7f80) != 0x7f80].reshape(510, 128)
    x = pat.to(torch.int16).view(BF16)
    want = mx.mx_quantize(x, F4)
    _same_bytes(ops.mx_quantize_act(x.cuda(), fmt=F4), want, "every pattern")
    rc.assert_bits_equal(
        ops.mx_quantize_act(x.cuda(), roundtrip=True, fmt=F4),
        mx.dequantize_ref(want), "round trip")


def test_quantize_strided_views_and_out_buffers():
    """x a view of a NaN buffer; codes, scales (an unaligned view: the byte
    path, the test above takes the dword path) and the round trip written
    into views of sentinel buffers, which stay unchanged around them."""
    M, K = 67, 384
    g = rc.gen(5)
    x = rc.randn(g, M, K) * 2.0 ** torch.randint(-20, 21, (M, K), generator=g)
    want = mx.mx_quantize(x, F4)
    xb = torch.full((M + 2, K + 8), NAN, dtype=BF16, device="cuda")
    xb[1:M + 1, :K] = x.cuda()
    cb = torch.full((M + 2, K // 2 + 16), 0xA5, dtype=torch.uint8,
                    device="cuda")
    sb = torch.full((M + 2, K // 32 + 4), 0xA5, dtype=torch.uint8,
                    device="cuda")
    rb = torch.full((M + 2, K + 8), NAN, dtype=BF16, device="cuda")
    inner = (slice(1, M + 1), slice(8, K // 2 + 8))
    out = mx.MXWeight(cb[inner], sb[1:M + 1, 1:K // 32 + 1], F4, (M, K))
    xv = xb[1:M + 1, :K]
    assert ops.mx_quantize_act(xv, out=out, fmt=F4) is out
    _same_bytes(out, want, "strided")
    ops.mx_quantize_act(xv, roundtrip=True, out=rb[1:M + 1, :K], fmt=F4)
    rc.assert_bits_equal(rb[1:M + 1, :K], mx.dequantize_ref(want), "rt out=")
    cb[inner] = 0xA5
    sb[1:M + 1, 1:K // 32 + 1] = 0xA5
    rb[1:M + 1, :K] = NAN
    assert bool((cb == 0xA5).all()) and bool((sb == 0xA5).all()) and \
        bool(rb.isnan().all()), "written outside [M, K]"


# -- the GEMM ------------------------------------------------------------------

@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", range(5))
def test_exact(case, tile):
    M, N, K, epi = _cases(tile)[case]
    x, mw, b, r = _operands(M, N, K, M * N + K)
    assert torch.equal(mx.dequantize_ref(mx.mx_quantize(x, F4)), x)
    b = b if "bias" in epi else None
    r = r if "residual" in epi else None
    xd, bd, rd = _cuda(x, b, r)
    got = _raw(xd, mw.cuda(), bd, rd, tile=tile)
    rc.assert_bits_equal(got.cpu(), _exact(x, mw, b, r).to(BF16),
                         f"linear_mx_a4[{tile},{M},{N},{K},{epi}]")


@pytest.mark.parametrize("tile", TILES)
def test_placement(tile):
    """Pre-packed x whose codes cycle through all 16 e2m1 codes under a scale
    byte that changes with row and block, against one-hot weight rows (the
    code of 1.0 at (37 n + 5) % K) under their own varying scales: each
    output is one x value times both scales, exact in bf16. A wrong B lane
    map, nibble order, scale lane, swizzle or stage slot moves a value."""
    M, N, K = tile + 1, tile + 3, 384
    m, k, n = torch.arange(M), torch.arange(K), torch.arange(N)
    xcodes = ((m[:, None] * K + k[None, :]) % 16).to(torch.uint8)
    xs = (7 * m[:, None] + 5 * torch.arange(K // 32)[None, :]) % 41 - 20
    xq = _pack(xcodes, 127 + xs, F4)
    sel = (n * 37 + 5) % K
    s = (5 * n[:, None] + 3 * torch.arange(K // 32)[None, :]) % 11 - 5
    codes = torch.zeros(N, K, dtype=torch.uint8)
    codes[n, sel] = 2                                   # e2m1 1.0
    got = _raw(xq.cuda(), _pack(codes, 127 + s, F4).cuda(), tile=tile)
    xv = o.f64(mx.dequantize_ref(xq))
    want = xv[:, sel] * 2.0 ** s[n, sel // 32].double()[None, :] + 0.0
    rc.assert_bits_equal(got.cpu(), want.to(BF16), f"placement {tile}")


@pytest.mark.parametrize("tile", TILES)
def test_random(tile):
    M, N, K = 2 * tile + 5, 503, 1152
    g = rc.gen(M + N)
    x, b, r = rc.randn(g, M, K), rc.randn(g, N), rc.randn(g, M, N)
    mw = ops.mx_quantize(rc.randn(g, N, K, scale=K ** -0.5), F4)
    xq = mx.dequantize_ref(mx.mx_quantize(x, F4))
    floor = K * 2.0 ** -23 * (
        o.f64(xq).abs() @ o.f64(mx.dequantize_ref(mw)).abs().t()
        + o.f64(b).abs() + o.f64(r).abs())
    got = _raw(*_cuda(x, mw, b, r), tile=tile).cpu()
    want = _exact(xq, mw, b, r)
    err, unit, tol = o.ulp_error(got, want, floor)
    print(f"randn a4 {tile}: largest err / bound "
          f"{float((err / tol).max()):.3f}")
    o.assert_within_ulp(got, want, floor, f"randn a4 {tile}")


@pytest.mark.parametrize("tile", TILES)
def test_gelu_and_strided_views_in_nan_buffers(tile):
    """bias + gelu at the elementwise bound; then the residual and y as views
    of NaN buffers, x as a view of a NaN buffer: nothing outside [M, N] may
    change, nothing outside the operands may reach the result."""
    M, N, K = tile + 1, tile + 3, 384
    x, mw, b, _ = _operands(M, N, K, 3, wexps=(-9, -7))
    a = _exact(x, mw, b)
    got = _raw(x.cuda(), mw.cuda(), b.cuda(), act="gelu", tile=tile)
    o.assert_within_ulp(got.cpu(), o.gelu_fwd(a),
                        rc.ELEM * a.abs().clamp_min(1.0), "bias+gelu")
    x, mw, b, r = _operands(M, N, K, 77)
    xb = torch.full((M + 2, K + 8), NAN, dtype=BF16, device="cuda")
    rb = torch.full((M + 2, N + 5), NAN, dtype=BF16, device="cuda")
    yb = torch.full((M + 2, N + 13), NAN, dtype=BF16, device="cuda")
    xb[1:M + 1, :K] = x.cuda()
    rb[1:M + 1, 2:N + 2] = r.cuda()
    out = yb[1:M + 1, 5:N + 5]
    _raw(xb[1:M + 1, :K], mw.cuda(), b.cuda(), rb[1:M + 1, 2:N + 2],
         tile=tile, out=out)
    rc.assert_bits_equal(out.cpu(), _exact(x, mw, b, r).to(BF16), "inside")
    yb[1:M + 1, 5:N + 5] = NAN
    assert bool(yb.isnan().all()), "written outside [M, N]"


def test_repeat_and_graph_replay():
    M, N, K = 133, 503, 1152
    g = rc.gen(9)
    x = rc.randn(g, 7, M // 7, K).cuda()      # leading dims are flattened
    r = rc.randn(g, 7, M // 7, N).cuda()
    mw = ops.mx_quantize(rc.randn(g, N, K), F4).cuda()

    def call():
        return ops.linear_mx_a8(x, mw, residual=r, act_format=F4)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = call()
        assert first.shape == r.shape
        rc.assert_bits_equal(first, call(), "two eager calls")
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


def test_refusals():
    g = rc.gen(1)
    x = rc.randn(g, 70, 192).cuda()
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.linear_mx_a8(x, _int_weight(g, 16, 192, F4).cuda(),
                         act_format=F4)
    xq = ops.mx_quantize_act(x[:, :128], fmt=F4)
    for arg in (x[:, :128], xq):
        with pytest.raises(ValueError, match="W8A4"):
            ops.linear_mx_a8(arg, _int_weight(g, 16, 128, "mxfp8").cuda(),
                             act_format=F4)
    shifted = torch.zeros(70, 80, dtype=torch.uint8, device="cuda")[:, 4:68]
    shifted.copy_(xq.codes)
    with pytest.raises(ValueError, match="16-byte-aligned base"):
        ops.linear_mx_a8(mx.MXWeight(shifted, xq.scales, F4, xq.shape),
                         _int_weight(g, 16, 128, F4).cuda())


# -- engine: the two-layer models of test_linear_decode_mx_gpu.py ------------

@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_matches_cpu_engine(kind):
    """A 12-token prefill and one further step under weight_format = act_format
    = "mxfp4" against the same Generator on a CPU copy of the model (reference
    ops). The bound is the rule of the a8 engine test: an activation that
    another rounding order moves across a code boundary changes by a whole
    e2m1 step, so the yardstick is the CPU engine against itself on an fp32
    copy of the model; max(3e-2 max|want|, twice that) is allowed, and both
    figures are printed (docs/KERNELS.md has them)."""
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    cpu = copy.deepcopy(model).cpu()
    gens = [Generator(m, weight_format=F4, act_format=F4)
            for m in (model, cpu, copy.deepcopy(cpu).float())]
    S0, D = 12, cfg.n_embd // cfg.n_head
    ids = torch.randint(0, cfg.vocab_size, (1, S0 + 1))
    res = []
    for gen in gens:
        w = gen.m.wte
        kc = [torch.zeros(1, gen.kv_heads, 32, D, dtype=w.dtype,
                          device=w.device) for _ in range(cfg.n_layer)]
        vc = [torch.zeros_like(t) for t in kc]
        i = ids.to(w.device)
        with torch.no_grad():
            x0 = gen._embed(i[:, :S0], torch.arange(S0, device=w.device))
            x1 = gen._embed(i[:, S0:], torch.tensor([S0], device=w.device))
            p = gen._stack(x0, kc, vc, 0)
            h = gen._stack(x1, kc, vc, S0)
            res.append([t.float().cpu() for t in (p, h, gen._logits(h))])
    fails = []
    for got, want, f32, what in zip(*res, ("prefill hidden", "hidden",
                                           "logits")):
        err = (got - want).abs().max().item()
        yard = (want - f32).abs().max().item()
        bound = max(3e-2 * want.abs().max().item(), 2 * yard)
        print(f"{kind} a4 {what}: max err {err:.3e}, yardstick {yard:.3e}, "
              f"bound {bound:.3e}")
        if got.shape != want.shape or not err <= bound:
            fails.append((what, err, bound))
    assert not fails, fails


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_generate_graph_equals_eager(kind, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, weight_format=F4, act_format=F4)
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)


def test_engine_needs_mxfp4_weights():
    from tepdist_amd.inference import Generator
    _, model = _model("gpt2")
    with pytest.raises(ValueError, match="act_format"):
        Generator(model, act_format=F4, weight_format="bf16")
