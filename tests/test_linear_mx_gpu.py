"""ops.linear_mx (csrc/mx_gemm.hip, both tiles through hip._mx_gemm_raw) and
the engine's mx_linear knob, on the GPU. The reference is always fp64 on
mx.dequantize_ref(mw); operands, exactness argument (every fp32 partial sum
exact for K <= 1152) and models are those of test_linear_decode_mx_gpu.py.
Random data is held to 1 bf16 ulp + K 2^-23 (|x| . |dq(w)|^T + |bias| +
|res|): (K - 1) 2^-24 per unit of term magnitude for a sum of K terms in any
order, doubled because MFMA accumulation is not promised to round to nearest
(tests/gemm_checks.py)."""

import copy

import pytest
import torch

import rowwise_checks as rc
from test_linear_decode_mx_gpu import (_cuda, _exact, _int_weight, _ints,
                                       _model, _operands, _pack)
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import mx

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FMTS = ["mxfp8", "mxfp4"]
TILES = [64, 128]
EPI = {"none": 0, "bias": 1, "residual": 3, "bias+residual": 4}


def _cases(T):
    """Two ragged tiles each way on one K-tile; exact fit, two K-tiles; less
    than one tile; the pipeline wrapping past its three stages, twice."""
    return [(T + 1, T + 3, 128, "bias+residual"), (T, T, 256, "none"),
            (17, 40, 384, "bias"), (2 * T + 5, T - 8, 640, "residual"),
            (T - 1, 2 * T + 4, 1152, "bias+residual")]


def _raw(x, mw, b=None, r=None, act="none", tile=0, out=None):
    from tepdist_amd.ops import hip
    return hip._mx_gemm_raw(x, mw, b, r, hip.skinny_epi(b, act, r), tile, out)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", range(5))
def test_exact(case, tile, fmt):
    M, N, K, epi = _cases(tile)[case]
    x, mw, b, r = _operands(M, N, K, fmt, M * N + K)
    b = b if "bias" in epi else None
    r = r if "residual" in epi else None
    xd, bd, rd = _cuda(x, b, r)
    got = _raw(xd, mw.cuda(), bd, rd, tile=tile)
    rc.assert_bits_equal(got.cpu(), _exact(x, mw, b, r).to(BF16),
                         f"linear_mx[{fmt},{tile},{M},{N},{K},{epi}]")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
def test_strided_views_in_nan_buffers(tile, fmt):
    """x and the residual are views with ld > extent of NaN-filled buffers,
    y a view of a NaN sentinel: nothing outside [M, N] may change, nothing
    outside the operands may reach the result."""
    M, N, K = tile + 1, tile + 3, 384
    x, mw, b, r = _operands(M, N, K, fmt, 77)
    nan = float("nan")
    xb = torch.full((M + 2, K + 8), nan, dtype=BF16, device="cuda")
    rb = torch.full((M + 2, N + 5), nan, dtype=BF16, device="cuda")
    yb = torch.full((M + 2, N + 13), nan, dtype=BF16, device="cuda")
    xb[1:M + 1, :K] = x.cuda()
    rb[1:M + 1, 2:N + 2] = r.cuda()
    out = yb[1:M + 1, 5:N + 5]
    _raw(xb[1:M + 1, :K], mw.cuda(), b.cuda(), rb[1:M + 1, 2:N + 2],
         tile=tile, out=out)
    rc.assert_bits_equal(out.cpu(), _exact(x, mw, b, r).to(BF16), "inside")
    yb[1:M + 1, 5:N + 5] = nan
    assert bool(yb.isnan().all()), "written outside [M, N]"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
def test_placement(tile, fmt):
    """The one-hot-weight / distinct-x construction of
    test_linear_decode_mx_gpu.py at (T + 1, T + 3, 384): a wrong nibble
    order, lane-to-block map, scale byte, swizzle or stage slot moves a
    value. Exponents stay inside bf16's normals for up to 130 rows."""
    M, N, K = tile + 1, tile + 3, 384
    k = torch.arange(K)
    x = ((1.0 + (k % 128) / 128.0)[None, :]
         * 2.0 ** (torch.arange(M)[:, None] + 4 * (k[None, :] // 128) - 80.0))
    x = x * (1 - 2 * ((torch.arange(M)[:, None] + k[None, :]) % 2))
    n = torch.arange(N)
    sel = (n * 37 + 5) % K
    s = (5 * n[:, None] + 3 * torch.arange(K // 32)[None, :]) % 11 - 5
    one = int((mx.table(fmt) == 1.0).nonzero()[0])
    codes = torch.zeros(N, K, dtype=torch.uint8)
    codes[n, sel] = one
    got = _raw(x.to(BF16).cuda(), _pack(codes, 127 + s, fmt).cuda(),
               tile=tile)
    want = x[:, sel] * 2.0 ** s[n, sel // 32].double()[None, :]
    rc.assert_bits_equal(got.cpu(), want.to(BF16), f"placement {fmt} {tile}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
def test_random(tile, fmt):
    M, N, K = 2 * tile + 5, 503, 1152
    g = rc.gen(M + N)
    x, b, r = rc.randn(g, M, K), rc.randn(g, N), rc.randn(g, M, N)
    mw = ops.mx_quantize(rc.randn(g, N, K, scale=K ** -0.5), fmt)
    w64 = o.f64(mx.dequantize_ref(mw))
    floor = K * 2.0 ** -23 * (o.f64(x).abs() @ w64.abs().t()
                              + o.f64(b).abs() + o.f64(r).abs())
    got = _raw(*_cuda(x, mw, b, r), tile=tile)
    o.assert_within_ulp(got.cpu(), _exact(x, mw, b, r), floor,
                        f"randn {fmt} {tile}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
def test_gelu(tile, fmt):
    M, N, K = tile + 1, tile + 3, 384
    x, mw, b, _ = _operands(M, N, K, fmt, 3, exps=(-9, -7))
    a = _exact(x, mw, b)
    print(f"gelu pre-activations in [{a.min():.2f}, {a.max():.2f}]")
    got = _raw(x.cuda(), mw.cuda(), b.cuda(), act="gelu", tile=tile)
    o.assert_within_ulp(got.cpu(), o.gelu_fwd(a),
                        rc.ELEM * a.abs().clamp_min(1.0), "bias+gelu")


@pytest.mark.parametrize("fmt", FMTS)
def test_repeat_and_graph_replay(fmt):
    M, N, K = 133, 503, 1152
    g = rc.gen(9)
    x = rc.randn(g, 7, M // 7, K).cuda()      # leading dims are flattened
    r = rc.randn(g, 7, M // 7, N).cuda()
    mw = ops.mx_quantize(rc.randn(g, N, K), fmt).cuda()

    def call():
        return ops.linear_mx(x, mw, residual=r)

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


@pytest.mark.parametrize("fmt", FMTS)
def test_refusals(fmt):
    g = rc.gen(1)
    x = _ints(g, 70, 192).cuda()
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.linear_mx(x, _int_weight(g, 16, 192, fmt).cuda())
    mw = _int_weight(g, 16, 128, fmt).cuda()
    kb = mw.codes.shape[1]
    shifted = torch.zeros(16, kb + 16, dtype=torch.uint8,
                          device="cuda")[:, 4:4 + kb]
    shifted.copy_(mw.codes)
    with pytest.raises(ValueError, match="16-byte-aligned base"):
        ops.linear_mx(x[:, :128], mx.MXWeight(shifted, mw.scales, fmt,
                                              mw.shape))


# -- engine: the two-layer models of test_linear_decode_mx_gpu.py ------------

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_fused_matches_dequantized_model(kind, fmt):
    """A 12-token prefill and one further step under mx_linear="fused"
    against the decode_linear="gemm" engine on the dequantized model."""
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    deq = copy.deepcopy(model)
    with torch.no_grad():
        for w in Generator.quantized_params(deq):
            w.copy_(mx.dequantize_ref(ops.mx_quantize(w, fmt)))
    gm = Generator(model, weight_format=fmt, mx_linear="fused")
    gg = Generator(deq, decode_linear="gemm")
    S0, D = 12, cfg.n_embd // cfg.n_head
    ids = torch.randint(0, cfg.vocab_size, (1, S0 + 1), device="cuda")
    kc = [torch.zeros(1, gg.kv_heads, 32, D, dtype=BF16, device="cuda")
          for _ in range(cfg.n_layer)]
    vc = [torch.zeros_like(t) for t in kc]
    km, vm = [t.clone() for t in kc], [t.clone() for t in vc]
    with torch.no_grad():
        x0 = gg._embed(ids[:, :S0], torch.arange(S0, device="cuda"))
        x1 = gg._embed(ids[:, S0:], torch.tensor([S0], device="cuda"))
        pm, pg = gm._stack(x0, km, vm, 0), gg._stack(x0, kc, vc, 0)
        hm, hg = gm._stack(x1, km, vm, S0), gg._stack(x1, kc, vc, S0)
        lm, lg = gm._logits(hm), gg._logits(hg)
    for got, want, what in ((pm, pg, "prefill hidden"), (hm, hg, "hidden"),
                            (lm, lg, "logits")):
        err = (got.float() - want.float()).abs().max().item()
        bound = 3e-2 * want.float().abs().max().item()
        print(f"{kind} {fmt} {what}: max err {err:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_fused_generate_graph_equals_eager(kind, fmt, monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model(kind)
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    gen = Generator(model, weight_format=fmt, mx_linear="fused")
    monkeypatch.delenv("TEPDIST_DECODE_GRAPH", raising=False)
    a = gen.generate(ids, 10)
    monkeypatch.setenv("TEPDIST_DECODE_GRAPH", "0")
    b = gen.generate(ids, 10)
    assert a.shape == (2, 22)
    assert torch.equal(a, b), (a, b)


def test_engine_default_is_dequant(monkeypatch):
    from tepdist_amd.inference import Generator
    cfg, model = _model("gpt2")
    monkeypatch.delenv("TEPDIST_MX_LINEAR", raising=False)
    with pytest.raises(ValueError, match="mx_linear"):
        Generator(model, weight_format="mxfp8", mx_linear="tiled")
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    a = Generator(model, weight_format="mxfp8").generate(ids, 10)
    b = Generator(model, weight_format="mxfp8",
                  mx_linear="dequant").generate(ids, 10)
    assert torch.equal(a, b)
