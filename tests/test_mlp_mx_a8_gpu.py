"""ops.linear_mx_a8(act="swiglu", up=, out_format=) (csrc/mx_swiglu_a8.hip,
both tiles through hip._mx_swiglu_a8_raw) and the engine's mx_mlp knob, on the
GPU, against fp64 on mx.dequantize_ref of all three operands. Exact operands:
x codes on the activation grid under block scales 2^-1 .. 2^0 (multiples of
2^-2, |x| <= 8), weight codes worth multiples of 2^-3 up to 8 under 2^-9 ..
2^-7 (multiples of 2^-12, |w| <= 2^-4): a sum over K <= 1152 stays below 576 =
2^23.2 units of 2^-14, so every fp32 partial sum is exact, with
pre-activations within about [-12, 12]."""

import copy

import pytest
import torch

import rowwise_checks as rc
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o
from tepdist_amd.ops import mx

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PAIRS = [("mxfp4", "mxfp8"), ("mxfp8", "mxfp8"), ("mxfp4", "mxfp4")]  # w, x
TILES = [64, 128]
SHAPES = [(1, 32, 128), (133, 96, 256), (64, 160, 384), (129, 64, 512),
          (37, 503, 1152)]
pairs = pytest.mark.parametrize("pair", PAIRS, ids="x".join)
tiles = pytest.mark.parametrize("tile", TILES)


def _pack(codes, exps, fmt):
    """MXWeight of unpacked codes [N, K] and block exponents [N, K / 32]."""
    shape = tuple(codes.shape)
    if fmt == "mxfp4":
        codes = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return mx.MXWeight(codes.contiguous(), (127 + exps).to(torch.uint8), fmt,
                       shape)


def _grid(g, N, K, fmt, step, exps):
    """Codes worth multiples of `step` up to 8 under block scales 2^exps."""
    t = mx.table(fmt).double()
    pool = torch.arange(t.numel(), dtype=torch.uint8)[
        ~t.isnan() & (t / step == (t / step).round()) & (t.abs() <= 8)]
    return _pack(pool[torch.randint(0, pool.numel(), (N, K), generator=g)],
                 torch.randint(exps[0], exps[1] + 1, (N, K // 32),
                               generator=g), fmt)


def _operands(kind, M, I, K, pair, seed=0):
    """(xq, gate, up) on the CPU. Every kind ends with a token row of zeros
    (row M // 2, where M > 1) and, where I % 32 == 0 and I > 32, an all-zero
    last hidden block: the one-token, one-block shape keeps its data."""
    wfmt, xfmt = pair
    g = rc.gen(M * I + K + seed)
    if kind == "randn":
        xq = mx.mx_quantize(rc.randn(g, M, K), xfmt)
        mg, mu = (mx.mx_quantize(rc.randn(g, I, K, scale=K ** -0.5), wfmt)
                  for _ in range(2))
    else:
        xq = _grid(g, M, K, xfmt, 1.0 if xfmt == "mxfp8" else 0.5, (-1, 0))
        mg, mu = (_grid(g, I, K, wfmt, 0.125, (-9, -7)) for _ in range(2))
    if kind == "onehot":    # row j picks one x value times its own 2^e(j)
        one, j = int((mx.table(wfmt) == 1.0).nonzero()[0]), torch.arange(I)
        for w, a, b in ((mg, 37, 5), (mu, 11, 2)):
            c = torch.zeros(I, K, dtype=torch.uint8)
            c[j, (a * j + b) % K] = one
            p = _pack(c, (b * j[:, None] + torch.arange(K // 32)) % 7 - 4,
                      wfmt)
            w.codes, w.scales = p.codes, p.scales
    if M > 1:
        xq.codes[M // 2] = 0
    if I % 32 == 0 and I > 32:
        mu.codes[I - 32:] = 0
    return xq, mg, mu


def _ref(xq, mg, mu):
    x = o.f64(mx.dequantize_ref(xq))
    return tuple(x @ o.f64(mx.dequantize_ref(w)).t() for w in (mg, mu))


def _raw(xq, mg, mu, out_format=None, tile=0, out=None):
    from tepdist_amd.ops import hip
    return hip._mx_swiglu_a8_raw(xq.cuda(), mg.cuda(), mu.cuda(), out_format,
                                 tile, out)


def _floor(G, U):
    return rc.ELEM * G.abs().clamp_min(1.0) * U.abs()


@pairs
@tiles
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_sums(shape, tile, pair):
    ops_ = _operands("exact", *shape, pair)
    G, U = _ref(*ops_)
    o.assert_within_ulp(_raw(*ops_, tile=tile).cpu(), o.swiglu_fwd(G, U),
                        _floor(G, U), f"swiglu {pair} {tile} {shape}")


@pairs
@tiles
@pytest.mark.parametrize("shape", SHAPES[:4], ids=str)
def test_quantized_out_equals_quantizer(shape, tile, pair):
    for kind in ("exact", "randn", "onehot"):
        ops_ = _operands(kind, *shape, pair)
        h = _raw(*ops_, tile=tile).cpu()
        if kind == "onehot":    # a swapped gate / up pairing shows here
            G, U = _ref(*ops_)
            o.assert_within_ulp(h, o.swiglu_fwd(G, U), _floor(G, U), kind)
        for fmt in mx.FORMATS:
            got, want = _raw(*ops_, fmt, tile), mx.mx_quantize(h, fmt)
            what = f"{kind} {fmt} {pair} {tile} {shape}"
            assert got.fmt == fmt and got.shape == h.shape, what
            assert torch.equal(got.scales.cpu(), want.scales), what + " scales"
            assert torch.equal(got.codes.cpu(), want.codes), what + " codes"


@pairs
@tiles
def test_random_against_fp64(tile, pair):
    M, I, K = 2 * tile + 5, 160, 1152
    xq, mg, mu = _operands("randn", M, I, K, pair)
    G, U = _ref(xq, mg, mu)
    xa = o.f64(mx.dequantize_ref(xq)).abs()
    Eg, Eu = (K * 2.0 ** -23 * (xa @ o.f64(mx.dequantize_ref(w)).abs().t())
              for w in (mg, mu))
    floor = 1.1 * U.abs() * Eg + (G * torch.sigmoid(G)).abs() * Eu \
        + _floor(G, U)
    got, want = _raw(xq, mg, mu, tile=tile).cpu(), o.swiglu_fwd(G, U)
    err, _, tol = o.ulp_error(got, want, floor)
    print(f"randn {pair} {tile}: largest err / bound "
          f"{float((err / tol).max()):.3f}")
    o.assert_within_ulp(got, want, floor, f"randn {pair} {tile}")


@pairs
@tiles
def test_strided_views_in_filled_buffers(tile, pair):
    """Operands and outputs as views inside 0xFF (NaN) buffers: the packed
    operands' results, and nothing outside the views changes."""
    M, I, K = tile + 1, 96, 384
    xq, mg, mu = (w.cuda() for w in _operands("exact", M, I, K, pair))

    def view(rows, nbytes, off, src=None):
        buf = torch.full((rows + 2, nbytes + 2 * off), 255, dtype=torch.uint8,
                         device="cuda")
        v = buf[1:rows + 1, off:off + nbytes]
        return buf, v if src is None else v.copy_(src)

    def strided(w, rows):
        return mx.MXWeight(view(rows, w.codes.shape[1], 16, w.codes)[1],
                           view(rows, w.scales.shape[1], 4, w.scales)[1],
                           w.fmt, w.shape)

    xv, gv, uv = strided(xq, M), strided(mg, I), strided(mu, I)
    want = _raw(xq, mg, mu, tile=tile)
    ybuf, y = view(M, 2 * I, 16)
    _raw(xv, gv, uv, tile=tile, out=y.view(BF16))
    rc.assert_bits_equal(y.view(BF16), want, "bf16 view")
    y.fill_(255)
    assert bool((ybuf == 255).all()), "written outside h"
    for fmt in mx.FORMATS:
        q = _raw(xq, mg, mu, fmt, tile)
        cbuf, c = view(M, q.codes.shape[1], 8)      # rows 8-byte aligned
        sbuf, s = view(M, I // 32, 1)
        _raw(xv, gv, uv, fmt, tile, mx.MXWeight(c, s, fmt, (M, I)))
        assert torch.equal(c, q.codes) and torch.equal(s, q.scales), fmt
        c.fill_(255), s.fill_(255)
        assert bool((cbuf == 255).all()) and bool((sbuf == 255).all()), \
            f"{fmt}: written outside the codes and scales"


@pairs
def test_repeat_and_graph_replay(pair):
    xq, mg, mu = (w.cuda() for w in _operands("randn", 133, 160, 1152, pair))

    def call():
        q = ops.linear_mx_a8(xq, mg, act="swiglu", up=mu, out_format=pair[1])
        return ops.linear_mx_a8(xq, mg, act="swiglu", up=mu), q.codes, q.scales

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = call()
        assert all(torch.equal(a, b) for a, b in zip(first, call()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in range(3):
        new = _operands("randn", 133, 160, 1152, pair, seed=i + 1)[0].cuda()
        xq.codes.copy_(new.codes)
        xq.scales.copy_(new.scales)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, call())), i


def test_refusals():
    xq, mg, mu = (w.cuda() for w in _operands("exact", 70, 96, 128, PAIRS[1]))
    x4, m4, odd = (w.cuda() for w in _operands("exact", 70, 40, 128, PAIRS[2]))
    r = torch.zeros(70, 96, dtype=BF16, device="cuda")
    for kw in (dict(act="swiglu", up=mu, bias=r[0]),
               dict(act="swiglu", up=mu, residual=r), dict(act="swiglu"),
               dict(up=mu), dict(out_format="mxfp8"),
               dict(act="swiglu", up=m4),                   # format and shape
               dict(act="swiglu", up=mx.MXWeight(mu.codes[:64], mu.scales[:64],
                                                 mu.fmt, (64, 128))),
               dict(act="swiglu", up=mx.MXWeight(      # strides alone differ
                   mu.codes.repeat(1, 2)[:, :128], mu.scales, mu.fmt,
                   mu.shape))):
        with pytest.raises(ValueError):
            ops.linear_mx_a8(xq, mg, **kw)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.linear_mx_a8(x4, m4, act="swiglu", up=odd, out_format="mxfp4")
    with pytest.raises(ValueError, match="W8A4"):
        ops.linear_mx_a8(x4, mg, act="swiglu", up=mu)


@pairs
def test_engine_fused_mlp(pair, monkeypatch):
    """12-token prefill and one step, mx_mlp="fused" on the GPU against the
    same on CPU, bound max(3e-2 max|want|, twice the CPU engine against itself
    on an fp32 copy); with the knob unset the MLP is the composed sequence."""
    from tepdist_amd.inference import Generator
    from tepdist_amd.models.llama import Llama, LlamaConfig
    monkeypatch.delenv("TEPDIST_MX_MLP", raising=False)
    torch.manual_seed(0)
    cfg = LlamaConfig("mlp-mx-test", n_layer=2, n_embd=256, n_head=4,
                      n_ctx=64, vocab_size=503, n_kv_head=2)
    model = Llama(cfg, dtype=BF16).cuda().eval()
    cpu = copy.deepcopy(model).cpu()
    kw = dict(weight_format=pair[0], act_format=pair[1])
    S0, D, res = 12, cfg.n_embd // cfg.n_head, []
    ids = torch.randint(0, cfg.vocab_size, (1, S0 + 1))
    for m in (model, cpu, copy.deepcopy(cpu).float()):
        gen, w = Generator(m, mx_mlp="fused", **kw), m.wte
        kc = [torch.zeros(1, gen.kv_heads, 32, D, dtype=w.dtype,
                          device=w.device) for _ in range(cfg.n_layer)]
        vc = [torch.zeros_like(t) for t in kc]
        with torch.no_grad():
            e = gen._embed(ids.to(w.device), None)
            p = gen._stack(e[:, :S0], kc, vc, 0)
            res.append([t.float().cpu()
                        for t in (p, gen._stack(e[:, S0:], kc, vc, S0))])
    for got, want, f32, what in zip(*res, ("prefill hidden", "hidden")):
        err = (got - want).abs().max().item()
        yard = (want - f32).abs().max().item()
        bound = max(3e-2 * want.abs().max().item(), 2 * yard)
        print(f"fused mlp {pair} {what}: max err {err:.3e}, yardstick "
              f"{yard:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, err, bound)
    gen, blk = Generator(model, **kw), model.blocks[0]
    x = rc.randn(rc.gen(3), 1, S0, cfg.n_embd).cuda()
    with torch.no_grad():
        xq = ops.mx_quantize_act(ops.rmsnorm(x[0], blk.ln2_g, cfg.rms_eps),
                                 fmt=pair[1])
        h = ops.swiglu(*(ops.linear_mx_a8(xq, gen.mxw[id(w)])
                         for w in (blk.w_gate, blk.w_up)))
        want = ops.linear_mx_a8(h, gen.mxw[id(blk.w_down)], residual=x[0],
                                act_format=pair[1])
        rc.assert_bits_equal(gen._llama_mlp(x, blk)[0], want, "default mlp")
    outs = []
    for extra in ({}, dict(mx_mlp="composed")):     # the knob unset: composed
        gen = Generator(model, **kw, **extra)
        kc = [torch.zeros(1, gen.kv_heads, 32, D, dtype=BF16, device="cuda")
              for _ in range(cfg.n_layer)]
        with torch.no_grad():
            outs.append(gen._stack(gen._embed(ids[:, :S0].cuda(), None), kc,
                                   [torch.zeros_like(t) for t in kc], 0))
    assert gen.mx_mlp == "composed"
    rc.assert_bits_equal(outs[0], outs[1], "default prefill")
    for bad in (dict(mx_mlp="fused", weight_format="mxfp8"),
                dict(mx_mlp="both", **kw)):
        with pytest.raises(ValueError, match="mx_mlp"):
            Generator(model, **bad)
