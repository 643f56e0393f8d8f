"""Fused MoE routing kernels (ops/csrc/moe_route.hip) against the reference
ops run on CPU copies of the same inputs.

Integer outputs and the dispatch copy must match exactly. Sums (dispatch
backward, combine forward, dy) are exact fp32 sums of at most four terms
rounded to bf16 once, i.e. at most 2^-9 relative; the criterion is
|got - ref| <= 2^-8 * max(1, max|ref|), a factor of two over that. dw is an
fp32 dot product: |dw - ref| <= d * 2^-23 * sum_i |y_i * dout_i| (the fp32
summation bound for any order), against a float64 reference."""

import functools

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.models.moe import MoELayer
from tepdist_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")


def _gates(pattern, T, E, dtype, gen):
    """Rows of distinct values j/128 (exact in bf16 for j <= 64), so that no
    comparison depends on a tie unless the pattern asks for one."""
    vals = (torch.arange(E) + 1).float() / 128
    if pattern == "random":
        g = torch.stack([vals[torch.randperm(E, generator=gen)]
                         for _ in range(T)])
    elif pattern == "identical":        # one expert set takes every token
        g = vals[torch.randperm(E, generator=gen)].expand(T, E).contiguous()
    elif pattern == "equal":            # the tie rule
        g = torch.full((T, E), 0.25)
    else:
        raise AssertionError(pattern)
    return g.to(dtype)


def _assert_route_equal(got, want, msg):
    for name, a, b in zip(("topi", "slot", "src", "counts"), got, want):
        assert a.dtype == torch.int32 and a.shape == b.shape, (msg, name)
        assert torch.equal(a.cpu(), b), f"{msg}: {name} differs"


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E", [3, 8, 64])
@pytest.mark.parametrize("T", [1, 63, 65, 257, 700])
def test_route_exact(T, E, dtype):
    gen = torch.Generator().manual_seed(1000 * T + E)
    for pattern in ("random", "identical", "equal"):
        g = _gates(pattern, T, E, dtype, gen)
        g_dev = g.cuda()
        for k in (1, 2, 4):
            if k > E:
                continue
            for C in sorted({1, 5, T}):
                got = ops.moe_route(g_dev, k, C)
                want = ref.moe_route(g, k, C)
                _assert_route_equal(got, want,
                                    f"{pattern} T={T} E={E} k={k} C={C}")
    # the tie rule itself, independent of the reference
    topi = ops.moe_route(_gates("equal", T, E, dtype, gen).cuda(),
                         min(4, E), 5).topi.cpu()
    assert torch.equal(topi, torch.arange(min(4, E), dtype=torch.int32)
                       .expand(T, min(4, E)))


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E,k", [(8, 2), (5, 4), (64, 3)])
def test_route_nan_gates_stay_in_range(E, k, dtype):
    T, C = 300, 7
    gen = torch.Generator().manual_seed(E)
    g = torch.rand(T, E, generator=gen)
    g[torch.rand(T, E, generator=gen) < 0.3] = NAN
    g[::17] = NAN                                   # whole rows of NaN
    topi, slot, src, counts = (t.cpu().long() for t in
                               ops.moe_route(g.to(dtype).cuda(), k, C))
    assert ((topi >= 0) & (topi < E)).all()
    srt = topi.sort(-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "experts of a row not distinct"
    assert ((slot >= -1) & (slot < E * C)).all()
    flat = slot.reshape(-1)
    kept = flat >= 0
    assert torch.equal(src[flat[kept]], torch.arange(T * k)[kept])
    assert (src >= 0).sum() == kept.sum() and (src[src < 0] == -1).all()
    assert (flat[kept] // C == topi.reshape(-1)[kept]).all()
    assert torch.equal(counts, torch.bincount(topi.reshape(-1), minlength=E))


# -- rows -------------------------------------------------------------------

T_ROW, E_ROW, K_ROW, C_ROW = 65, 8, 2, 20


@functools.lru_cache(maxsize=None)
def _row_case(d):
    """One routing with filled, dropped and empty slots, computed once per
    d and shared (read-only) by the row tests: expert 0 is the first choice
    of 40 tokens (capacity 20 -> drops), expert 7 is nobody's (-> empty)."""
    gen = torch.Generator().manual_seed(d)
    g = _gates("random", T_ROW, E_ROW, BF16, gen).float()
    g[:, 7] = 0.0
    g[:40, 0] = 1.0
    g = g.to(BF16)
    route = ref.moe_route(g, K_ROW, C_ROW)
    topi, slot, src, counts = route
    assert (slot < 0).any() and (src < 0).any() and (src >= 0).any()
    x = torch.randn(T_ROW, d, generator=gen).to(BF16)
    y = torch.randn(E_ROW * C_ROW, d, generator=gen).to(BF16)
    y[src < 0] = NAN                    # never-filled slots must not matter
    w = torch.rand(T_ROW, K_ROW, generator=gen) + 0.1
    dout = torch.randn(T_ROW, d, generator=gen).to(BF16)
    dD = torch.randn(E_ROW * C_ROW, d, generator=gen).to(BF16)
    cpu = dict(g=g, route=route, x=x, y=y, w=w, dout=dout, dD=dD)
    dev = {n: t.cuda() for n, t in cpu.items() if n != "route"}
    dev["route"] = ops.moe_route(dev["g"], K_ROW, C_ROW)
    torch.cuda.synchronize()
    return cpu, dev


def _close(got, want):
    got = got.float().cpu()
    assert got.shape == want.shape
    assert torch.isfinite(got).all(), "a never-filled (NaN) slot was used"
    err = (got - want).abs().max().item()
    bound = 2.0 ** -8 * max(1.0, want.abs().max().item())
    assert err <= bound, f"max err {err} > {bound}"


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("d", [8, 64, 200])
def test_dispatch_forward_bit_equal(d):
    cpu, dev = _row_case(d)
    _assert_route_equal(dev["route"], cpu["route"], "row case")
    got = ops.moe_dispatch(dev["x"], dev["route"])
    want = ref.moe_dispatch_fwd(cpu["x"], cpu["route"][2], K_ROW)
    assert got.dtype == BF16 and got.shape == (E_ROW * C_ROW, d)
    assert torch.equal(_bits(got).cpu(), _bits(want))
    assert (got[dev["route"].src < 0] == 0).all()


@pytest.mark.parametrize("d", [8, 64, 200])
def test_dispatch_backward(d):
    cpu, dev = _row_case(d)
    x = dev["x"].clone().requires_grad_()
    ops.moe_dispatch(x, dev["route"]).backward(dev["dD"])
    want = ref.moe_dispatch_bwd(cpu["dD"].float(), cpu["route"][1])
    assert x.grad.dtype == BF16
    _close(x.grad, want)


@pytest.mark.parametrize("d", [8, 64, 200])
def test_combine_forward(d):
    cpu, dev = _row_case(d)
    got = ops.moe_combine(dev["y"], dev["w"], dev["route"])
    want = ref.moe_combine_fwd(cpu["y"].float(), cpu["w"], cpu["route"][1])
    assert got.dtype == BF16
    _close(got, want)


@pytest.mark.parametrize("d", [8, 64, 200])
def test_combine_backward(d):
    cpu, dev = _row_case(d)
    _, slot, src, _ = cpu["route"]
    y = dev["y"].clone().requires_grad_()
    w = dev["w"].clone().requires_grad_()
    ops.moe_combine(y, w, dev["route"]).backward(dev["dout"])
    dy_ref, _ = ref.moe_combine_bwd(cpu["dout"].float(), cpu["y"].float(),
                                    cpu["w"], slot, src)
    assert y.grad.dtype == BF16 and w.grad.dtype == torch.float32
    _close(y.grad, dy_ref)
    assert (y.grad.cpu()[src < 0] == 0).all()

    y64, do64 = cpu["y"].double(), cpu["dout"].double()
    rows = y64[slot.long().clamp_min(0)]                     # [T, k, d]
    prod = rows * do64.unsqueeze(1)
    dw_ref, mag = prod.sum(-1), prod.abs().sum(-1)
    dw = w.grad.cpu()
    kept = slot >= 0
    assert (dw[~kept] == 0).all(), "dw of a dropped entry is not exactly 0"
    assert torch.isfinite(dw).all()
    err = (dw.double() - dw_ref).abs()[kept]
    bound = (d * 2.0 ** -23 * mag)[kept]
    assert (err <= bound).all(), (err.max().item(), bound.min().item())


def test_bit_reproducible():
    cpu, dev = _row_case(200)

    def run():
        route = ops.moe_route(dev["g"], K_ROW, C_ROW)
        x = dev["x"].clone().requires_grad_()
        y = dev["y"].clone().requires_grad_()
        w = dev["w"].clone().requires_grad_()
        D = ops.moe_dispatch(x, route)
        out = ops.moe_combine(y, w, route)
        D.backward(dev["dD"])
        out.backward(dev["dout"])
        return list(route) + [_bits(D), _bits(out), _bits(x.grad),
                              _bits(y.grad), w.grad.view(torch.int32)]

    big = _gates("random", 700, 64, BF16, torch.Generator().manual_seed(9))
    big = big.cuda()
    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, v in zip(ops.moe_route(big, 4, 5), ops.moe_route(big, 4, 5)):
        assert torch.equal(u, v)


def test_bad_arguments_raise():
    cpu, dev = _row_case(8)
    route = dev["route"]
    T, k, EC = T_ROW, K_ROW, E_ROW * C_ROW
    bad = [
        lambda: ops.moe_dispatch(torch.zeros(T, 12, dtype=BF16,
                                             device="cuda"), route),
        lambda: ops.moe_dispatch(torch.zeros(T, 8, dtype=torch.float16,
                                             device="cuda"), route),
        lambda: ops.moe_combine(torch.zeros(EC, 12, dtype=BF16,
                                            device="cuda"), dev["w"], route),
        lambda: ops.moe_combine(torch.zeros(EC, 8, dtype=torch.float16,
                                            device="cuda"), dev["w"], route),
        lambda: ops.moe_route(torch.rand(16, 65, device="cuda"), 2, 4),
        lambda: ops.moe_route(torch.rand(16, 8, device="cuda"), 5, 4),
        lambda: ops.moe_route(torch.rand(16, 3, device="cuda"), 4, 4),
        lambda: ops.moe_route(torch.rand(16, 8, device="cuda"), 2, 0),
        lambda: ops.moe_route(torch.rand(8, 16, device="cuda").t(), 2, 4),
        lambda: ops.moe_route(torch.rand(16, 16, device="cuda")[:, ::2],
                              2, 4),
        # maps that do not fit the rows they are used with
        lambda: ops.moe_dispatch(torch.zeros(T, 8, dtype=BF16,
                                             device="cuda"),
                                 route._replace(src=route.src.long())),
        lambda: ops.moe_combine(torch.zeros(EC, 8, dtype=BF16,
                                            device="cuda"),
                                dev["w"][:-1], route),
    ]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
    torch.cuda.synchronize()


# -- layer ------------------------------------------------------------------

def _tie_free_layer_inputs(d, E, B, S, gen):
    """w_gate and x built so that the logits of a token are a permutation of
    {1, ..., E} EXACTLY (sums of a few multiples of 1/32, exact in bf16 and
    in the fp32 accumulator): the gates of a row differ by factors of e."""
    blk = d // E
    w_gate = torch.zeros(E, d)
    for e in range(E):
        w_gate[e, e * blk:(e + 1) * blk] = 2.0
    x = torch.empty(B * S, d)
    for t in range(B * S):
        perm = torch.randperm(E, generator=gen) + 1
        x[t] = (perm.float() * 0.5 / blk).repeat_interleave(blk)
    return w_gate, x.reshape(B, S, d)


def _make_layers(d, E, k, gen):
    layers = {m: MoELayer(d, E, k, route=m).cuda()
              for m in ("composed", "fused")}
    base = layers["composed"]
    with torch.no_grad():
        for p in base.parameters():
            p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(BF16))
    return layers


def test_layer_fused_matches_composed():
    d, E, k, B, S = 64, 4, 2, 2, 33
    gen = torch.Generator().manual_seed(0)
    layers = _make_layers(d, E, k, gen)
    w_gate, x = _tie_free_layer_inputs(d, E, B, S, gen)
    with torch.no_grad():
        layers["composed"].w_gate.copy_(w_gate.to(BF16))
        for p, q in zip(layers["fused"].parameters(),
                        layers["composed"].parameters()):
            p.copy_(q)
    x = x.to(BF16).cuda()
    with torch.no_grad():
        want = layers["composed"](x).float().cpu()
        got = layers["fused"](x).float().cpu()
        aux = [layers[m].aux_loss.item() for m in ("composed", "fused")]
    assert want.abs().max() > 0 and torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    bound = 2.0 ** -6 * max(1.0, want.abs().max().item())
    assert err <= bound, f"max err {err} > {bound}"
    assert abs(aux[0] - aux[1]) <= 1e-5 * max(1.0, abs(aux[0]))


def test_layer_capture_replay_bit_equal():
    d, E, k, B, S = 64, 4, 2, 2, 33
    gen = torch.Generator().manual_seed(1)
    layers = _make_layers(d, E, k, gen)
    layer = layers["fused"]
    with torch.no_grad():
        for p, q in zip(layer.parameters(), layers["composed"].parameters()):
            p.copy_(q)
    xs = [torch.randn(B, S, d, generator=gen).to(BF16).cuda()
          for _ in range(2)]
    static_x = xs[0].clone().requires_grad_()

    def step(inp):
        for p in layer.parameters():
            p.grad = None
        inp.grad = None
        out = layer(inp)
        (out.float().square().sum() + layer.aux_loss).backward()
        layer.aux_loss = layer.aux_loss.detach()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(static_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    # capture on the warm-up stream: the parameters' AccumulateGrad nodes
    # were created there, and the whole step stays on one stream
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = step(static_x)
    static_dx = static_x.grad
    static_dw = layer.w1.grad

    with torch.no_grad():
        static_x.copy_(xs[1])
    graph.replay()
    torch.cuda.synchronize()
    got = [static_out.detach().clone(), static_dx.clone(), static_dw.clone()]

    eager_x = xs[1].clone().requires_grad_()
    out = step(eager_x)
    torch.cuda.synchronize()
    want = [out.detach(), eager_x.grad, layer.w1.grad]
    for a, b in zip(got, want):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(_bits(a), _bits(b))
