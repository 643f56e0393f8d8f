"""MoE routing ops (ops.moe_route / moe_dispatch / moe_combine) on CPU: the
pure-torch reference ops against the composed static_dispatch /
static_combine on tie-free fp32 inputs (random fp32 gates do not tie), the
tie rule, and MoELayer(route="fused") against route="composed"."""

import pytest
import torch

from tepdist_amd import ops
from tepdist_amd.models.moe import MoELayer, static_combine, static_dispatch

CASES = [(16, 4, 2, 3), (37, 8, 2, 100), (9, 3, 1, 2)]
D_MODEL = 12


def _inputs(T, E, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(T, D_MODEL, generator=gen)
    gates = torch.softmax(torch.randn(T, E, generator=gen), -1)
    assert all(r.unique().numel() == E for r in gates)      # tie-free
    return x, gates


def _weights(gates, topi):
    w = gates.float().gather(1, topi.long())
    return w / w.sum(-1, keepdim=True).clamp_min(1e-9)


@pytest.mark.parametrize("T,E,k,C", CASES)
def test_reference_ops_match_composed(T, E, k, C):
    x, gates = _inputs(T, E, seed=T)
    D_ref, (flat_t, slot_safe, keep, flat_w) = static_dispatch(
        x, gates, k, C, route="composed")
    route = ops.moe_route(gates, k, C)
    for t in route:
        assert t.dtype == torch.int32
    assert route.topi.shape == (T, k) and route.slot.shape == (T, k)
    assert route.src.shape == (E * C,) and route.counts.shape == (E,)

    D = ops.moe_dispatch(x, route)
    assert D.shape == (E * C, D_MODEL)
    assert torch.equal(D.reshape(E, C, D_MODEL), D_ref)

    slot = route.slot.reshape(-1).long()
    assert torch.equal(slot >= 0, keep)
    assert torch.equal(slot[keep], slot_safe[keep])
    assert torch.equal(_weights(gates, route.topi).reshape(-1), flat_w)
    assert torch.equal(route.counts.long(),
                       torch.bincount(route.topi.reshape(-1).long(),
                                      minlength=E))
    # src is the inverse of slot on the filled slots, -1 elsewhere
    src = route.src.long()
    assert torch.equal(src[slot[keep]], torch.arange(T * k)[keep])
    assert (src >= 0).sum() == keep.sum()
    assert (src[src < 0] == -1).all()


@pytest.mark.parametrize("T,E,k,C", CASES)
def test_gradients_match_composed(T, E, k, C):
    """dispatch -> scale -> combine, gradients to x and to gates."""
    x0, g0 = _inputs(T, E, seed=100 + T)
    gen = torch.Generator().manual_seed(7)
    scale = torch.randn(E, C, D_MODEL, generator=gen)
    dout = torch.randn(T, D_MODEL, generator=gen)

    def run(fused):
        x = x0.clone().requires_grad_()
        logits = g0.log().clone().requires_grad_()
        gates = torch.softmax(logits, -1)
        if fused:
            route = ops.moe_route(gates, k, C)
            D = ops.moe_dispatch(x, route).reshape(E, C, D_MODEL)
            out = ops.moe_combine((D * scale).reshape(E * C, D_MODEL),
                                  _weights(gates, route.topi), route)
        else:
            D, _ = static_dispatch(x, gates, k, C, route="composed")
            out = static_combine(D * scale, x, gates, k, route="composed")
        (out * dout).sum().backward()
        return out.detach(), x.grad, logits.grad

    got, want = run(True), run(False)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 1e-6


def test_static_functions_follow_route():
    """static_dispatch/static_combine with route="fused" run the ops and
    keep their return shapes; "auto" on CPU stays composed."""
    T, E, k, C = CASES[0]
    x, gates = _inputs(T, E, seed=3)
    D_c, aux_c = static_dispatch(x, gates, k, C, route="composed")
    D_f, aux_f = static_dispatch(x, gates, k, C, route="fused")
    D_a, _ = static_dispatch(x, gates, k, C)
    assert torch.equal(D_f, D_c) and torch.equal(D_a, D_c)
    keep = aux_c[2]
    assert torch.equal(aux_f[0], aux_c[0]) and torch.equal(aux_f[2], keep)
    assert torch.equal(aux_f[1][keep], aux_c[1][keep])
    assert torch.equal(aux_f[3], aux_c[3])
    y = torch.randn(E, C, D_MODEL, generator=torch.Generator().manual_seed(4))
    want = static_combine(y, x, gates, k, route="composed")
    got = static_combine(y, x, gates, k, route="fused")
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-6


def test_tie_rule_lower_expert_first():
    for dtype in (torch.float32, torch.bfloat16):
        gates = torch.full((5, 6), 0.25, dtype=dtype)
        route = ops.moe_route(gates, 3, 4)
        assert torch.equal(route.topi,
                           torch.arange(3, dtype=torch.int32).expand(5, 3))
        # experts 0..2 receive all five tokens in token order, capacity 4
        want = torch.tensor([[e * 4 + t if t < 4 else -1 for e in range(3)]
                             for t in range(5)], dtype=torch.int32)
        assert torch.equal(route.slot, want)
        assert route.counts.tolist() == [5, 5, 5, 0, 0, 0]
    # partial tie: the larger gate first, then the tied ones by index
    gates = torch.tensor([[0.1, 0.3, 0.3, 0.2, 0.3]])
    assert ops.moe_route(gates, 4, 1).topi.tolist() == [[1, 2, 4, 3]]


def test_combine_ignores_never_filled_slots():
    T, E, k, C = 9, 3, 1, 2
    x, gates = _inputs(T, E, seed=5)
    route = ops.moe_route(gates, k, C + 20)          # plenty of empty slots
    y = torch.randn(E * (C + 20), D_MODEL)
    y[route.src < 0] = float("nan")
    out = ops.moe_combine(y, _weights(gates, route.topi), route)
    assert torch.isfinite(out).all()


def test_moe_layer_fused_matches_composed_cpu():
    torch.manual_seed(0)
    layers = {}
    for mode in ("composed", "fused"):
        layer = MoELayer(32, num_experts=4, top_k=2, dtype=torch.float32,
                         route=mode)
        layers[mode] = layer
    src = layers["composed"]
    with torch.no_grad():
        for p in src.parameters():
            p.normal_(0, 0.3)
        for p, q in zip(layers["fused"].parameters(), src.parameters()):
            p.copy_(q)
    x0 = torch.randn(2, 19, 32)
    res = {}
    for mode, layer in layers.items():
        x = x0.clone().requires_grad_()
        out = layer(x)
        (out.square().sum() + layer.aux_loss).backward()
        res[mode] = [out.detach(), layer.aux_loss.detach(), x.grad] + \
            [p.grad for p in layer.parameters()]
    assert res["fused"][0].abs().max() > 0
    for a, b in zip(res["fused"], res["composed"]):
        assert a is not None and b is not None
        assert (a - b).abs().max().item() <= 1e-5


def test_moe_layer_route_selector(monkeypatch):
    with pytest.raises(ValueError):
        MoELayer(32, 4, 2, dtype=torch.float32, route="fast")
    monkeypatch.setenv("TEPDIST_MOE_ROUTE", "nonsense")
    with pytest.raises(ValueError):
        MoELayer(32, 4, 2, dtype=torch.float32)
    monkeypatch.setenv("TEPDIST_MOE_ROUTE", "fused")
    assert MoELayer(32, 4, 2, dtype=torch.float32).route == "fused"
    monkeypatch.delenv("TEPDIST_MOE_ROUTE")
    assert MoELayer(32, 4, 2, dtype=torch.float32).route == "auto"
