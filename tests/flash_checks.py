"""Cases, inputs and derived error floors for the flash attention kernels
(ops/csrc/attention.hip), shared by test_flash_oracle_cpu.py (a plain-torch
emulation of the kernels' arithmetic, and wrong variants of it) and
test_flash_edges_gpu.py (the HIP kernels): both run the same check_*
functions with the same seeded CPU inputs and the same floors against the
float64 oracles of tepdist_amd/ops/fp64_reference.py.

The criterion is rowwise_checks.judge: per element, |got - fp64| <= 1 ulp of
the fp64 value + floor. The floors follow the kernels' rounding points.
U = 2^-24 (one fp32 rounding). H8 = 2^-8 is the relative error of rounding
P or dS to bf16 ahead of the second MFMA: half a bf16 ulp is 2^-8 of a
value at the bottom of its binade and 2^-9 at the top, and the kernel
rounds p~ = p * l * exp(m_final - m_then), whose place in its binade the
oracle cannot know. 2^-9 is not a bound: where a row rests on two keys
(the diag inputs: dq = scale * dS_a (k_a - k_b)) nothing averages, and with
2^-9 the emulation below, which rounds exactly there and nowhere else,
left 1 to 3 % of the dq elements of every diag case outside (worst 1.83
times the allowed error; dk 1.66, dv 1.36, out 1.15). With 2^-8 its worst
element is at 0.97. With ss = scale * q.k, p the softmax and T =
ceil(S / 64) kv tiles:

  rel_ij   the relative fp32 error of one probability. P is exp2 of
           fma(s, scale*log2e, -m*log2e): the constant scale*log2e is
           rounded (1.5 U with log2e's own representation error), so is
           -m*log2e, and the fma rounds |ss - m| * log2e once; times ln 2
           that is 1.5 U (|ss| + |m|) + U |ss - m| <= 2.5 U (|ss| + |m|).
           The alpha = exp2((m_old - m_new) * log2e) chain that carries
           earlier tiles to the final maximum adds the same form once more
           (the increments of m sum to under 2 max|ss|), and exp2 itself 2 U.
           Forward: rel = (4 (|ss_ij| + max_j |ss_ij|) + 8) U.
           Backward (m replaced by the lse it was given, no alpha chain,
           same form kept): relb = (4 (|ss_ij| + |lse_i|) + 8) U.
  c_acc    fp32 accumulation: the MFMA adds 32-term partial dot products
           into its accumulator, S / 32 roundings, the row sum l takes 16
           per-lane adds + 2 shuffles + the alpha multiply and add per
           tile (4 T), and 64 covers the partial products' own roundings,
           the final 1 / l and the multiplication by it:
           c_acc = (S / 32 + 4 T + 64) U.

  out      (H8 + c_acc) * A + sum_j p rel |v| + (sum_j p rel) * A
           with A = sum_j p_ij |v_jd|: P's rounding, each term's own
           relative error, and the denominator's (the p-weighted mean of
           rel) on the whole sum.
  lse      fp32: sum_j p rel + c_acc (the relative error of l is the
           absolute error of its logarithm) + 8 U max(1, |lse|) for
           m = max * scale, __logf, its scaling by ln 2 and the final add.
  dv       sum_i p^ (H8 + relb + c_acc) |dout|.
  dq, dk   dS = p^ (dP - delta) is formed in fp32 and rounded to bf16.
           dP is a D-term fp32 dot product and so is delta: where they
           cancel, their absolute error E_ij = D U (sum_d |dout||v| +
           sum_d |dout||out|) is what is left, carried by p^. So
           err(dS_ij) = |dS_ij| (H8 + relb + 2 U + c_acc) + p^_ij E_ij and
           the floors are scale * sum_j err(dS) |k| and scale * sum_i
           err(dS) |q|.

Results under 2^-126 may flush to zero in fp32 (exp2's output, a product):
each floor carries that as FTZ times the factor the flushed value would
have been multiplied by.

A term would be enlarged only where the GPU kernels measurably exceeded it,
with the reason and the measured factor written beside it. None had to be:
on the MI355X the worst element of any case is at 0.63 (out), 0.10 (lse),
0.72 (dv), 0.93 (dq) and 0.85 (dk) of its allowed error (docs/KERNELS.md).

`cap`: None asserts every element (the GPU tests). The CPU proof passes
1e-4, as test_fp64_reference_cpu.py does. `sink`: a dict; when given
nothing is asserted and the largest error / allowed error per output is
recorded in it (how the CPU proof shows which check a wrong variant fails,
and by what factor).
"""

import math

import torch

import rowwise_checks as rc
from tepdist_amd import ops
from tepdist_amd.ops import fp64_reference as o

BF16 = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24
H8 = 2.0 ** -8
FTZ = 2.0 ** -126
LOG2E = 1.4426950408889634
NO_LSE = o.NO_LSE
KB = 64               # kv rows per tile, every kernel
PAD_ROWS = 70         # NaN rows behind the `padding` inputs

# Kernel constants behind the shapes: kv tile 64, q pairs of 32; D = 64:
# fwd/dQ block 512, dK/dV block 256 in 128-slabs; D = 128: 256 and 128.
# One row; either side of a pair and of a tile; one row into the second
# slab, the second dK/dV block and the second fwd/dQ block; both blocks full.
SEQS = {64: [1, 31, 33, 63, 64, 65, 129, 200, 257, 513, 520, 1024],
        128: [1, 65, 129, 257, 328, 640]}
# (2, 3) heads: bh / H, bh % H and the packed layout's head strides, at one
# ragged and one multi-block S per D
MULTI_HEAD = {64: [200, 520], 128: [65, 328]}
DIAG_PATTERNS = ["self", "first", "tile_start", "prev", "rand"]
KINDS = ["randn", "uniform", "uniform_k0"] + \
    ["diag:" + p for p in DIAG_PATTERNS] + ["next", "padding"]


def cases_4d():
    """(D, S, causal, kind) of the 4-D entry points at B = H = 1."""
    for D, seqs in SEQS.items():
        for S in seqs:
            for kind in KINDS:
                for causal in (True, False):
                    if kind == "next" and not causal:
                        continue
                    yield D, S, causal, kind


def cases_layout():
    """(B, H, D, S, causal, kind, layout): several heads in every layout,
    the packed and transposed-view layouts at one head, NaN padding behind
    the packed layout."""
    for D, seqs in MULTI_HEAD.items():
        for S in seqs:
            for causal in (True, False):
                for layout in ("4d", "packed", "4d_noncontig"):
                    yield 2, 3, D, S, causal, "randn", layout
                yield 1, 3, D, S, causal, "padding", "packed"
                yield 1, 1, D, S, causal, "diag:rand", "packed"
                yield 1, 1, D, S, causal, "uniform", "4d_noncontig"


# --------------------------------------------------------------------------
# Inputs (all seeded on the CPU)
# --------------------------------------------------------------------------

def _targets(pattern, S, g):
    i = torch.arange(S)
    if pattern == "self":
        return i
    if pattern == "first":
        return torch.zeros_like(i)
    if pattern == "tile_start":
        return i // KB * KB
    if pattern == "prev":
        return (i - 1).clamp_min(0)
    if pattern == "rand":
        return (torch.rand(S, generator=g) * (i + 1)).long().clamp_max(i)
    raise AssertionError(pattern)


def _diag_qk(pattern, B, H, S, D, causal, g):
    """k_j in {+-1}^D, q_i = beta (k_i + k_t(i)): keys i and t(i) <= i get
    the same score beta (D + k_i.k_t) / sqrt(D). beta >= 3 is raised until
    they lead every other key the row may see by >= 10 nats; the keys are
    drawn again (same generator) while some row's lead at beta = 1 is under
    0.25, which keeps beta <= 40 and q exact in bf16."""
    scale = 1.0 / math.sqrt(D)
    i = torch.arange(S)
    for _ in range(50):
        k = (torch.randint(0, 2, (B, H, S, D), generator=g) * 2 - 1).to(F64)
        t = _targets(pattern, S, g)
        q1 = k + k[:, :, t]
        ss = q1 @ k.transpose(-1, -2) * scale
        other = torch.ones(S, S, dtype=torch.bool)
        if causal:
            other &= i[None, :] <= i[:, None]
        other[i, i] = False
        other[i, t] = False
        rest = ss.masked_fill(~other, -math.inf).max(-1).values
        lead = float((ss[:, :, i, i] - rest).min())
        if lead >= 0.25:
            break
    else:
        raise AssertionError("no dominated key set in 50 draws")
    beta = max(3.0, math.ceil(10.0 / lead * 8) / 8)
    return (beta * q1).to(BF16), k.to(BF16)


def flash_inputs(kind, B, H, S, D, causal):
    """Returns bf16 (q, k, v, dout), each [B, H, S, D]."""
    g = rc.gen(7919 * S + 13 * D + 101 * KINDS.index(kind) + B * H
               + (1 if causal else 0))
    shape = (B, H, S, D)
    v, dout = rc.randn(g, *shape), rc.randn(g, *shape)
    if kind in ("randn", "padding"):
        return rc.randn(g, *shape), rc.randn(g, *shape), v, dout
    if kind in ("uniform", "uniform_k0"):
        # every allowed score is 0, every p~ exactly 1: with V[j] = e_(j mod
        # D), out[i][c] is the number of allowed keys j = c (mod D) over
        # their total. uniform_k0 is the twin whose dK does not vanish.
        x, z = rc.randn(g, *shape), torch.zeros(shape, dtype=BF16)
        v = torch.zeros(shape, dtype=BF16)
        j = torch.arange(S)
        v[:, :, j, j % D] = 1.0
        return (z, x, v, dout) if kind == "uniform" else (x, z, v, dout)
    if kind == "next":
        # the dominant key of row i is i + 1, the first one the causal mask
        # hides: a correct kernel returns an ordinary softmax over the rest
        k = (torch.randint(0, 2, (B, H, S + 1, D), generator=g) * 2 - 1)
        return (3.0 * k[:, :, 1:]).to(BF16), k[:, :, :S].to(BF16), v, dout
    q, k = _diag_qk(kind.split(":")[1], B, H, S, D, causal, g)
    return q, k, v, dout


# --------------------------------------------------------------------------
# Running a backend in one of the layouts
# --------------------------------------------------------------------------

def _place(t, dev, pad):
    """t on `dev`; with pad, as the [:S] slice along dim -2 of a buffer
    whose further PAD_ROWS rows hold NaN. The slice must be contiguous (one
    batch entry, and one head in the 4-D layout), so that no wrapper copies
    it and the NaN rows do lie behind the rows the kernel may read."""
    if not pad:
        return t.to(dev)
    S = t.shape[-2]
    buf = torch.full(t.shape[:-2] + (S + PAD_ROWS, t.shape[-1]),
                     float("nan"), dtype=t.dtype)
    buf[..., :S, :] = t
    view = buf.to(dev)[..., :S, :]
    assert view.is_contiguous(), "padding needs a slice that stays a view"
    return view


def _pack(t):
    B, H, S, D = t.shape
    return t.transpose(1, 2).reshape(B, S, H * D)


def _unpack(t, H):
    B, S, d = t.shape
    return t.reshape(B, S, H, d // H).transpose(1, 2)


def run_flash(be, dev, layout, q, k, v, dout, causal, pad=False):
    """Forward and backward of `be` in `layout`. Returns CPU tensors (out,
    lse, dq, dk, dv): [B, H, S, D], lse [B, H, S]. On a GPU the packed and
    transposed-view layouts go through the autograd functions of
    tepdist_amd.ops, as the models call them; a CPU stand-in is called
    directly (ops dispatches CPU tensors to ops/reference.py)."""
    B, H, S, D = q.shape
    autograd = str(dev) != "cpu"
    if layout == "4d":
        qd, kd, vd, dd = (_place(t, dev, pad) for t in (q, k, v, dout))
        out, res = be.attention_fwd(qd, kd, vd, causal=causal)
        assert len(res) == 2, "not the flash path"
        lse = res[1]
        dq, dk, dv = be.attention_bwd(dd, qd, kd, vd, res, causal=causal)
    elif layout == "packed":
        qkv = _place(torch.cat([_pack(t) for t in (q, k, v)], -1), dev, pad)
        dd = _place(_pack(dout), dev, pad)
        if autograd:
            qkv.requires_grad_()
            outp = ops.attention_qkv(qkv, H, causal=causal)
            lse = outp.grad_fn.saved_tensors[-1]
            assert lse.dtype == torch.float32, "not the flash path"
            outp.backward(dd)
            dqkv = qkv.grad
        else:
            outp, res = be.attention_qkv_fwd(qkv, H, causal=causal)
            lse = res[1]
            dqkv = be.attention_qkv_bwd(dd, qkv, H, res, causal=causal)
        out = _unpack(outp.detach(), H)
        dq, dk, dv = (_unpack(t, H) for t in dqkv.split(H * D, dim=-1))
    elif layout == "4d_noncontig":
        assert not pad
        # [B, S, H, D] storage seen as [B, H, S, D]: what a model holds
        # after reshape(B, S, H, D).transpose(1, 2) without .contiguous()
        qd, kd, vd, dd = (t.transpose(1, 2).contiguous().to(dev)
                          .transpose(1, 2) for t in (q, k, v, dout))
        assert not qd.is_contiguous() or H == 1 or S == 1
        if autograd:
            for t in (qd, kd, vd):
                t.requires_grad_()
            out = ops.attention(qd, kd, vd, causal=causal)
            lse = out.grad_fn.saved_tensors[-1]
            assert lse.dtype == torch.float32, "not the flash path"
            out.backward(dd)
            dq, dk, dv = qd.grad, kd.grad, vd.grad
            out = out.detach()
        else:
            out, res = be.attention_fwd(qd, kd, vd, causal=causal)
            lse = res[1]
            dq, dk, dv = be.attention_bwd(dd, qd, kd, vd, res, causal=causal)
    else:
        raise AssertionError(layout)
    return (out.detach().cpu(), lse.detach().cpu().reshape(B, H, S),
            dq.detach().cpu(), dk.detach().cpu(), dv.detach().cpu())


# --------------------------------------------------------------------------
# Floors
# --------------------------------------------------------------------------

def _c_acc(S):
    return (S / 32 + 4 * math.ceil(S / KB) + 64) * U


def fwd_floors(q, k, v, causal, scale, p, rlse):
    """(floor of out, floor of lse); see the module docstring."""
    S = q.shape[-2]
    s, allowed = o.attention_scores(q, k, causal, scale)
    ss = s.abs() * allowed
    rel = (4 * (ss + ss.max(-1, keepdim=True).values) + 8) * U
    av = o.f64(v).abs()
    A = p @ av
    prel = p * rel
    mean_rel = prel.sum(-1, keepdim=True)
    fl_out = (H8 + _c_acc(S) + mean_rel) * A + prel @ av \
        + FTZ * av.sum(-2, keepdim=True)
    fl_lse = mean_rel[..., 0] + _c_acc(S) + 8 * U * rlse.abs().clamp_min(1.0)
    return fl_out, fl_lse


def bwd_floors(dout, q, k, v, out, lse, causal, scale):
    """(floor of dq, of dk, of dv) for the (out, lse) the backward was
    given; see the module docstring."""
    S, D = q.shape[-2], q.shape[-1]
    sc = o.f32r(scale)
    s, allowed = o.attention_scores(q, k, causal, scale)
    ph = o.attention_p_given_lse(q, k, lse, causal, scale)
    l = o.f64(lse).reshape(s.shape[:-1])[..., None]
    l = torch.where(l > -1.0e38, l.abs(), torch.zeros_like(l))
    relb = (4 * (s.abs() * allowed + l) + 8) * U
    do, v64 = o.f64(dout), o.f64(v)
    dpd = (do @ v64.transpose(-1, -2)
           - (do * o.f64(out)).sum(-1, keepdim=True))        # dP - delta
    E = D * U * (do.abs() @ v64.abs().transpose(-1, -2)
                 + (do * o.f64(out)).abs().sum(-1, keepdim=True))
    errs = (ph * dpd).abs() * (H8 + relb + 2 * U + _c_acc(S)) + ph * E \
        + FTZ * (dpd.abs() + 1.0)
    fl_dq = sc * (errs @ o.f64(k).abs()) + FTZ
    fl_dk = sc * (errs.transpose(-1, -2) @ o.f64(q).abs()) + FTZ
    fl_dv = (ph * (H8 + relb + _c_acc(S)) + FTZ).transpose(-1, -2) @ do.abs()
    return fl_dq, fl_dk, fl_dv


def _judge(got, ref64, floor, what, cap, sink):
    if sink is None:
        return rc.judge(got, ref64, floor, what, cap)
    err, _, tol = o.ulp_error(got, ref64, floor)
    worst = float(torch.nan_to_num(err / tol, nan=math.inf).max())
    key = what.split("[")[0]
    sink[key] = max(sink.get(key, 0.0), worst)


def judge_bwd(got, dout, q, k, v, out, lse, causal, tag, cap, sink,
              only_dv=False):
    """got = (dq, dk, dv) against the oracle of the (out, lse) given."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    rdq, rdk, rdv = o.attention_bwd(dout, q, k, v, out, lse, causal, scale)
    fl_dq, fl_dk, fl_dv = bwd_floors(dout, q, k, v, out, lse, causal, scale)
    _judge(got[2], rdv, fl_dv, "flash_bwd.dv" + tag, cap, sink)
    if only_dv:
        return
    _judge(got[0], rdq, fl_dq, "flash_bwd.dq" + tag, cap, sink)
    _judge(got[1], rdk, fl_dk, "flash_bwd.dk" + tag, cap, sink)


# --------------------------------------------------------------------------
# The checks
# --------------------------------------------------------------------------

def check_flash(be, dev, B, H, S, D, causal, kind, layout="4d", cap=None,
                sink=None):
    q, k, v, dout = flash_inputs(kind, B, H, S, D, causal)
    scale = 1.0 / math.sqrt(D)
    tag = (f"[{B}x{H}x{S}x{D} {'causal' if causal else 'full'} {kind} "
           f"{layout}]")
    out, lse, dq, dk, dv = run_flash(be, dev, layout, q, k, v, dout, causal,
                                     pad=(kind == "padding"))
    rout, rlse, p = o.attention_fwd(q, k, v, causal, scale)
    fl_out, fl_lse = fwd_floors(q, k, v, causal, scale, p, rlse)
    _judge(out, rout, fl_out, "flash_fwd.out" + tag, cap, sink)
    _judge(lse, rlse, fl_lse, "flash_fwd.lse" + tag, cap, sink)
    # the backward against the oracle of the (out, lse) it was given. With
    # one dominant key (diag:self) dP - delta cancels to rounding noise and
    # only dv carries information.
    judge_bwd((dq, dk, dv), dout, q, k, v, out, lse, causal, tag, cap, sink,
              only_dv=(kind == "diag:self"))


GLOBAL_LSE_S = {64: 200, 128: 328}


def check_flash_bwd_global_lse(be, dev, D, sentinel=False, cap=None,
                               sink=None):
    """The ring-attention backward: attention_bwd(causal=False) on one
    block of the keys with the (out, lse) of ALL keys, so that the block's
    p^ sums to under 1. The S keys of a non-causal problem are split into
    two unequal parts, each padded with zero rows to S (the kernels take
    one S for queries and keys); the zero rows are keys like any other
    (score 0, value 0) of the global problem, which therefore has 2 S keys.
    With `sentinel`, every other row carries NO_LSE: such a row must get
    dq = 0 and add exactly nothing to dk and dv."""
    B, H, S = 1, 2, GLOBAL_LSE_S[D]
    g = rc.gen(S + D + (5 if sentinel else 0))
    q, k, v, dout = (rc.randn(g, B, H, S, D) for _ in range(4))
    a = 2 * S // 3 + 3
    tag = f"[global lse {S}x{D}{' sentinel' if sentinel else ''}]"

    def padded(t, lo, hi):
        z = torch.zeros_like(t)
        z[:, :, :hi - lo] = t[:, :, lo:hi]
        return z
    halves = [(padded(k, 0, a), padded(v, 0, a)),
              (padded(k, a, S), padded(v, a, S))]
    qd, dd = q.to(dev), dout.to(dev)
    parts = []
    for kh, vh in halves:
        out_h, res = be.attention_fwd(qd, kh.to(dev), vh.to(dev),
                                      causal=False)
        parts.append((o.f64(out_h), o.f64(res[1]).reshape(B, H, S)))
    # merged on the CPU in float64, rounded to what the kernel stores
    lse64 = torch.logaddexp(parts[0][1], parts[1][1])
    out_g = sum(oh * (lh - lse64).exp()[..., None]
                for oh, lh in parts).to(BF16)
    lse_g = lse64.to(torch.float32)
    rows = torch.arange(S) % 2 == 1
    if sentinel:
        lse_g[:, :, rows] = NO_LSE
    res_g = (out_g.to(dev), lse_g.reshape(B * H, S).to(dev))
    for n, (kh, vh) in enumerate(halves):
        got = tuple(t.detach().cpu() for t in be.attention_bwd(
            dd, qd, kh.to(dev), vh.to(dev), res_g, causal=False))
        judge_bwd(got, dout, q, kh, vh, out_g, lse_g, False,
                  tag[:-1] + f" part {n}]", cap, sink)
        if not sentinel or sink is not None:
            continue
        assert not got[0][:, :, rows].any(), \
            "flash_bwd.dq" + tag + ": a row without lse has dq != 0"
        # exactly nothing: other q and dout in those rows, same dk and dv
        q2, d2 = q.clone(), dout.clone()
        q2[:, :, rows] = rc.randn(g, B, H, int(rows.sum()), D)
        d2[:, :, rows] = rc.randn(g, B, H, int(rows.sum()), D)
        _, dk2, dv2 = be.attention_bwd(d2.to(dev), q2.to(dev), kh.to(dev),
                                       vh.to(dev), res_g, causal=False)
        rc.assert_bits_equal(dk2, got[1], "flash_bwd.dk" + tag)
        rc.assert_bits_equal(dv2, got[2], "flash_bwd.dv" + tag)


# --------------------------------------------------------------------------
# The CPU stand-in: the kernels' arithmetic in plain torch
# --------------------------------------------------------------------------

MUTANTS = {
    "a": "rows with q % 64 == 63 also see key q + 1",
    "b": "one 16x16 diagonal block dropped from dK/dV and dQ",
    "c": "keys S .. 64 ceil(S/64) - 1 enter the last ragged pair's "
         "denominator with score 0",
    "d": "key S - 1 dropped when S % 64 == 1",
    "e": "the second q pair of a wave (15 - w) takes the running max/sum "
         "of the first",
    "f": "delta of row i taken from row i ^ 16",
    "g": "backward ignores the given lse and renormalises within the block",
}


class FlashEmulation:
    """ops/csrc/attention.hip in fp32 torch, written from the kernels'
    comments and rounding where they round: kv tiles of 64, online softmax
    on the raw scores with p = exp2(fma(s, scale*log2e, -m*log2e)), P and
    dS rounded to bf16 ahead of the second product, `scale` applied once to
    the dK/dQ sums, rows without a key stored as NO_LSE. `mutant` (a key
    of MUTANTS) turns on one deliberate defect."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def _allowed(self, S, causal):
        """[S, 64 ceil(S/64)]: may query i see (zero-padded) key j."""
        i = torch.arange(S)[:, None]
        j = torch.arange((S + KB - 1) // KB * KB)[None, :]
        ok = (j < S) & ((j <= i) | (not causal))
        if self.mutant == "a":
            ok = ok | ((i % KB == KB - 1) & (j == i + 1) & (j < S))
        if self.mutant == "c" and S % 32:
            ok = ok | ((i >= S // 32 * 32) & (j >= S)
                       & ((j <= i) | (not causal)))
        if self.mutant == "d" and S % KB == 1:
            ok = ok & (j != S - 1)
        return ok

    def attention_fwd(self, q, k, v, causal=True):
        B, H, S, D = q.shape
        f32 = torch.float32
        scale = torch.tensor(1.0 / math.sqrt(D), dtype=f32)
        sl2 = scale * torch.tensor(LOG2E, dtype=f32)
        ok = self._allowed(S, causal)
        Sp = ok.shape[1]
        qf = q.float()
        kf, vf = (torch.zeros(B, H, Sp, D).index_copy_(
            2, torch.arange(S), t.float()) for t in (k, v))
        m = torch.full((B, H, S), NO_LSE, dtype=f32)
        l = torch.zeros(B, H, S)
        acc = torch.zeros(B, H, S, D)
        for kv0 in range(0, S, KB):
            st = qf @ kf[:, :, kv0:kv0 + KB].transpose(-1, -2)
            st = torch.where(ok[:, kv0:kv0 + KB], st,
                             torch.full_like(st, NO_LSE))
            mn = torch.maximum(m, st.max(-1).values * scale)
            alpha = torch.exp2((m - mn) * LOG2E)
            p = torch.exp2(st * sl2 + (-mn * LOG2E)[..., None])
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + \
                p.to(BF16).float() @ vf[:, :, kv0:kv0 + KB]
            m = mn
        if self.mutant == "e" and D == 64:
            r = torch.arange(S)
            pair = r % 512 // 32
            src = torch.where(pair >= 8,
                              r - r % 512 + 32 * (15 - pair) + r % 32, r)
            m, l = m[:, :, src], l[:, :, src]
        has = l > 0
        inv = torch.where(has, 1.0 / l, torch.zeros_like(l))
        out = (acc * inv[..., None]).to(BF16)
        lse = torch.where(has, m + torch.log(l), torch.full_like(l, NO_LSE))
        return out, (out, lse.reshape(B * H, S))

    def attention_bwd(self, dout, q, k, v, residuals, causal=True):
        out, lse = residuals
        B, H, S, D = q.shape
        f32 = torch.float32
        scale = torch.tensor(1.0 / math.sqrt(D), dtype=f32)
        sl2 = scale * torch.tensor(LOG2E, dtype=f32)
        qf, kf, vf, dof = q.float(), k.float(), v.float(), dout.float()
        delta = (dof * out.float()).sum(-1)
        if self.mutant == "f":
            r = torch.arange(S) ^ 16
            delta = delta[:, :, torch.where(r < S, r, torch.arange(S))]
        lse = lse.reshape(B, H, S).float()
        ok = self._allowed(S, causal)[:, :S] & (lse > -1.0e38)[..., None]
        st = qf @ kf.transpose(-1, -2)
        if self.mutant == "g":
            ss = torch.where(ok, st * scale, torch.full_like(st, -math.inf))
            lse = torch.logsumexp(ss, -1)
        arg = st * sl2 + (-lse * LOG2E)[..., None]
        p = torch.exp2(torch.where(ok, arg, torch.full_like(arg, NO_LSE)))
        if self.mutant == "b":
            r0 = 448 if S >= 464 else max(S // 16 - 1, 0) * 16
            p[:, :, r0:r0 + 16, r0:r0 + 16] = 0.0
        ds = p * (dof @ vf.transpose(-1, -2) - delta[..., None])
        p, ds = p.to(BF16).float(), ds.to(BF16).float()
        dq = ((ds @ kf) * scale).to(BF16)
        dk = ((ds.transpose(-1, -2) @ qf) * scale).to(BF16)
        dv = (p.transpose(-1, -2) @ dof).to(BF16)
        return dq, dk, dv

    def attention_qkv_fwd(self, qkv, heads, causal=True):
        q, k, v = (_unpack(t, heads) for t in qkv.chunk(3, dim=-1))
        out, res = self.attention_fwd(q, k, v, causal=causal)
        return _pack(out), (out, res[1])

    def attention_qkv_bwd(self, dout, qkv, heads, residuals, causal=True):
        q, k, v = (_unpack(t, heads) for t in qkv.chunk(3, dim=-1))
        grads = self.attention_bwd(_unpack(dout, heads), q, k, v, residuals,
                                   causal=causal)
        return torch.cat([_pack(t) for t in grads], -1)
