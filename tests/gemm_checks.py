"""Cases, inputs and criteria for the 128-tile hand GEMM (ops/csrc/gemm.hip),
shared by test_gemm128_edges_gpu.py (the kernel) and test_gemm_oracle_cpu.py
(a CPU stand-in, and deliberately wrong stand-ins that the criteria must
reject). Pure torch; the backend is passed in.

A backend has one method,

    gemm(a, b, a_kc, b_kc, M, N, K, lda, ldb, sa, sb, batch, bias, epi,
         out, out_pre, ws_fill=None)

with the meaning of hip._gemm_raw: `a` and `b` are the operands as stored
(a is [Bt, M, K] when a_kc else [Bt, K, M], b is [Bt, N, K] when b_kc else
[Bt, K, N], row stride ld, batch stride sa / sb in elements, 0 = broadcast),
`out` and `out_pre` are contiguous [batch, M, N] views it writes. ws_fill,
when given, is the value a split plan's workspace holds before the call.

Three oracles, all independent of ops/reference.py and of the kernel:

  int   operands are integers in [-8, 8] (bias: distinct integers per
        column, |bias| <= 63), so every fp32 partial sum is exact in any
        order (64 K + 63 < 2^24) and the result must be the bits of the
        float64 product rounded once to bf16.
  sel   one operand is a signed selection matrix (one +-1 per output row or
        column, at a permuted k), the other is randn spread over forty
        binades. Every output element is a single product by +-1: C is a
        signed, permuted copy of the dense operand, bit for bit, with all
        eight mantissa bits and many exponents in play.
  rand  randn operands: |got - fp64| <= 1 bf16 ulp of the fp64 value
        + K * 2^-23 * (|a| @ |b| + |bias|), per element. The floor is the
        bound of an fp32 sum of K terms taken in any order (K - 1 additions,
        each within 2^-24 relative of a partial sum no larger than the sum
        of the magnitudes), doubled because MFMA accumulation is not
        promised to round to nearest. Split-K keeps fp32 partials and rounds
        once, so the same floor holds. Relative to an ulp of a typical
        element (|c| ~ sqrt(K)) it grows as K^1.5: ~1e-2 ulp at K = 64,
        ~6e-2 at K = 320, so there each element is held to 1 ulp of its own
        value; at the split cases' K ~ 2000 it passes one ulp, and the
        sharp check of those is `int`.

The gelu epilogues (epi 2, 3) return the rounded pre-activation c_pre and
c = gelu(c_pre): c_pre is held to `int` / `rand`, c to the float64 gelu of
the c_pre the backend returned under rowwise_checks.gelu_floor.

Operands are views into larger buffers whose every other element is NaN
(before the first element, between a row's extent and its ld, between batch
elements, and a whole tile of rows after the last), so anything read outside
[F, K] turns the result NaN instead of leaving the allocation. Outputs are
views into buffers filled with a NaN sentinel that must be bit-identical
outside [batch, M, N] afterwards, and finite inside. Every operand base is
16-byte aligned.
"""

import zlib
from typing import NamedTuple, Optional, Tuple

import torch

import rowwise_checks as rc
from tepdist_amd.ops import fp64_reference as o

BF16 = torch.bfloat16
GUARD = 64                 # elements before an operand / output
SENT = 0x7FA5              # the outputs' sentinel: a NaN with its own payload
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]


class Case(NamedTuple):
    name: str
    M: int
    N: int
    K: int
    a_kc: bool
    b_kc: bool
    pad_a: int = 0          # lda - (K when a_kc else M)
    pad_b: int = 0
    epi: int = 0
    batch: int = 1
    bcast: str = ""         # "a" / "b": that operand has stride 0
    oracles: Tuple[str, ...] = ("int", "rand")
    kernel: int = 128       # what the plan must give
    split: Tuple[int, int] = (1, 0)

    @property
    def lda(self):
        return (self.K if self.a_kc else self.M) + self.pad_a

    @property
    def ldb(self):
        return (self.K if self.b_kc else self.N) + self.pad_b

    @property
    def lay(self):
        return ("kc" if self.a_kc else "ko") + "," + \
            ("kc" if self.b_kc else "ko")


def _case(family, M, N, K, lay, tag="", **kw):
    c = Case("", M, N, K, lay[0], lay[1], **kw)
    return c._replace(name=f"{family}-{M}x{N}x{K}-{c.lay}{tag}")


def _build_cases():
    out = []
    # K pipeline: one, two, three and five K-tiles
    for K in (64, 128, 192, 320):
        out += [_case("pipe", 128, 128, K, lay) for lay in LAYOUTS]
    # K tails; with k-contiguous operands an odd K is also an odd ld (element
    # loads). "-ld8": the same K in rows padded to 16 bytes, so the DMA runs
    # the full tiles and registers only the tail tile of the same operand.
    for K in (1, 7, 8, 9, 63, 65, 72, 127, 136):
        for lay in LAYOUTS:
            out.append(_case("ktail", 128, 128, K, lay))
            if K % 8 and (lay[0] or lay[1]):
                p = -K % 8
                out.append(_case("ktail", 128, 128, K, lay, "-ld8",
                                 pad_a=p if lay[0] else 0,
                                 pad_b=p if lay[1] else 0))
    # M/N edges: one operand by DMA and the other through registers, odd
    # extents of k-outer operands
    for M, N, K in [(1, 1, 64), (129, 128, 64), (128, 129, 64),
                    (127, 130, 136), (200, 136, 72), (257, 255, 200),
                    (130, 67, 64)]:
        out += [_case("edge", M, N, K, lay) for lay in LAYOUTS]
    # leading dimensions: 16-byte rows, 4-byte rows, odd rows
    for M, N, K in [(200, 136, 72), (128, 128, 136)]:
        for d in (8, 2, 3):
            out += [_case("ld", M, N, K, lay, f"-ld+{d}", pad_a=d, pad_b=d)
                    for lay in LAYOUTS]
    # grids that are no multiple of 8 blocks (15 and 9): the XCD remap
    for M, N, K in [(384, 640, 64), (1152, 128, 64)]:
        out += [_case("grid", M, N, K, lay, oracles=("int",))
                for lay in LAYOUTS]
    # split-K: 16 chunks of 128; 17 chunks, the last 8 elements long, and
    # M*N % 4 == 2 (the reduce kernel's scalar tail, odd parts at 8-byte
    # addresses); 11 chunks of 192
    for (M, N, K), split in [((128, 128, 2048), (16, 128)),
                             ((130, 67, 2056), (17, 128)),
                             ((200, 136, 2112), (11, 192))]:
        for lay in LAYOUTS:
            rand = (K, lay) in [(2056, (True, True)), (2112, (False, True))]
            out.append(_case("split", M, N, K, lay, split=split,
                             oracles=("int", "rand") if rand else ("int",)))
    # batched: per-batch strides, then each operand broadcast
    for bc in ("", "a", "b"):
        out += [_case("batch", 129, 136, 72, lay, f"-bc{bc or '0'}", batch=3,
                      bcast=bc) for lay in LAYOUTS]
    # epilogues, k-contiguous and with a k-outer B (the dgrad layout)
    for epi in (1, 2, 3):
        for M, N, K in [(128, 128, 64), (200, 136, 72), (257, 255, 200)]:
            out += [_case(f"epi{epi}", M, N, K, lay, epi=epi)
                    for lay in LAYOUTS[:2]]
    return out


CASES = _build_cases()
# selection oracle: an interior shape, a partial-tile shape, a K-tail shape
# and one that is both; the selection on either side
SEL_CASES = [_case("sel", M, N, K, lay, f"-{side}", oracles=(f"sel_{side}",))
             for M, N, K in [(128, 128, 192), (257, 255, 200), (128, 128, 65),
                             (127, 130, 136)]
             for lay in LAYOUTS for side in "ab"]
# the 256 kernel's gelu epilogues, per element (test_gemm256_stagger_gpu.py
# holds the same shapes to its max-norm bound)
EPI256_CASES = [_case(f"epi{epi}", M, N, K, LAYOUTS[0], "-256", epi=epi,
                      kernel=256)
                for epi in (2, 3) for M, N, K in [(256, 256, 128),
                                                  (512, 256, 320)]]
ALL_CASES = CASES + SEL_CASES + EPI256_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def check_plan(ext, case):
    """The plan gives `case` the kernel and split it is here to exercise."""
    got = ext.gemm_plan(case.M, case.N, case.K, case.lda, case.ldb,
                        case.a_kc, case.b_kc, case.epi, case.batch)
    assert got == (case.kernel,) + case.split + ("",), (case.name, got)


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------

def _gen(case, salt):
    return torch.Generator().manual_seed(
        zlib.crc32(f"{case.name}/{salt}".encode()))


def _nb(case, side):
    return 1 if case.bcast == side else case.batch


def int_inputs(case):
    g = _gen(case, "int")
    a = torch.randint(-8, 9, (_nb(case, "a"), case.M, case.K), generator=g)
    b = torch.randint(-8, 9, (_nb(case, "b"), case.N, case.K), generator=g)
    # distinct per column: n+-1 differs by 5, n+-16 by 80 (mod 127)
    bias = (torch.arange(case.N) * 5 % 127 - 63) if case.epi in (1, 2) \
        else None
    assert 64 * case.K + 63 < 2 ** 24
    return a.to(BF16), b.to(BF16), None if bias is None else bias.to(BF16)


def rand_inputs(case):
    g = _gen(case, "rand")
    a = torch.randn(_nb(case, "a"), case.M, case.K, generator=g).to(BF16)
    b = torch.randn(_nb(case, "b"), case.N, case.K, generator=g).to(BF16)
    bias = torch.randn(case.N, generator=g).to(BF16) \
        if case.epi in (1, 2) else None
    return a, b, bias


def sel_inputs(case, side):
    """Returns (a, b, want): logical a [1, M, K], b [1, N, K] and the exact
    bf16 result [1, M, N]."""
    g = _gen(case, "sel")
    M, N, K = case.M, case.N, case.K
    F, G = (M, N) if side == "a" else (N, M)      # selection rows, dense rows
    perm = torch.randperm(K, generator=g)
    kidx = perm[torch.arange(F) % K]
    sign = (torch.randint(0, 2, (F,), generator=g) * 2 - 1).to(BF16)
    sel = torch.zeros(F, K, dtype=BF16)
    sel[torch.arange(F), kidx] = sign
    dense = torch.randn(G, K, generator=g).to(BF16)
    dense[dense == 0] = 1.0                       # -1 * 0 + 0 is +0, not -0
    dense = torch.ldexp(dense.float(), torch.randint(
        -20, 21, (G, K), generator=g)).to(BF16)   # exact: a power of two
    picked = dense[:, kidx] * sign                # [G, F], exact
    if side == "a":
        return sel[None], dense[None], picked.t().contiguous()[None]
    return dense[None], sel[None], picked.contiguous()[None]


def _place(vals, kc, pad, dev):
    """Stores logical [Bt, F, K] values as the kernel reads them, inside a
    NaN-filled buffer. Returns (stored view on dev, ld, batch stride)."""
    st = vals if kc else vals.transpose(-1, -2)
    Bt, R, C = st.shape
    ld = C + pad
    bs = R * ld + 16
    flat = torch.full((GUARD + Bt * bs + 128 * ld + 128,), float("nan"),
                      dtype=BF16)
    torch.as_strided(flat, (Bt, R, C), (bs, ld, 1), GUARD).copy_(st)
    flat = flat.to(dev)
    view = torch.as_strided(flat, (Bt, R, C), (bs, ld, 1), GUARD)
    assert view.data_ptr() % 16 == 0
    return view, ld, bs


def _sentinel_buffer(n, dev):
    return torch.full((GUARD + n + GUARD,), SENT,
                      dtype=torch.int16).view(BF16).to(dev)


def _collect(flat, case, what):
    n = case.batch * case.M * case.N
    bits = flat.cpu().view(torch.int16)
    assert bool((bits[:GUARD] == SENT).all()) and \
        bool((bits[GUARD + n:] == SENT).all()), \
        f"{what}: wrote outside its [{case.batch}, {case.M}, {case.N}]"
    got = bits[GUARD:GUARD + n].view(BF16).view(case.batch, case.M, case.N)
    assert bool(torch.isfinite(got).all()), \
        f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite " \
        "(unwritten, or computed from data outside the operands)"
    return got


def run(be, dev, case, a, b, bias, ws_fill=None):
    """Runs `case` on logical CPU operands a [Bt, M, K], b [Bt, N, K].
    Returns (c, c_pre) as CPU [batch, M, N] tensors (c_pre None below
    epi 2), after the sentinel and finiteness checks."""
    a_st, lda, sa = _place(a, case.a_kc, case.pad_a, dev)
    b_st, ldb, sb = _place(b, case.b_kc, case.pad_b, dev)
    assert (lda, ldb) == (case.lda, case.ldb)
    n = case.batch * case.M * case.N
    shape = (case.batch, case.M, case.N)
    c_flat = _sentinel_buffer(n, dev)
    p_flat = _sentinel_buffer(n, dev) if case.epi >= 2 else None
    be.gemm(a_st, b_st, case.a_kc, case.b_kc, case.M, case.N, case.K, lda,
            ldb, sa if a.shape[0] > 1 else 0, sb if b.shape[0] > 1 else 0,
            case.batch, None if bias is None else bias.to(dev), case.epi,
            c_flat[GUARD:GUARD + n].view(shape),
            None if p_flat is None else p_flat[GUARD:GUARD + n].view(shape),
            ws_fill=ws_fill)
    c = _collect(c_flat, case, f"{case.name} c")
    pre = None if p_flat is None else _collect(p_flat, case,
                                               f"{case.name} c_pre")
    return c, pre


# --------------------------------------------------------------------------
# the criteria
# --------------------------------------------------------------------------

def _gelu_of_pre(case, c, pre, key):
    p64 = o.f64(pre)
    rc.judge(c, o.gelu_fwd(pre), rc.gelu_floor(p64),
             f"gemm{case.kernel} gelu {key}[{case.name}]")


def check_int(be, dev, case, ws_fill=None):
    a, b, bias = int_inputs(case)
    want = o.gemm(a, b, True, True, bias)[0]
    assert float(want.abs().max()) < 2 ** 24
    # + 0.0: the sign of an exact zero is not held. A lone product -a * 0 is
    # -0 in the float64 product, and +0 once added to an accumulator.
    want = want.to(BF16).expand(case.batch, case.M, case.N) + 0.0
    c, pre = run(be, dev, case, a, b, bias, ws_fill)
    if case.epi >= 2:
        rc.assert_bits_equal(pre + 0.0, want, f"{case.name} int c_pre")
        _gelu_of_pre(case, c, pre, "int")
    else:
        rc.assert_bits_equal(c + 0.0, want, f"{case.name} int")


def check_sel(be, dev, case, side):
    a, b, want = sel_inputs(case, side)
    c, _ = run(be, dev, case, a, b, None)
    rc.assert_bits_equal(c, want, f"{case.name} sel")


def check_rand(be, dev, case):
    a, b, bias = rand_inputs(case)
    ref, mag = o.gemm(a, b, True, True, bias)
    shape = (case.batch, case.M, case.N)
    ref, mag = ref.expand(shape), mag.expand(shape)
    floor = case.K * 2.0 ** -23 * mag
    c, pre = run(be, dev, case, a, b, bias)
    key = f"gemm{case.kernel} rand {case.lay}"
    if case.epi >= 2:
        rc.judge(pre, ref, floor, f"{key}[{case.name} c_pre]")
        _gelu_of_pre(case, c, pre, "rand")
    else:
        rc.judge(c, ref, floor, f"{key}[{case.name}]")


def check(be, dev, case, oracle):
    if oracle == "int":
        check_int(be, dev, case)
    elif oracle == "rand":
        check_rand(be, dev, case)
    elif oracle in ("sel_a", "sel_b"):
        check_sel(be, dev, case, oracle[-1])
    else:
        raise ValueError(oracle)


def check_all(be, dev, case):
    for oracle in case.oracles:
        check(be, dev, case, oracle)


def measured_lines():
    """The figures of docs/KERNELS.md: per key, the largest error as a
    fraction of 1 ulp + floor (and in ulps) over everything judged so far."""
    return [f"{key:28s} {frac:6.3f} of the bound, {anywhere:6.3f} ulp"
            for key, (_, anywhere, frac) in sorted(rc.MEASURED.items())
            if key.startswith("gemm")]
