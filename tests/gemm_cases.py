"""Edge cases, references and reference mutants of the GEMM kernels: vt_gemm_nt (csrc/vt_gemm.hip, vt_gemm192.hip, the epilogues of
vt_gemm_epilogue.h), vt_gemm_tn_grouped and vt_decode_norm_linear (csrc/vt_ar.hip).  torch on the CPU only: no GPU and no built library.
The pattern is that of tests/attention_cases.py, tests/gated_cases.py and tests/vq_cases.py; tests/test_gemm_cases_cpu.py proves that the
cases discriminate, tests/test_gemm_edges_gpu.py runs the kernels against them.

EXACT FAMILY (NT_CASES).  Operands are small integers held in bf16, drawn from a generator seeded by the case's name: A in [-2, 2], B in
[-3, 3] times a per-case integer `bscale`.  Bias, residual, rowmod and the aux of VT_EPI_BF16_MULAUX are multiples of 1/4, out_scale is a
power of two, |acc| < 2^21.  Every fp32 sum is then exact in any order (split-K partials included), so the expected output is a bit
pattern.  `nt_reference` evaluates in float64 in the order of nt_epilogue -- bias, round_bf16, residual at omap(m), rowmod at m % period,
out_scale, out2 = bf16(out) -- and asserts that every value it rounds to fp32 is representable: the exactness claim is checked, not
assumed.  For the MULAUX column sums it asserts sum |out| < 2^20 per slab as well: the outputs are multiples of 1/16, so every partial
sum, in any order, fits 24 bits.  `bscale` is the first of BSCALES at which at least a quarter of every bf16-rounded quantity of the case
needs rounding and at least a quarter is representable (`shares`; found from the reference alone, asserted by the CPU test).
    case list: 10 x VT_EPI_BF16, 13 x VT_EPI_F32, 11 x VT_EPI_BF16_MULAUX over M in {1,17,64,65,127,129,191,193,200} (+120, 260 for
    the row maps), N in {4,6,18,130,192,196,198,380}, K/64 in {1,2,3,4,5,7}; ldo / ldo2 = N rounded up to 4, +4 or +8; lda = K + 8 or
    + 16, ldb = K + 8; ldr = ldaux = N rounded up to 4, + 4.  F32 cases carry bias, round_bf16, residual, rowmod (period 40, N % 4 == 0
    only: the library refuses rowmod otherwise), a row map (grp 40 inside every tile -> the rolled loop of the 192 kernel, grp 200 ->
    its one-wrap fast path), out2 and out_scale.  Nine MULAUX cases carry colsum_partial where N % 4 == 0 (exact on this data: by
    bits); two more have N % 4 == 0 without it, so that MULAUX reaches the 128x128 kernels, the skinny kernel and split-K at an
    aligned N too.
GELU FAMILY (GELU_CASES: 4 x VT_EPI_BF16_GELU, 3 x _GELU_GRAD, 4 x _DGELU, two of those with colsum_partial).  Integer A ([-1, 1]
from K = 320 on); B integers times 2^-s with s chosen so that h = acc + bias has a standard deviation of 2 to 3 and covers [-6, 6]: every
half-unit bin of [-6, 6] is hit, every unit bin in the two cases of fewer than 4000 outputs (asserted on the CPU).  h is
bf16-representable (asserted), so `out` of VT_EPI_BF16_GELU is compared by bits and only the transcendental is inexact:
|got - ref64| <= 2^-8 |ref64| + floor (times |h| for DGELU), floor = 4 x the largest distance over every bf16 input in [-8, 8] between
the fp32 restatement of vt_common.h's formulas (`gelu32`) and float64 (`gelu64`).
    measured floors (gelu_floor()): gelu 4 x 3.69e-07 = 1.477e-06, gelu' 4 x 2.38e-07 = 9.50e-07  (GELU_FLOOR_DOC; the CPU test holds
    the measurement within 10 % of these; the GPU test uses the measurement itself)
    colsum_partial under DGELU: against the float64 sum of the kernel's own bf16 outputs, bar rows * 2^-23 * sum |r|.
POISON AND CONTAINMENT.  Every operand is the leading part of a larger allocation whose remainder is NaN (rows >= M of A, >= N of B,
columns K.. of both, columns N.. of aux / residual, bias[N:], rows >= period of rowmod); every output allocation is prefilled with a
NaN sentinel (SENT32 / SENT16) and every element outside the addressed rows x N must still hold its bits after the call.
KERNEL PATHS (`nt_paths`): every case without colsum_partial on tile 1 (128x128, 2-deep ring), 16 (4-deep ring), 2 (192x192
persistent), 6 (192x192 one tile per workgroup), 0 (auto), and 7 (skinny) when M <= 64; with K/64 in {3,5,7} also on tiles 1 and 16 with
split-K forced to 2, 3, K/64 and 8 (clamped to K/64).  A colsum_partial case runs on the 192 kernel whatever the tile: it takes tiles
2, 6, 0 and, once, the forced tile 1 that the library overrides.
MUTANTS (`nt_mutants`): the reference with one tile-level error -- ktile_drop(t), row_clamp, col_clamp, last4_drop, last4_prev,
bias_shift4, residual_no_omap, rowmod_period(+1 / -1), round_after_residual, scale_skipped, out2_before_scale, corner_transposed,
splitk_drop(S, z).  A mutant is CAUGHT when it changes the expected bits of an asserted element (exact outputs) or moves an element by
32 x its bar (transcendental outputs).
    exemptions (EXEMPT, exact and capped at 5 % by the CPU test): none.
RANDOM FAMILY (RANDOM_SHAPES, RANDOM_PATHS): N(0,1) and N(0,4) bf16 operands at three ragged shapes per kernel path, forced split-K
of 2, 3 and 8 on tiles 1 and 16 included (K/64 = 3, 5, 7: uneven shares, 8 clamped).  Judged per element against the float64 product of
the bf16 values with |err| <= K 2^-23 (|A| @ |B|^T) + 2^-8 |ref| (second term: bf16 outputs only), which holds for any order of the
same sums.  Catches what integers cannot: a bf16 accumulator, a partial sum that loses bits on its way through the workspace.
TN (TN_CASES, TN_GROUP): out = A^T B by bits with the same poison and sentinels; tiles 1, 2, 7; M in {64,128,320}; (P,Q) in
{(8,8),(136,200),(192,392)}; p_lim / q_lim in {full,24,21,1}; ldo in {Q, q_lim up to 4, odd}; row_perm; lda > P, ldb > Q; one launch of
four problems in both orders.  Mutants: mtile_drop, row_extra / row_short, col_extra / col_short, perm_ignored.
DECODE (DECODE_CASES): M in {1,16,17,32,33,64} x modes 0, 1, 2 x with / without norm_w, K in {128,384,1024}, N in {16,48,512}, ldo =
cols, +4 or +8.  Every entry of row m of x is +-2^j(m), norm_w holds integers in [-4, 4], W small integers (`decode_inputs`):
bf16(x rstd w) is exactly +-w, also with rsqrt off by +-4 ulp (`decode_operand32`, asserted on the CPU), so modes 0 and 2 are compared
by bits with float64 and mode 1 (SwiGLU; bf16(acc) exact, silu not) with |got - ref64| <= 2^-8 |ref64| + 2^-8 |silu(g)| |x|.
Mutants: row_clamp, wrow_shift, kstep_drop, swiglu_swapped."""
import collections
import functools
import math

import torch

EPI_BF16, EPI_GELU, EPI_F32, EPI_DGELU, EPI_GELU_GRAD, EPI_MULAUX = 0, 1, 2, 3, 4, 5
SENT32, SENT16 = 0x7FC5A5A5, 0x7FC5            # NaN sentinels of the fp32 / bf16 outputs (0x7FC5 as int16)
NAN = float("nan")
BSCALES = (1, 3, 5, 7, 11, 13, 19, 29, 37)
U8 = 2.0 ** -8
GELU_FLOOR_DOC = {"gelu": 1.477e-06, "grad": 9.50e-07}


def ceil4(n):
    return (n + 3) // 4 * 4


def rbf(x):
    """float64 -> nearest-even bf16 -> float64.  The fp32 step in between is exact for every value of the exact families."""
    return x.to(torch.float32).to(torch.bfloat16).double()


def is_f32(x):
    return bool(((x.to(torch.float32).double() == x) | x.isnan()).all())


def is_bf16(x):
    return (rbf(x) == x) | x.isnan()


def sentinel(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16).view(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_bits(got, exp, what):
    gb, eb = bits(got), bits(exp)
    if not torch.equal(gb, eb):
        bad = (gb != eb).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {gb.numel()} elements differ, first at {i}: got {got[i].item()!r} ({gb[i].item():#x}) "
                             f"expected {exp[i].item()!r} ({eb[i].item():#x})")


def check_output(alloc, rows, ncols, exp, bar, what):
    """alloc: a whole output allocation after the call (CPU).  Its addressed part [rows, :ncols] against exp (float64) by bits -- or under `bar`,
    where a NaN fails --, every other element against the sentinel's bits."""
    inside = alloc[rows][:, :ncols]
    if bar is None:
        assert_bits(inside, exp.to(torch.float32).to(alloc.dtype), what)
    else:
        ok = (inside.double() - exp).abs() <= bar
        if not bool(ok.all()):
            i = tuple((~ok).nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int((~ok).sum())} elements outside the bar, first at {i}: got {inside[i].item()!r} expected {exp[i].item()!r} "
                                 f"bar {bar[i].item():.3e}")
    rest = bits(alloc).clone()                 # (as integers: the sentinel's NaN payload is what is compared)
    rest[rows, :ncols] = SENT32 if alloc.dtype == torch.float32 else SENT16
    assert_bits(rest.view(alloc.dtype), sentinel(alloc.shape, alloc.dtype), what + " (outside the addressed part)")


def check_nt(c, ref, got, what):
    """got: name -> the output allocations of one vt_gemm_nt call on the case (CPU), against the reference `ref`"""
    for name in ("out", "out2", "colsum"):
        if name in ref:
            r = ref[name]
            check_output(got[name], r["rows"], c.N, r["exp"], r["bar"], f"{what} {name}")
    if c.colsum and c.epi == EPI_DGELU:         # fixed-order fp32 sums of the kernel's own rounded outputs, per 192-row slab
        slabs = (c.M + 191) // 192
        o = got["out"][: c.M, : c.N].double()
        exp = torch.stack([o[t * 192:(t + 1) * 192].sum(0) for t in range(slabs)])
        bar = torch.stack([min(192, c.M - t * 192) * 2.0 ** -23 * o[t * 192:(t + 1) * 192].abs().sum(0) for t in range(slabs)])
        check_output(got["colsum"], torch.arange(slabs), c.N, exp, bar, f"{what} colsum")


def simulate_nt(c, ref):
    """the output allocations a kernel that computes `ref` (a reference or a mutant of it) would leave: for the CPU self-test of check_nt"""
    b = nt_buffers(c.name)
    got = {}
    for name in ("out", "out2", "colsum"):
        if name in ref:
            alloc = b[name][0].clone()
            v = ref[name]["exp"].to(torch.float32).to(alloc.dtype)
            keep = ~ref[name]["exp"].isnan()                      # a mutant's NaN = left unwritten
            blk = alloc[ref[name]["rows"]][:, : c.N]
            blk[keep] = v[keep]
            alloc[ref[name]["rows"], : c.N] = blk
            got[name] = alloc
    if c.colsum and c.epi == EPI_DGELU:
        slabs = (c.M + 191) // 192
        alloc = b["colsum"][0].clone()
        o = got["out"][: c.M, : c.N].float()
        alloc[:slabs] = torch.stack([o[t * 192:(t + 1) * 192].sum(0) for t in range(slabs)])
        got["colsum"] = alloc
    return got


def _gen(*key):
    seed = 0
    for c in repr(key).encode():
        seed = (seed * 131 + c) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def padded(x, rows, ld, dtype):
    """x [r, c] as the leading part of a NaN-filled [rows, ld] allocation of `dtype`"""
    buf = torch.full((rows, ld), NAN, dtype=dtype)
    buf[: x.shape[0], : x.shape[1]] = x.to(dtype)
    return buf


# ------------------------------------------------------------------------------------------------ GELU: float64 and the fp32 restatement
def gelu64(x):
    return x * 0.5 * torch.erfc(-x * math.sqrt(0.5))


def gelu_grad64(x):
    return 0.5 * torch.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) * 0.39894228040143267794


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).to(torch.float32)


def _gelu_parts32(x):
    """gelu_parts of csrc/vt_common.h in fp32 (rcp and exp2 as correctly rounded fp32 operations)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    z = x.abs() * f(0.70710678118654752440)
    t = f(1.0) / _fma32(f(0.3275911), z, f(1.0))
    p = _fma32(f(1.061405429), t, f(-1.453152027))
    p = _fma32(p, t, f(1.421413741))
    p = _fma32(p, t, f(-0.284496736))
    p = _fma32(p, t, f(0.254829592))
    e = torch.exp2((f(-0.72134752044448170368) * x * x).double()).to(torch.float32)
    hq = f(0.5) * p * t * e
    return torch.where(x >= 0, f(1.0) - hq, hq), e


def gelu32(x):
    cdf, _ = _gelu_parts32(x)
    return x * cdf


def gelu_grad32(x):
    cdf, e = _gelu_parts32(x)
    return _fma32(x * torch.tensor(0.39894228040143267794, dtype=torch.float32), e, cdf)


@functools.lru_cache(None)
def gelu_floor():
    """{'gelu', 'grad'}: 4 x max |fp32 restatement - float64| over every bf16 value in [-8, 8]"""
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    x = allb[allb.abs() <= 8.0]
    return {"gelu": 4.0 * float((gelu32(x).double() - gelu64(x.double())).abs().max()),
            "grad": 4.0 * float((gelu_grad32(x).double() - gelu_grad64(x.double())).abs().max())}


# ------------------------------------------------------------------------------------------------ NT cases
_NT_FIELDS = dict(name=None, epi=EPI_BF16, M=1, N=4, K=64, bias=True, round_bf16=False, residual=False, rowmod=0, omap=None, out2=False,
                  out_scale=0.0, lda_pad=8, ldo_pad=0, ldo2_pad=0, colsum=False)
NTCase = collections.namedtuple("NTCase", list(_NT_FIELDS), defaults=list(_NT_FIELDS.values()))

_MS = (1, 17, 64, 65, 127, 129, 191, 193, 200)
_NS = (4, 6, 18, 130, 192, 196, 198, 380)
_KS = (64, 128, 192, 256, 320, 448)
_PADS = (0, 4, 8)


def _nt_cases():
    cs = []
    for i, M in enumerate(_MS):
        N, K = _NS[i % 8], _KS[i % 6]
        cs.append(NTCase(f"bf16_{M}x{N}x{K}", EPI_BF16, M, N, K, bias=i % 3 != 2, lda_pad=8 + 8 * (i % 2), ldo_pad=_PADS[i % 3]))
    for i, M in enumerate(_MS):
        N, K = _NS[(i + 5) % 8], _KS[(i + 4) % 6]
        cs.append(NTCase(f"mulaux_{M}x{N}x{K}", EPI_MULAUX, M, N, K, bias=i % 2 == 0, lda_pad=8 + 8 * (i % 2), ldo_pad=_PADS[(i + 1) % 3],
                         colsum=N % 4 == 0))
    cs += [NTCase("mulaux_64x196x192", EPI_MULAUX, 64, 196, 192, ldo_pad=4),              # N % 4 == 0 without colsum_partial: 128x128, skinny, split-K
           NTCase("mulaux_193x192x320", EPI_MULAUX, 193, 192, 320, bias=False, lda_pad=16, ldo_pad=8)]
    full = dict(round_bf16=True, residual=True, out2=True)
    cs += [
        NTCase("f32_plain_64x4x64", EPI_F32, 64, 4, 64, bias=False),
        NTCase("f32_map40_120x196x192", EPI_F32, 120, 196, 192, rowmod=40, omap=(40, 48, 3), out_scale=0.5, ldo_pad=4, **full),
        NTCase("f32_map40_200x380x320", EPI_F32, 200, 380, 320, rowmod=40, omap=(40, 44, 0), out_scale=0.25, ldo2_pad=4, **full),
        NTCase("f32_map200_260x196x64", EPI_F32, 260, 196, 64, rowmod=40, omap=(200, 210, 1), out_scale=2.0, ldo_pad=8, ldo2_pad=8, **full),
        NTCase("f32_map40_129x130x64", EPI_F32, 129, 130, 64, omap=(40, 41, 2), out_scale=0.5, **full),
        NTCase("f32_map40_193x198x192", EPI_F32, 193, 198, 192, omap=(40, 56, 0), out_scale=4.0, ldo_pad=4, ldo2_pad=8, **full),
        NTCase("f32_1x6x448", EPI_F32, 1, 6, 448, out_scale=0.5, lda_pad=16, **full),
        NTCase("f32_17x18x128", EPI_F32, 17, 18, 128, out_scale=0.125, ldo_pad=8, ldo2_pad=4, **full),
        NTCase("f32_65x192x256", EPI_F32, 65, 192, 256, rowmod=40, out_scale=0.5, ldo2_pad=4, **full),
        NTCase("f32_127x4x320", EPI_F32, 127, 4, 320, rowmod=40, residual=True, out_scale=2.0),
        NTCase("f32_191x380x128", EPI_F32, 191, 380, 128, round_bf16=True, residual=True, rowmod=40, ldo_pad=4),
        NTCase("f32_64x130x448", EPI_F32, 64, 130, 448, residual=True, out2=True, omap=(40, 64, 5), ldo_pad=8),
        NTCase("f32_200x192x64", EPI_F32, 200, 192, 64, bias=False, round_bf16=True, out_scale=0.5, ldo_pad=8),
    ]
    cs.append(NTCase("bf16_200x192x128", EPI_BF16, 200, 192, 128, ldo_pad=8))          # N % 8 == 0 and ldo % 8 == 0: the 16-byte read-back
    return cs


NT_CASES = _nt_cases()
GELU_CASES = [
    NTCase("gelu_129x196x64", EPI_GELU, 129, 196, 64, ldo_pad=4),
    NTCase("gelu_200x130x192", EPI_GELU, 200, 130, 192, ldo2_pad=4),
    NTCase("gelu_17x192x256", EPI_GELU, 17, 192, 256, bias=False, ldo_pad=8, ldo2_pad=8),
    NTCase("gelu_193x192x128", EPI_GELU, 193, 192, 128, ldo2_pad=4),                   # N % 8 == 0, ldo2 % 8 != 0: back to the 8-byte read-back
    NTCase("gelugrad_193x380x64", EPI_GELU_GRAD, 193, 380, 64, ldo2_pad=4),
    NTCase("gelugrad_65x198x320", EPI_GELU_GRAD, 65, 198, 320, ldo_pad=4),
    NTCase("gelugrad_64x192x128", EPI_GELU_GRAD, 64, 192, 128, ldo_pad=8, ldo2_pad=8),
    NTCase("dgelu_200x196x192", EPI_DGELU, 200, 196, 192, colsum=True, ldo_pad=4),
    NTCase("dgelu_127x18x64", EPI_DGELU, 127, 18, 64, bias=False),
    NTCase("dgelu_129x130x192", EPI_DGELU, 129, 130, 192),                             # no colsum_partial: the 128x128 kernels and split-K
    NTCase("dgelu_193x192x448", EPI_DGELU, 193, 192, 448, bias=False, colsum=True, ldo_pad=8),
]
NT_BY_NAME = {c.name: c for c in NT_CASES + GELU_CASES}
GELU_EPIS = (EPI_GELU, EPI_GELU_GRAD, EPI_DGELU)


def nt_paths(c):
    """(tile, splitk) of every kernel path the case runs on"""
    if c.colsum:                                   # the 192 kernel whatever the tile: the forced 128 tile once, for the override
        return [(t, 1) for t in (2, 6, 0, 1)]
    paths = [(t, 1) for t in (1, 16, 2, 6, 0)]
    if c.M <= 64:
        paths.append((7, 1))
    nt = c.K // 64
    if nt in (3, 5, 7):
        paths += [(t, s) for t in (1, 16) for s in sorted({2, 3, nt, 8})]
    return paths


def nt_splits(c):
    nt = c.K // 64
    return sorted({min(s, nt) for _, s in nt_paths(c) if s > 1})


def out_rows_of(c):
    """output row of every m (the row map), and the rows of the output allocation's addressed view"""
    m = torch.arange(c.M)
    if c.omap is None:
        return m, c.M
    grp, stride, off = c.omap
    rows = (m // grp) * stride + off + m % grp
    return rows, int(rows.max()) + 1 + 2           # out_rows > M: two rows behind the last mapped one belong to the view


def _nt_raw(c, bscale):
    g = _gen("nt", c.name)
    M, N, K = c.M, c.N, c.K
    d = {"A": _ints(g, -2, 2, (M, K))}
    if c.epi in GELU_EPIS:
        a = 2 if K < 320 else 1                                               # var(A) = 2 or 2/3, var(B) = 4 before the scale
        d["A"] = _ints(g, -a, a, (M, K))
        s = 3
        while math.sqrt(K * (2.0 if a == 2 else 2.0 / 3.0) * 4.0) / 2 ** s > 3.5:
            s += 1
        d["B"] = _ints(g, -3, 3, (N, K)) / 2 ** s
        d["bias"] = _ints(g, -8, 8, (N,)) / 8
        d["aux"] = rbf(_ints(g, -1024, 1024, (M, N)) / 128)                 # DGELU: the saved pre-activation, [-8, 8]
    else:
        d["B"] = _ints(g, -3, 3, (N, K)) * bscale
        d["bias"] = _ints(g, -40, 40, (N,)) / 4
        d["aux"] = _ints(g, -16, 16, (M, N)) / 4
    _, orows = out_rows_of(c)
    d["residual"] = _ints(g, -400, 400, (orows, N)) / 4
    d["rowmod"] = _ints(g, -400, 400, (max(c.rowmod, 1) + 1, N)) / 4        # one row more than the period: the period + 1 mutant reads it
    return d


def shares(ref):
    """per bf16-rounded quantity of the case: (share that needs rounding, share that is representable)"""
    out = []
    for q in ref["pre_round"]:
        ok = is_bf16(q).double().mean().item()
        out.append((1.0 - ok, ok))
    return out


@functools.lru_cache(None)
def nt_inputs(name):
    """float64 values of the case's operands ('A', 'B', 'bias', 'aux', 'residual', 'rowmod') and its 'bscale'"""
    c = NT_BY_NAME[name]
    if c.epi in GELU_EPIS:
        d = _nt_raw(c, 1)
        d["bscale"] = 1
        return d
    for bscale in BSCALES:
        d = _nt_raw(c, bscale)
        d["bscale"] = bscale
        ref = nt_reference(c, d)
        if all(a >= 0.25 and b >= 0.25 for a, b in shares(ref)):
            return d
    raise AssertionError(f"{name}: no bscale of {BSCALES} meets the rounding shares")


def nt_buffers(name):
    """the allocations a kernel call gets: name -> (allocation, rows, cols) whose leading [rows, cols] (or [:cols] for bias) is the operand;
    outputs hold the sentinel.  The views' strides are the allocations' widths."""
    c = NT_BY_NAME[name]
    d = nt_inputs(name)
    M, N, K = c.M, c.N, c.K
    n4 = ceil4(N)
    _, orows = out_rows_of(c)
    odt = torch.float32 if c.epi == EPI_F32 else torch.bfloat16
    b = {"A": (padded(d["A"], M + 1, K + c.lda_pad, torch.bfloat16), M, K),
         "B": (padded(d["B"], N + 1, K + 8, torch.bfloat16), N, K),
         "out": (sentinel((orows + 1, n4 + c.ldo_pad), odt), orows, N)}
    if c.bias:
        b["bias"] = (padded(d["bias"].view(1, -1), 1, n4 + 8, torch.float32).view(-1), 1, N)
    if c.epi in (EPI_DGELU, EPI_MULAUX):
        b["aux"] = (padded(d["aux"], M + 1, n4 + 4, torch.bfloat16), M, N)
    if c.residual:
        b["residual"] = (padded(d["residual"], orows + 1, n4 + 4, torch.float32), orows, N)
    if c.rowmod:
        b["rowmod"] = (padded(d["rowmod"][: c.rowmod], c.rowmod + 2, N, torch.float32), c.rowmod, N)
    if c.out2 or c.epi in (EPI_GELU, EPI_GELU_GRAD):
        b["out2"] = (sentinel((orows + 1, n4 + c.ldo2_pad), torch.bfloat16), orows, N)
    if c.colsum:
        b["colsum"] = (sentinel(((M + 191) // 192 + 1, N), torch.float32), (M + 191) // 192, N)
    return b


def _drop_tiles(A, tiles):
    A = A.clone()
    for t in tiles:
        A[:, t * 64:(t + 1) * 64] = 0
    return A


def split_tiles(nt, S, z):
    return range(z * nt // S, (z + 1) * nt // S)


def nt_mutants(c):
    nt = c.K // 64
    ms = [("ktile_drop", t) for t in range(nt)]
    if c.M > 1:
        ms.append(("row_clamp", None))
    ms += [("col_clamp", None), ("last4_drop", None)]
    if min(c.M - (c.M - 1) // 128 * 128, c.N - (c.N - 1) // 128 * 128) >= 2:      # the ragged corner tile holds a square of 2 x 2 at least
        ms.append(("corner_transposed", None))
    if c.N > 4:
        ms.append(("last4_prev", None))
    if c.bias and c.N > 4:
        ms.append(("bias_shift4", None))
    if c.epi == EPI_F32:
        if c.residual and c.omap:
            ms.append(("residual_no_omap", None))
        if c.rowmod:
            ms += [("rowmod_period", 1), ("rowmod_period", -1)]
        if c.round_bf16 and c.residual:
            ms.append(("round_after_residual", None))
        if c.out_scale:
            ms.append(("scale_skipped", None))
        if c.out_scale and c.out2:
            ms.append(("out2_before_scale", None))
    ms += [("splitk_drop", (S, z)) for S in nt_splits(c) for z in range(S)]
    return ms


def mutant_id(m):
    return m[0] if m[1] is None else f"{m[0]}{m[1]}".replace(" ", "")


EXEMPT = {}          # (case name, mutant id) -> reason


def nt_reference(c, d=None, mut=None):
    """expected outputs of the case (or of the reference with the one error `mut`): name -> dict(rows, exp [M, N] float64, dtype, bar or None);
    'colsum' likewise with rows = the slabs; 'pre_round': the float64 quantities that a bf16 rounding is applied to; 'h' for the GELU family"""
    d = nt_inputs(c.name) if d is None else d
    kind, arg = mut if mut else (None, None)
    M, N, K = c.M, c.N, c.K
    A, B = d["A"], d["B"]
    if kind == "ktile_drop":
        A = _drop_tiles(A, [arg])
    if kind == "splitk_drop":
        A = _drop_tiles(A, split_tiles(K // 64, *arg))
    acc = A @ B.t()
    assert float(acc.abs().max()) < 2 ** 21
    if kind == "row_clamp":
        acc[M - 1] = acc[M - 2]
    if kind == "col_clamp":
        acc[:, N - 1] = acc[:, N - 2]
    g0 = (N - 1) // 4 * 4
    if kind == "last4_drop":
        acc[:, g0:] = NAN
    if kind == "last4_prev":
        acc[:, g0:] = acc[:, g0 - 4:g0 - 4 + N - g0]
    if kind == "corner_transposed":
        m0, n0 = (M - 1) // 128 * 128, (N - 1) // 128 * 128
        s = min(M - m0, N - n0)
        acc[m0:m0 + s, n0:n0 + s] = acc[m0:m0 + s, n0:n0 + s].t().clone()
    bias = d["bias"] if c.bias else torch.zeros(N, dtype=torch.float64)
    if kind == "bias_shift4":
        bias = torch.roll(bias, -4)
    v = acc + bias
    rows, _ = out_rows_of(c)
    midx = torch.arange(M)
    res = {"pre_round": []}

    def put(name, x, dtype, bar=None, r=rows):
        if bar is None:
            assert is_f32(x), f"{c.name}: {name} is not exact in fp32"
            if dtype == torch.bfloat16:
                assert bool(is_bf16(x).all())
        res[name] = dict(rows=r, exp=x, dtype=dtype, bar=bar)

    if c.epi == EPI_F32:
        if c.round_bf16 and kind != "round_after_residual":
            res["pre_round"].append(v)
            v = rbf(v)
        if c.residual:
            v = v + d["residual"][midx if kind == "residual_no_omap" else rows]
        if c.round_bf16 and kind == "round_after_residual":
            v = rbf(v)
        if c.rowmod:
            period = c.rowmod + (arg if kind == "rowmod_period" else 0)
            v = v + d["rowmod"][midx % period]
        out = v * c.out_scale if c.out_scale and kind != "scale_skipped" else v
        put("out", out, torch.float32)
        if c.out2:
            pre2 = v if kind == "out2_before_scale" else out
            res["pre_round"].append(pre2)
            put("out2", rbf(pre2), torch.bfloat16)
        return res
    if c.epi in (EPI_BF16, EPI_MULAUX):
        res["pre_round"].append(v)
        h = rbf(v)
        if c.epi == EPI_BF16:
            put("out", h, torch.bfloat16)
            return res
        res["pre_round"].append(h * d["aux"])
        out = rbf(h * d["aux"])
        put("out", out, torch.bfloat16)
        if c.colsum:
            slabs = (M + 191) // 192
            cs = torch.stack([out[t * 192:(t + 1) * 192].nan_to_num(0.0).sum(0) for t in range(slabs)])
            if mut is None:                    # multiples of 1/16 below 2^20 in sum: every partial sum is exact in fp32, in any order
                assert bool((out * 16 == (out * 16).round()).all())
                assert all(float(out[t * 192:(t + 1) * 192].abs().sum(0).max()) < 2 ** 20 for t in range(slabs))
            put("colsum", cs, torch.float32, r=torch.arange(slabs))
        return res
    # GELU family: h = bf16(acc + bias) is exact, the transcendental is not
    if mut is None:
        assert bool(is_bf16(v).all()), f"{c.name}: acc + bias is not bf16-representable"
    h = rbf(v)
    res["h"] = h
    fl = gelu_floor()
    if c.epi == EPI_GELU:
        put("out", h, torch.bfloat16)
        g = gelu64(h)
        put("out2", g, torch.bfloat16, bar=U8 * g.abs() + fl["gelu"])
    elif c.epi == EPI_GELU_GRAD:
        g, dg = gelu64(h), gelu_grad64(h)
        put("out", dg, torch.bfloat16, bar=U8 * dg.abs() + fl["grad"])
        put("out2", g, torch.bfloat16, bar=U8 * g.abs() + fl["gelu"])
    else:
        o = h * gelu_grad64(d["aux"])
        put("out", o, torch.bfloat16, bar=U8 * o.abs() + fl["grad"] * h.abs())
    return res


def caught(ref, mutref):
    """does the mutant change an asserted element of the reference: other bits (exact) or 32 bars away (transcendental)"""
    for name, r in ref.items():
        if name in ("pre_round", "h"):
            continue
        a, b = r["exp"], mutref[name]["exp"]
        if r["bar"] is None:
            ta = a.to(r["dtype"]) if r["dtype"] == torch.float32 else a.to(torch.float32).to(torch.bfloat16)
            tb = b.to(r["dtype"]) if r["dtype"] == torch.float32 else b.to(torch.float32).to(torch.bfloat16)
            if not torch.equal(bits(ta), bits(tb)):
                return True
        else:
            diff = (a - b).abs()
            if bool((diff.isnan() | ((diff > 0) & (diff >= 32.0 * r["bar"]))).any()):
                return True
    return False


# ------------------------------------------------------------------------------------------------ random family
RANDOM_SHAPES = {"tiles": [(129, 130, 192), (193, 198, 320), (200, 380, 448)], "skinny": [(17, 198, 192), (64, 130, 320), (1, 380, 448)]}
RANDOM_STDS = (1.0, 2.0)
# (tile, splitk, family of shapes): every kernel path, the forced splits of tiles 1 and 16 included
RANDOM_PATHS = [(t, 1, "tiles") for t in (1, 16, 2, 6, 0)] + [(7, 1, "skinny"), (0, 1, "skinny")] + [(t, s, "tiles") for t in (1, 16) for s in (2, 3, 8)]


@functools.lru_cache(None)
def random_case(M, N, K, std):
    """A, B bf16 ~ N(0, std^2); ref = their float64 product; bound32 / bound16 = the per-element bars of an fp32 / a bf16 output"""
    g = _gen("random", M, N, K, std)
    A = (torch.randn(M, K, generator=g) * std).to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)
    ref = A.double() @ B.double().t()
    b32 = K * 2.0 ** -23 * (A.double().abs() @ B.double().abs().t())
    return dict(A=A, B=B, ref=ref, bound32=b32, bound16=b32 + U8 * ref.abs())


# ------------------------------------------------------------------------------------------------ TN
_TN_FIELDS = dict(name=None, M=64, P=8, Q=8, p_lim=None, q_lim=None, ldo="Q", perm=False)
TNCase = collections.namedtuple("TNCase", list(_TN_FIELDS), defaults=list(_TN_FIELDS.values()))
TN_TILES = (1, 2, 7)


def _tn_cases():
    cs = []
    lims = (None, 24, 21, 1)
    ldos = ("Q", "lim4", "odd")
    i = 0
    for M in (64, 128, 320):
        for P, Q in ((8, 8), (136, 200), (192, 392)):
            for k in range(2):                       # two limit / ldo / perm settings per shape: every value of each axis at every (P, Q)
                pl, ql = lims[(i + k) % 4], lims[(i + 2 * k + 1) % 4]
                pl = None if pl is not None and pl > P else pl
                ql = None if ql is not None and ql > Q else ql
                cs.append(TNCase(f"tn_{M}_{P}x{Q}_p{pl or 'full'}_q{ql or 'full'}_{ldos[(i + k) % 3]}{'_perm' if (i + k) % 2 else ''}",
                                 M, P, Q, pl, ql, ldos[(i + k) % 3], bool((i + k) % 2)))
            i += 1
    return cs


# one launch of four problems of different tile counts (8, 4, 2, 1 tiles of 128x128), largest first; the GPU test also reverses it
TN_GROUP = [TNCase("tn_group_320_192x392", 320, 192, 392, None, None, "odd", True), TNCase("tn_group_128_136x200", 128, 136, 200, None, None, "Q", False),
            TNCase("tn_group_64_192x392_q21", 64, 192, 392, None, 21, "lim4", True), TNCase("tn_group_128_8x8", 128, 8, 8, None, 1, "odd", False)]
TN_CASES = _tn_cases() + TN_GROUP
TN_BY_NAME = {c.name: c for c in TN_CASES}


def tn_dims(c):
    pl, ql = c.p_lim or c.P, c.q_lim or c.Q
    ldo = {"Q": c.Q, "lim4": ceil4(ql), "odd": ql + 1 - ql % 2 + 2}[c.ldo]
    return pl, ql, ldo, pl + (3 if c.perm else 0)


@functools.lru_cache(None)
def tn_inputs(name):
    c = TN_BY_NAME[name]
    g = _gen("tn", name)
    pl, ql, ldo, orows = tn_dims(c)
    d = {"A": _ints(g, -2, 2, (c.M, c.P)), "B": _ints(g, -3, 3, (c.M, c.Q))}
    d["perm"] = torch.randperm(orows, generator=g)[:pl].to(torch.int32) if c.perm else None
    return d


def tn_buffers(name):
    c = TN_BY_NAME[name]
    d = tn_inputs(name)
    pl, ql, ldo, orows = tn_dims(c)
    return {"A": (padded(d["A"], c.M + 1, c.P + 8, torch.bfloat16), c.M, c.P), "B": (padded(d["B"], c.M + 1, c.Q + 16, torch.bfloat16), c.M, c.Q),
            "out": (sentinel((orows + 1, ldo), torch.float32), orows, ql)}


def tn_mutants(c):
    pl, ql, _, _ = tn_dims(c)
    ms = [("mtile_drop", t) for t in range(c.M // 64)]
    ms += [("row_short", None), ("col_short", None)]
    if pl < c.P:
        ms.append(("row_extra", None))
    if ql < c.Q and tn_dims(c)[2] > ql:
        ms.append(("col_extra", None))
    if c.perm:
        ms.append(("perm_ignored", None))
    return ms


def tn_reference(c, mut=None):
    """the expected output ALLOCATION (sentinel where nothing is stored), fp32"""
    d = tn_inputs(c.name)
    kind, arg = mut if mut else (None, None)
    pl, ql, ldo, orows = tn_dims(c)
    A = d["A"]
    if kind == "mtile_drop":
        A = A.clone()
        A[arg * 64:(arg + 1) * 64] = 0
    full = A.t() @ d["B"]
    assert is_f32(full) and float(full.abs().max()) < 2 ** 21
    r1 = pl + (kind == "row_extra") - (kind == "row_short")
    q1 = ql + (kind == "col_extra") - (kind == "col_short")
    exp = sentinel((orows + 1, ldo), torch.float32)
    rows = d["perm"].long() if c.perm and kind != "perm_ignored" else torch.arange(pl)
    if kind == "row_extra":
        rows = torch.cat([rows, torch.tensor([orows])])          # the row behind the last: the first row of the sentinel tail
    exp[rows[:r1], :q1] = full[:r1, :q1].float()
    return exp


# ------------------------------------------------------------------------------------------------ decode: RMSNorm + Linear [+ SwiGLU]
DecodeCase = collections.namedtuple("DecodeCase", "name M K N norm mode ldo_pad")
DECODE_EPS = 1e-5


def _decode_cases():
    cs = []
    Ms, Ks, Ns = (1, 16, 17, 32, 33, 64), (128, 384, 1024), (16, 48, 512)
    i = 0
    for mi, M in enumerate(Ms):
        for mode in (0, 1, 2):
            for norm in (True, False):
                K, N = Ks[(mi + mode + i) % 3], Ns[(mi + 2 * mode + norm) % 3]
                cs.append(DecodeCase(f"decode_m{mode}_{'norm' if norm else 'plain'}_{M}x{N}x{K}", M, K, N, norm, mode, (0, 4, 8)[(i + mi) % 3]))
                i += 1
    return cs


DECODE_CASES = _decode_cases()
DECODE_BY_NAME = {c.name: c for c in DECODE_CASES}


@functools.lru_cache(None)
def decode_inputs(name):
    """x: every entry of row m is +-2^j(m) (fp32; mean(x^2) = 4^j) -- or, without the norm, the bf16 integers the norm would have produced;
    norm_w integers in [-4, 4]; W small integers (mode 1: sparse, times 1/4); 'xn' = the exact normalised operand"""
    c = DECODE_BY_NAME[name]
    g = _gen("decode", name)
    sign = _ints(g, 0, 1, (c.M, c.K)) * 2 - 1
    j = _ints(g, -2, 5, (c.M, 1))
    w = _ints(g, -4, 4, (c.K,))
    xn = sign * w                                                 # bf16(x * rstd * w) exactly
    W = _ints(g, -2, 2, (c.N, c.K))
    if c.mode == 1:           # sparse quarters: the gate covers [-8, 8] or so and bf16(acc) stays exact (|acc| < 64 in multiples of 1/4)
        W = _ints(g, -1, 1, (c.N, c.K)) * (_ints(g, 0, 7, (c.N, c.K)) == 0) / 4
    d = dict(W=W, xn=xn)
    if c.norm:
        d["x"], d["norm_w"] = sign * 2.0 ** j, w
    else:
        d["x"] = xn
    return d


def decode_operand32(x, w, ulps):
    """bf16(x * rstd * w) as the kernel forms it in fp32, with rsqrt(mean + eps) moved by `ulps` fp32 ulps"""
    x32, w32 = x.to(torch.float32), w.to(torch.float32)
    mean = (x32 * x32).sum(1, keepdim=True) * torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    r = (1.0 / torch.sqrt((mean + torch.tensor(DECODE_EPS, dtype=torch.float32)).double())).to(torch.float32)
    r = (r.view(torch.int32) + ulps).view(torch.float32)
    return (x32 * r * w32).to(torch.bfloat16).double()


def decode_buffers(name):
    c = DECODE_BY_NAME[name]
    d = decode_inputs(name)
    cols = c.N // 2 if c.mode == 1 else c.N
    b = {"x": (padded(d["x"], c.M + 1, c.K, torch.float32 if c.norm else torch.bfloat16), c.M, c.K),
         "W": (padded(d["W"], c.N + 1, c.K, torch.bfloat16), c.N, c.K),
         "out": (sentinel((c.M + 1, cols + c.ldo_pad), torch.float32 if c.mode == 2 else torch.bfloat16), c.M, cols)}
    if c.norm:
        b["norm_w"] = (padded(d["norm_w"].view(1, -1), 1, c.K + 8, torch.float32).view(-1), 1, c.K)
    return b


def decode_reference(c, mut=None):
    """exp [M, cols] float64 and bar (None: by bits).  Mutants: 'row_clamp', 'wrow_shift' (weight row n + 1), 'kstep_drop' (the last 32
    columns of K left out), 'swiglu_swapped' (mode 1: value and gate slabs exchanged)"""
    d = decode_inputs(c.name)
    xn, W = d["xn"], d["W"]
    if mut == "kstep_drop":
        xn = xn.clone()
        xn[:, -32:] = 0
    if mut == "wrow_shift":
        W = torch.roll(W, -1, 0)
    acc = xn @ W.t()
    if mut == "row_clamp":
        acc[c.M - 1] = acc[c.M - 2]
    assert is_f32(acc)
    if c.mode != 1:
        return rbf(acc), None
    a = acc.view(c.M, c.N // 16, 2, 8)
    val, gate = (a[:, :, 0], a[:, :, 1]) if mut != "swiglu_swapped" else (a[:, :, 1], a[:, :, 0])
    val, gate = val.reshape(c.M, -1), gate.reshape(c.M, -1)
    if mut is None:
        assert bool(is_bf16(val).all()) and bool(is_bf16(gate).all()), f"{c.name}: bf16(acc) is not exact"
    s = gate / (1.0 + torch.exp(-gate))
    exp = s * val
    return exp, U8 * exp.abs() + U8 * s.abs() * val.abs()


def decode_mutants(c):
    ms = ["wrow_shift", "kstep_drop"]
    if c.M > 1:
        ms.append("row_clamp")
    if c.mode == 1:
        ms.append("swiglu_swapped")
    return ms
