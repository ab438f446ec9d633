"""Edge cases, float64 references and reference mutants of the attention kernels (vt_attention_fwd / _bwd, their _rows and causal
variants, vt_decode_attention / _step).  Plain torch on the CPU: importing this module needs no GPU and no built library.

A case is built from bf16 values; the reference evaluates the same formula as the kernel in float64 on exactly those values.  A MUTANT is
the reference with one element miscounted (a key dropped, a padded key counted, a clamped key counted twice, a query of the kept suffix
off by one, ...): the errors a tile / tail / mask bug makes.  For every case and every asserted quantity

    dev_q(m)  = max over rows of |mutant m - reference| in quantity q   (lse2: absolute; o, dQ, dK, dV: L2 norm of the row)
    noise_q   = the same distance for an evaluation that rounds where the kernel rounds (scores, exponentials and sums in fp32; P and dS
                to bf16 before their products; o, dQ, dK, dV to bf16; delta from the rounded o), floored at one unit of the quantity's
                number format (2^-23 of the largest |lse2|, 2^-9 of the largest row norm) so that a lucky estimate cannot reach zero
    m is DETECTABLE in q  when  dev_q(m) >= 32 * noise_q
    tol_q     = 1/4 of the smallest dev_q(m) over the mutants detectable in q, and never above REL_CAP = 0.5 for the row-relative
                quantities (a bar of 1 would pass an all-zero row).  Where no mutant is detectable in q, or that bar would be below
                8 * noise_q, q is NOT ASSERTED in that case; NOT_ASSERTED names every (family, quantity) this happens to, with the reason.

Both numbers come from the reference alone, never from a kernel.  tests/test_attention_cases_cpu.py asserts, per case, that every mutant is
detectable in an asserted quantity unless (family, mutant) is named in EXEMPT_MUTANTS, that both tables are exact (nothing outside them is
left out, every entry is in use), that every row-relative bar is at most REL_CAP, and, per shape, that every mutant -- the exempt ones
included -- is seen by at least one family.  tests/test_attention_edges_gpu.py asserts the kernels against the same tolerances.

Families (each with B >= 2 and H >= 2 except the one L = 1536 shape, so that a wrong batch or head stride reads a neighbour):
  flat     q = 0: every score is 0, lse2 = log2(visible keys), o = the exact mean of small nonzero integers in V
  planted  special keys 16 e_a at the boundary indices, query i = 16 e_a of special i mod n: o_i = v[target(i)], an integer, to 1e-9;
           poison (a special key of twice the magnitude with v = 1000) in the first rows of the following sequence -- on coordinates the
           following sequence's own queries never use -- and in rows behind the tensor, which is a view of a larger allocation
  ramp     one coordinate of k grows with the key index by more than 8 log2 units per 64-key tile (rising, falling, or a wave whose
           32-key runs alternate ramp and flat), so the lazy rescale of fwd_tile fires on a non-empty accumulator in every tile; every
           eighth query is a probe with a zero ramp coordinate, for which every key weighs about 1/L (a dropped early key still shows)
  random   N(0, 1) and N(0, 2^2) operands, judged per row

Tolerance table (python -m tests.attention_cases prints it; `ratio` = tol / noise, `-` = quantity not produced).  One line per kernel,
family and head_dim: the range over that group's shapes of tol and the smallest ratio, over the cases that assert the quantity.

kernel  family     hd         lse2 tol (min ratio)            o tol (min ratio)           dq tol (min ratio)           dk tol (min ratio)           dv tol (min ratio)
full    flat       64  2.35e-04..2.50e-01 (   186)  1.90e-02..1.25e-01 (    10)  3.65e-02..2.50e-01 (     9)                            -  1.77e-02..2.50e-01 (     9)
full    planted    64  2.50e-01..2.50e-01 ( 45426)  2.47e-01..2.65e-01 (   126)                            -                            -  3.11e-02..2.50e-01 (    16)
full    ramp_rise  64  4.15e-04..2.50e-01 (    11)  2.56e-02..1.26e-01 (     9)  8.42e-02..1.21e-01 (     9)  6.16e-02..1.48e-01 (     8)  1.82e-02..2.50e-01 (     8)
full    ramp_fall  64  1.08e-03..2.48e-01 (   129)  2.56e-02..1.24e-01 (     8)  6.40e-02..1.18e-01 (     8)  4.23e-02..1.58e-01 (     8)  1.97e-02..2.50e-01 (     8)
full    ramp_wave  64  1.09e-03..2.50e-01 (    88)  2.65e-02..1.33e-01 (     8)  5.00e-01..5.00e-01 (    10)  6.30e-02..1.49e-01 (     8)  1.88e-02..2.50e-01 (     8)
full    random1    64  8.87e-04..2.50e-01 (   744)  6.79e-02..1.74e-01 (    20)  9.85e-02..1.84e-01 (    18)  8.92e-02..1.79e-01 (    24)  8.07e-02..2.50e-01 (    20)
full    random2    64  4.28e-05..2.50e-01 (    12)  6.53e-02..2.24e-01 (    24)                            -  1.77e-01..2.48e-01 (     8)  1.76e-01..2.50e-01 (    41)
rows    flat       64  1.08e-03..2.79e-03 (  1083)  1.57e-02..2.45e-02 (     8)  2.00e-02..4.27e-02 (     8)                            -  1.77e-02..2.50e-01 (     8)
rows    planted    64  2.50e-01..9.62e+00 ( 45426)  2.50e-01..2.58e-01 (   128)                            -                            -  5.02e-02..2.50e-01 (    26)
rows    ramp_rise  64  3.80e-05..2.79e-03 (     8)  2.29e-02..2.61e-01 (     8)                            -  4.88e-02..8.75e-02 (     9)  1.61e-02..6.45e-02 (     8)
rows    ramp_fall  64  3.92e-05..2.81e-03 (     9)  2.46e-02..2.60e-01 (     8)                            -  6.91e-02..8.34e-02 (    10)  2.00e-02..2.50e-01 (     8)
rows    ramp_wave  64  2.78e-04..2.82e-03 (    40)  2.42e-02..2.57e-01 (     8)                            -  5.72e-02..8.99e-02 (     8)  2.02e-02..2.50e-01 (     8)
rows    random1    64  8.07e-04..2.46e-03 (   697)  2.12e-02..7.34e-02 (     9)  2.71e-02..9.02e-02 (     8)  1.01e-01..2.50e-01 (    17)  9.86e-02..2.50e-01 (    26)
rows    random2    64  1.61e-05..8.20e-04 (     9)  1.88e-02..1.32e-01 (     9)  1.16e-01..2.50e-01 (    11)  2.50e-01..5.00e-01 (    10)  3.67e-02..2.50e-01 (    10)
full    flat       32  1.08e-03..2.50e-01 (  1083)  1.99e-02..1.25e-01 (    10)  4.08e-02..6.64e-02 (     9)                            -  1.56e-02..2.50e-01 (     8)
full    planted    32  2.50e-01..2.50e-01 ( 32121)  2.53e-01..2.72e-01 (   129)                            -                            -  2.96e-02..2.50e-01 (    15)
full    ramp_rise  32  1.09e-03..2.50e-01 (   130)  2.88e-02..1.28e-01 (     8)  9.91e-02..1.26e-01 (     9)  7.16e-02..1.27e-01 (     8)  1.92e-02..2.50e-01 (     8)
full    ramp_fall  32  1.10e-03..2.50e-01 (   132)  2.78e-02..1.26e-01 (     8)  7.01e-02..2.50e-01 (    10)  8.61e-02..1.54e-01 (     8)  1.75e-02..2.50e-01 (     9)
full    ramp_wave  32  1.09e-03..2.43e-01 (    88)  2.53e-02..1.23e-01 (     8)  5.00e-01..5.00e-01 (     9)  7.38e-02..2.50e-01 (     8)  1.93e-02..2.50e-01 (     8)
full    random1    32  9.04e-04..2.50e-01 (   753)  6.61e-02..1.51e-01 (    20)  7.83e-02..1.68e-01 (     9)  9.00e-02..1.81e-01 (    21)  9.55e-02..2.50e-01 (    23)
full    random2    32  9.19e-05..2.50e-01 (    23)  5.36e-02..2.48e-01 (    16)                            -  2.12e-01..2.46e-01 (     8)  1.18e-01..2.50e-01 (    22)
rows    flat       32  1.08e-03..2.79e-03 (  1083)  1.60e-02..2.23e-02 (     8)  1.93e-02..4.11e-02 (     8)                            -  1.69e-02..2.50e-01 (     9)
rows    planted    32  2.50e-01..1.42e+01 ( 32121)  2.52e-01..2.63e-01 (   129)                            -                            -  5.14e-02..2.50e-01 (    26)
rows    ramp_rise  32  4.06e-05..2.86e-03 (     9)  2.69e-02..2.61e-01 (     8)                            -  8.53e-02..1.07e-01 (     8)  1.61e-02..2.50e-01 (     8)
rows    ramp_fall  32  3.81e-05..2.85e-03 (     9)  2.55e-02..2.61e-01 (     8)                            -  7.38e-02..8.92e-02 (     8)  2.15e-02..2.50e-01 (     8)
rows    ramp_wave  32  2.47e-04..2.82e-03 (    35)  2.25e-02..2.60e-01 (     8)                            -  7.89e-02..2.50e-01 (     8)  2.22e-02..2.50e-01 (     9)
rows    random1    32  8.74e-04..2.46e-03 (   741)  2.32e-02..9.29e-02 (     9)  2.54e-02..1.15e-01 (     8)  1.14e-01..2.50e-01 (    25)  1.06e-01..2.50e-01 (    23)
rows    random2    32  2.61e-05..3.70e-04 (    10)  2.75e-02..1.28e-01 (     9)  5.03e-02..6.28e-02 (    15)  5.07e-02..5.00e-01 (     8)  5.08e-02..2.50e-01 (    12)
causal  flat       64  2.35e-04..2.50e-01 (   186)  1.99e-02..1.25e-01 (     9)  3.42e-02..1.08e-01 (     9)                            -  2.79e-02..2.50e-01 (     8)
causal  planted    64  2.50e-01..2.50e-01 ( 22713)  2.51e-01..2.65e-01 (   128)                            -                            -  4.39e-02..2.50e-01 (    22)
causal  ramp_rise  64  1.28e-03..2.50e-01 (   154)  5.96e-02..1.26e-01 (    20)  9.84e-02..1.08e-01 (     9)  1.02e-01..1.84e-01 (     9)  3.37e-02..2.50e-01 (     8)
causal  ramp_fall  64  4.08e-05..2.48e-01 (     8)  2.44e-02..1.24e-01 (     8)  1.21e-01..2.50e-01 (     8)  4.43e-02..1.55e-01 (     8)  2.76e-02..2.50e-01 (     8)
causal  ramp_wave  64  1.23e-03..2.50e-01 (    99)  4.08e-02..1.33e-01 (    14)  4.10e-01..5.00e-01 (     9)  9.37e-02..2.45e-01 (     9)  3.47e-02..2.50e-01 (     9)
causal  random1    64  6.54e-04..2.50e-01 (   549)  2.16e-02..1.74e-01 (     8)  6.26e-02..2.50e-01 (     8)  5.20e-02..2.48e-01 (     8)  4.22e-02..2.50e-01 (    11)
causal  random2    64  2.40e-05..2.50e-01 (     9)  2.30e-02..2.24e-01 (     8)                            -  2.29e-01..2.50e-01 (     8)  5.39e-02..2.50e-01 (    13)
decode  flat       64                            -  2.27e-02..1.25e-01 (     9)                            -                            -                            -
decode  planted    64                            -  2.45e-01..3.46e-01 (   125)                            -                            -                            -
decode  ramp       64                            -  1.94e-02..1.49e-01 (     9)                            -                            -                            -
decode  random     64                            -  2.35e-02..1.66e-01 (     8)                            -                            -                            -
"""
import functools
import math

import torch

LOG2E = 1.4426950408889634
EDGES = (0, 31, 32, 63, 64, 65, 127, 128)
FULL_L = (1, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 333)
DECODE_N = (1, 2, 7, 8, 9, 10, 63, 64, 65, 66, 80)       # n_keys; the step variant runs at pos = n_keys - 1
DECODE_LMAX = 80
POISON_ROWS = 8
POISON_V = 1000.0
ABS_FLOOR = 1e-6        # of a bf16 output row that is zero in the reference (planted dQ / dK): far below one miscounted element of O(1) inputs
REL_CAP = 0.5           # no row-relative tolerance above this, whatever the mutants allow
DETECT = 32.0           # a mutant counts in a quantity when it moves it by at least DETECT x noise
# (family, quantity) pairs that a case may leave unasserted (Bars.tol is None): no mutant moves the quantity by 32 x its noise there, or the
# bar that follows would not stay below REL_CAP.  tests/test_attention_cases_cpu.py asserts that nothing outside this table is left out and
# that every entry is in use.
_DS0 = "o_i = v[target(i)], so dS = 0 in exact arithmetic: dQ and dK are rounding residue that no miscount moves"
_ILL = ("sum_j dS_ij = 0 meets a ramp coordinate |k_0| of 100 and more; delta comes from the bf16 o, so the row's own noise reaches 10 % and "
        "more and no single miscount stands 32 x above it (dV, o and lse2 carry these cases; flat and random1 carry dQ / dK)")
_PEAK = "score std 4: a few keys hold the weight, delta's rounding dominates dS as in the ramps; random1 carries dQ / dK"
NOT_ASSERTED = {
    ("flat", "dk"): "q = 0: dK is identically 0 whatever is counted",
    ("flat", "dq"): "L = 1 only: one key, dS = 0",
    ("flat", "o"): "L >= 333 only: one key in L moves the mean by less than 32 bf16 roundings; lse2 (exact) carries the forward there",
    ("planted", "dq"): _DS0, ("planted", "dk"): _DS0,
    ("planted", "o"): "L = 1 only: o = v_0 whatever is counted",
    ("ramp_rise", "dq"): _ILL, ("ramp_rise", "dk"): _ILL, ("ramp_fall", "dq"): _ILL, ("ramp_fall", "dk"): _ILL,
    ("ramp_wave", "dq"): _ILL, ("ramp_wave", "dk"): _ILL,
    ("random1", "dq"): "L = 1 (dS = 0) and five more cases where no single miscount reaches 32 x noise",
    ("random1", "dk"): "L = 1 only: dS = 0",
    ("random2", "dq"): _PEAK, ("random2", "dk"): _PEAK,
}
# (family, mutant with its index stripped) pairs that some case of the family cannot see in any asserted quantity.  Every one of them is
# seen by another family at the same shape (asserted per shape in the CPU test); the table is asserted to be exact.
_W = "the miscounted key or query weighs 2^-10 and less next to the ramp's maximum (or, for a kept suffix, no kept query weighs it)"
_T = "no kept / visible query targets that key"
_Q = "touches dQ alone, which this family does not assert"
EXEMPT_MUTANTS = {
    ("flat", "fwd_rows_first+1"): "q = 0: every query row has the same lse2 and o", ("flat", "fwd_rows_first-1"): "q = 0: every query row has the same lse2 and o",
    ("planted", "fwd_zero_key"): "a zero key weighs 2^-46 (hd 32: 2^-65) of the planted one",
    ("planted", "bwd_dup_last_key"): _Q, ("planted", "fwd_drop_key"): _T, ("planted", "bwd_drop_key"): _T, ("planted", "fwd_dup_last_key"): _T,
    ("ramp_rise", "bwd_dup_last_key"): _Q, ("ramp_fall", "bwd_dup_last_key"): _Q, ("ramp_wave", "bwd_dup_last_key"): _Q,
    ("ramp_rise", "fwd_zero_key"): _W, ("ramp_fall", "fwd_zero_key"): _W, ("ramp_wave", "fwd_zero_key"): _W,
    ("ramp_rise", "fwd_drop_key"): _W, ("ramp_fall", "fwd_drop_key"): _W, ("ramp_wave", "fwd_drop_key"): _W,
    ("ramp_rise", "bwd_drop_key"): _W, ("ramp_fall", "bwd_drop_key"): _W, ("ramp_wave", "bwd_drop_key"): _W,
    ("ramp_rise", "bwd_drop_query"): _W, ("ramp_fall", "bwd_drop_query"): _W, ("ramp_wave", "bwd_drop_query"): _W,
    ("ramp_fall", "fwd_dup_last_key"): _W, ("ramp_fall", "fwd_hide_self"): _W, ("ramp_fall", "fwd_see_next"): _W,
    ("ramp_fall", "bwd_rows_first+1"): _W, ("ramp_fall", "bwd_rows_first-1"): _W, ("ramp_wave", "bwd_rows_first+1"): _W, ("ramp_wave", "bwd_rows_first-1"): _W,
    ("random1", "bwd_dup_last_key"): "moves dQ by P_i,L-1 of a row, under 32 x noise where L - 1 has little weight", ("random1", "bwd_drop_key"): "causal L = 333, key 332: one query sees it",
    ("random2", "bwd_dup_last_key"): _Q, ("random2", "bwd_drop_key"): "keys few queries weigh; dQ / dK unasserted", ("random2", "fwd_drop_key"): "a key no kept query weighs",
    ("random2", "fwd_dup_last_key"): "key L - 1 weighs little for every kept / visible query", ("random2", "fwd_zero_key"): "a zero key next to scores of std 4",
    ("random2", "fwd_hide_self"): "the diagonal key weighs little for that query", ("random2", "fwd_see_next"): "key i + 1 weighs little for query i",
}


def mutant_class(name):
    """the mutant's name without its trailing index"""
    head, _, tail = name.rpartition("_")
    return head if tail.isdigit() else name


# mutants that are provably no-ops for a kernel that recomputes P from lse2 (exempt from "must be caught"):
#   bwd_zero_key: a padded key with k = 0 adds dS * 0 to dQ, and its own dK / dV rows are never stored
EXEMPT = ("bwd_zero_key",)


def edges(L, q_begin=0):
    """the boundary indices of a case: tile and half-tile edges, the last two rows, and the rows around q_begin"""
    e = set(EDGES) | {L - 2, L - 1}
    if q_begin:
        e |= {q_begin - 1, q_begin, q_begin + 1}
    return sorted(i for i in e if 0 <= i < L)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, g, lo=1, hi=8):
    """nonzero integers with lo <= |v| <= hi"""
    mag = torch.randint(lo, hi + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return mag * sign


class Case:
    """kind: 'full' (q_begin = 0 or a kept suffix) | 'causal'.  qkv is rows [0, B * L) of `backing`, bf16 [B * L + POISON_ROWS, 3 * H * hd]
    in the kernels' packed layout [B, L, 3, H, hd]; dO bf16 [B * (L - q_begin), H * hd]."""

    def __init__(self, kind, family, B, L, H, hd, q_begin, backing, dO, planted=None):
        self.kind, self.family, self.B, self.L, self.H, self.hd, self.q_begin = kind, family, B, L, H, hd, q_begin
        self.backing, self.dO, self.planted = backing, dO, planted
        self.causal = kind == "causal"

    @property
    def qkv(self):
        return self.backing[: self.B * self.L]

    def qkv64(self):
        """q, k, v float64 [B, H, L, hd]"""
        x = self.qkv.double().reshape(self.B, self.L, 3, self.H, self.hd).permute(2, 0, 3, 1, 4)
        return x[0], x[1], x[2]

    def dO64(self):
        return self.dO.double().reshape(self.B, self.L - self.q_begin, self.H, self.hd).permute(0, 2, 1, 3)


def _planted_layout(B, L, q_begin, interseq):
    """per sequence: the special indices and their coordinates; sequences alternate between two disjoint coordinate sets, so the poison
    a sequence would find behind its end (coordinates of ITS specials) is invisible to the sequence that owns those rows"""
    lay = []
    for b in range(B):
        sp = edges(L, q_begin)
        if interseq and b > 0:
            sp = [i for i in sp if i >= POISON_ROWS]        # rows 0..7 of a following sequence hold the poison
        sp = sp[-14:]
        lay.append((sp, [n + (b % 2) * 14 for n in range(len(sp))]))      # 28 coordinates at the most: fits head_dim 32
    return lay


def build_case(kind, family, L, hd, q_begin=0, B=2, H=2, seed=0):
    g = _gen(1000 * L + 10 * hd + q_begin + seed + {"flat": 1, "planted": 2, "ramp_rise": 3, "ramp_fall": 4, "ramp_wave": 5, "random1": 6, "random2": 7}[family])
    causal = kind == "causal"
    Lq = L - q_begin
    q = torch.zeros(B, H, L, hd, dtype=torch.float64)
    k = torch.zeros_like(q)
    v = _ints((B, H, L, hd), g)
    dO = _ints((B, H, Lq, hd), g, 1, 4)
    dO[:, :, Lq - 1] *= 8                                    # the query a clamped load repeats: loud enough to show in dK / dV at any L
    # poison behind the tensor: every family gets a loud key there
    tail_k = torch.zeros(POISON_ROWS, H, hd, dtype=torch.float64)
    tail_v = torch.full((POISON_ROWS, H, hd), POISON_V, dtype=torch.float64)
    tail_q = torch.zeros_like(tail_k)
    if family == "flat":
        k = _ints((B, H, L, hd), g, 1, 3)
        k[:, :, L - 1] *= 32                                 # the key a clamped load repeats: loud enough to show in dQ at any L
        tail_k[:] = 3.0
    elif family == "planted":
        interseq = (not causal) and L >= 2 * POISON_ROWS
        lay = _planted_layout(B, L, q_begin, interseq)
        k = 0.5 * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        q = torch.zeros(B, H, L, hd, dtype=torch.float64)
        for b, (sp, co) in enumerate(lay):
            for idx, a in zip(sp, co):
                k[b, :, idx] = 0.0
                k[b, :, idx, a] = 16.0
            for i in range(L):
                vis = [n for n in range(len(sp)) if (not causal) or sp[n] <= i]
                n = sp.index(i) if causal and i in sp else vis[i % len(vis)]      # causal: a special query targets its own key (the diagonal)
                q[b, :, i, co[n]] = 16.0
            if causal:                                       # the key after a special one is twice as loud on ITS coordinate: query i must not see key i + 1
                for idx, a in zip(sp, co):
                    if idx + 1 < L:
                        k[b, :, idx + 1, a] = 32.0
            if interseq and b > 0:                           # poison for sequence b - 1: its own special coordinates, twice as loud
                pco = lay[b - 1][1]
                for r in range(POISON_ROWS):
                    k[b, :, r] = 0.0
                    k[b, :, r, pco[len(pco) - 1 - (r % len(pco))]] = 32.0
                    v[b, :, r] = POISON_V
        co = lay[B - 1][1]
        for r in range(POISON_ROWS):
            tail_k[r, :, co[len(co) - 1 - (r % len(co))]] = 64.0
    elif family.startswith("ramp"):
        # scaled score of a ramp query against key j, in log2 units: a step of 10 at every 64-key tile and a slope inside it, so that even a
        # one-key tail tile lies more than 8 above the reference point the tile before it left; 317 at L = 1536: fp32 holds
        j = torch.arange(L, dtype=torch.float64)
        if family == "ramp_wave":
            up = 10.0 * (j // 64) + 0.3 * (32 * (j // 64) + torch.clamp(j % 64, max=31))     # 32 keys of ramp, 32 flat, in every tile
        else:
            up = 10.0 * (j // 64) + 0.05 * j
        if family == "ramp_fall":
            up = up.flip(0)
        r = up / (4.0 * hd ** -0.5 * LOG2E)
        k = 0.25 * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        q = 0.25 * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        k[..., 0] = r
        q[..., 0] = 4.0
        q[:, :, 3::8, 0] = 0.0                               # probe queries: every key weighs about 1 / visible
        q[:, :, 3::8, 1:] *= 4.0
        tail_k[:, :, 0] = float(r.max()) + 64.0
    else:
        std = 1.0 if family == "random1" else 2.0
        q = std * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        k = std * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        v = std * torch.randn(B, H, L, hd, generator=g, dtype=torch.float64)
        dO = std * torch.randn(B, H, Lq, hd, generator=g, dtype=torch.float64)
        tail_k[:] = 4.0 * std
    body = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * hd)     # [B, L, 3, H, hd]
    tail = torch.stack([tail_q, tail_k, tail_v], 1).reshape(POISON_ROWS, 3 * H * hd)
    backing = torch.cat([body, tail], 0).to(torch.bfloat16).contiguous()
    dOb = dO.permute(0, 2, 1, 3).reshape(B * Lq, H * hd).to(torch.bfloat16).contiguous()
    case = Case(kind, family, B, L, H, hd, q_begin, backing, dOb)
    if family == "planted":                                  # target(i): the visible key with the largest score
        qq, kk, _ = case.qkv64()
        s = qq @ kk.transpose(-1, -2)
        if causal:
            s = s + torch.where(torch.arange(L)[None, :] <= torch.arange(L)[:, None], 0.0, -math.inf)
        case.planted = s.argmax(-1)
    return case


# ------------------------------------------------------------------------------------------------------------------ reference
class Ref:
    """float64 evaluation of one case with per-(query, key) multiplicities.  Every sum of the formula is weighted:
         forward   l_i = sum_j Wf_ij 2^(s_ij)   o_i = sum_j Wf_ij 2^(s_ij) v_j / l_i   (+ `extra` zero keys: score 0, v = 0)
         backward  P = 2^(s - lse2) from the TRUE lse2 (the kernels recompute it);  dS = P (dO v^T - delta),  delta_i = dO_i . o_i
                   dQ_i = scale sum_j Wq_ij dS_ij k_j;  dK_j = scale sum_i Wk_ij dS_ij q_i;  dV_j = sum_i Wk_ij P_ij dO_i
       W = the visibility mask (forward) or all ones on the visible part (backward) for the reference, one entry changed for a mutant.
       `emulate` rounds where the kernel rounds: the noise estimate."""

    def __init__(self, case):
        self.c = case
        self.q, self.k, self.v = case.qkv64()
        self.dO = case.dO64()
        self.scale = case.hd ** -0.5
        L, qb = case.L, case.q_begin
        self.qi = torch.arange(qb, L)
        self.vis = torch.ones(L - qb, L, dtype=torch.float64)
        if case.causal:
            self.vis = (torch.arange(L)[None, :] <= self.qi[:, None]).double()
        self.qk = self.q[:, :, qb:]
        self.raw = self.qk @ self.k.transpose(-1, -2)          # sums of exact bf16 products
        self.s2 = self.raw * (self.scale * LOG2E)
        self.m = (self.s2 + torch.where(self.vis > 0, 0.0, -math.inf)).amax(-1, keepdim=True)
        self.E = torch.exp2(self.s2 - self.m)                  # unmasked: a mutant may count a key the mask hides
        self.base = self.forward()
        lse, o = self.base["lse2"], self.base["o"]
        self.P = torch.exp2(self.s2 - lse.unsqueeze(-1)) * self.vis
        self.dS = self.P * (self.dO @ self.v.transpose(-1, -2) - (self.dO * o).sum(-1, keepdim=True))
        self.base.update(self.backward())

    def forward(self, Wf=None, extra=0, qshift=None):
        if qshift is not None:                                           # a kept suffix that starts one query off: row r holds query q_begin + r + qshift
            full = self.all_queries()
            idx = self.qi + qshift
            return {"lse2": full["lse2"][:, :, idx], "o": full["o"][:, :, idx]}
        EW = self.E * (self.vis if Wf is None else Wf)
        l = EW.sum(-1, keepdim=True) + extra * torch.exp2(-self.m)
        return {"lse2": (self.m + torch.log2(l)).squeeze(-1), "o": EW @ self.v / l}

    def backward(self, Wq=None, Wk=None, add_query=False):
        c = self.c
        dSq = self.dS if Wq is None else self.dS * Wq
        dSk, Pk = (self.dS, self.P) if Wk is None else (self.dS * Wk, self.P * Wk)
        dq = torch.zeros_like(self.q)
        dq[:, :, c.q_begin:] = self.scale * (dSq @ self.k)
        dk = self.scale * (dSk.transpose(-1, -2) @ self.qk)
        dv = Pk.transpose(-1, -2) @ self.dO
        if add_query:                                          # the query before q_begin joins, with the dO row of the first kept one
            full = self.all_queries()
            i = c.q_begin - 1
            s_i = (self.q[:, :, i:i + 1] @ self.k.transpose(-1, -2)) * (self.scale * LOG2E)
            P_i = torch.exp2(s_i - full["lse2"][:, :, i:i + 1].unsqueeze(-1))
            dO_i = self.dO[:, :, :1]
            dS_i = P_i * (dO_i @ self.v.transpose(-1, -2) - (dO_i * full["o"][:, :, i:i + 1]).sum(-1, keepdim=True))
            dq[:, :, i:i + 1] = self.scale * (dS_i @ self.k)
            dk = dk + self.scale * (dS_i.transpose(-1, -2) @ self.q[:, :, i:i + 1])
            dv = dv + P_i.transpose(-1, -2) @ dO_i
        return {"dq": dq, "dk": dk, "dv": dv}

    def all_queries(self):
        """lse2 / o of every query of the sequence, no mask (the _rows mutants need the rows before q_begin)"""
        s2 = (self.q @ self.k.transpose(-1, -2)) * (self.scale * LOG2E)
        m = s2.amax(-1, keepdim=True)
        E = torch.exp2(s2 - m)
        l = E.sum(-1, keepdim=True)
        return {"lse2": (m + torch.log2(l)).squeeze(-1), "o": E @ self.v / l}

    def emulate(self):
        """the same formula rounded where the kernel rounds: scores, exponentials, sums, lse2, dP and delta in fp32; P and dS to bf16 before
        their products; o, dQ, dK, dV to bf16; delta from the rounded o"""
        f32 = lambda t: t.float().double()
        b16 = lambda t: t.to(torch.bfloat16).double()
        c = self.c
        s2 = f32(f32(self.raw) * float(torch.tensor(self.scale * LOG2E, dtype=torch.float32)))
        m = (s2 + torch.where(self.vis > 0, 0.0, -math.inf)).amax(-1, keepdim=True)
        neg = torch.where(self.vis > 0, 0.0, -math.inf)           # masked before the exponential: 2^277 is no fp32 number
        E = f32(torch.exp2(s2 + neg - m))
        l = f32(E.sum(-1, keepdim=True))
        lse = f32(m + f32(torch.log2(l))).squeeze(-1)
        o = b16(b16(E) @ self.v / l)
        P = f32(torch.exp2(s2 + neg - lse.unsqueeze(-1)))
        # dP and delta are fp32 accumulations in two different orders (a matrix product and a row sum): where they cancel (dS of a row with
        # one dominant key is 0 in exact arithmetic) what is left is their accumulation error, so both are really summed in fp32 here
        dP = (self.dO.float() @ self.v.float().transpose(-1, -2)).double()
        delta = (self.dO.float() * o.float()).sum(-1, keepdim=True).double()
        dS = b16(P * f32(dP - delta))
        dq = torch.zeros_like(self.q)
        dq[:, :, c.q_begin:] = b16(self.scale * (dS @ self.k))
        return {"lse2": lse, "o": o, "dq": dq, "dk": b16(self.scale * (dS.transpose(-1, -2) @ self.qk)), "dv": b16(b16(P).transpose(-1, -2) @ self.dO)}

    # -------------------------------------------------------------------------------------------------------------- mutants
    def mutants(self):
        """name -> ("fwd" | "bwd", kwargs of forward() / backward()).  Forward mutants are judged on lse2 and o, backward mutants on dQ,
        dK and dV.  Left out where they are provably the reference: a dropped key when it is the only one, the last key counted twice in
        the backward at L = 1 (one key: the softmax is constant and dS = 0), a suffix that starts one query late when it is one query long
        (the clamped read repeats that query)."""
        c = self.c
        L, qb = c.L, c.q_begin
        vis = self.vis
        ones = torch.ones_like(vis)
        out = {}

        def put(W, rows, cols, val):
            W = W.clone()
            W[rows, cols] = val
            return W

        idx = edges(L, qb)
        for j in idx:
            if L > 1:
                W = put(vis, slice(None), j, 0.0)
                lone = W.sum(-1) == 0                           # causal query 0 sees key 0 only: it keeps its key
                W[lone] = vis[lone]
                out[f"fwd_drop_key_{j}"] = ("fwd", dict(Wf=W))
                Wb = put(ones, slice(None), j, 0.0)
                out[f"bwd_drop_key_{j}"] = ("bwd", dict(Wq=Wb, Wk=Wb))
        out["fwd_zero_key"] = ("fwd", dict(extra=1))
        out["fwd_dup_last_key"] = ("fwd", dict(Wf=put(vis, slice(None), L - 1, 2.0 * vis[:, L - 1])))
        if L > 1:
            out["bwd_dup_last_key"] = ("bwd", dict(Wq=put(ones, slice(None), L - 1, 2.0)))
        out["bwd_zero_key"] = ("bwd", dict())
        for i in idx:
            if i >= qb:
                Wb = put(ones, i - qb, slice(None), 0.0)
                out[f"bwd_drop_query_{i}"] = ("bwd", dict(Wq=Wb, Wk=Wb))
        out["bwd_dup_last_query"] = ("bwd", dict(Wk=put(ones, L - 1 - qb, slice(None), 2.0)))
        if c.causal:
            for i in idx:
                if i + 1 < L:
                    out[f"fwd_see_next_{i}"] = ("fwd", dict(Wf=put(vis, i, i + 1, 1.0)))
                if i > 0:
                    out[f"fwd_hide_self_{i}"] = ("fwd", dict(Wf=put(vis, i, i, 0.0)))
        if qb:
            if L - qb > 1:
                out["fwd_rows_first+1"] = ("fwd", dict(qshift=torch.cat([torch.ones(L - qb - 1, dtype=torch.long), torch.zeros(1, dtype=torch.long)])))
            out["fwd_rows_first-1"] = ("fwd", dict(qshift=-1))
            Wb = put(ones, 0, slice(None), 0.0)
            out["bwd_rows_first+1"] = ("bwd", dict(Wq=Wb, Wk=Wb))
            out["bwd_rows_first-1"] = ("bwd", dict(add_query=True))
        return out

    def mutant(self, name):
        part, kw = self.mutants()[name]
        return self.forward(**kw) if part == "fwd" else self.backward(**kw)


FWD_Q = ("lse2", "o")
BWD_Q = ("dq", "dk", "dv")


def row_err(name, a, ref):
    """per-row distance [B, H, rows] from the reference: absolute for lse2; for o, dQ, dK, dV the L2 norm of the row's error relative to
    the L2 norm of the reference row, which is floored at 2^-6 of the largest row (and at ABS_FLOOR) so that the small and the zero
    rows are judged too"""
    d = (a.double() - ref.double())
    if name == "lse2":
        return d.abs()
    n = ref.double().norm(dim=-1)
    return d.norm(dim=-1) / n.clamp(min=max(2.0 ** -6 * float(n.max()), ABS_FLOOR))


def _unit(name, ref):
    return 2.0 ** -23 * float(ref.abs().max().clamp(min=1.0)) if name == "lse2" else 2.0 ** -9


class Bars:
    """noise, per-mutant deviations and the tolerances of one case"""

    def __init__(self, case):
        ref = Ref(case)
        self.case, self.ref = case, ref
        base = ref.base
        emu = ref.emulate()
        self.noise = {n: max(float(row_err(n, emu[n], base[n]).max()), _unit(n, base[n])) for n in FWD_Q + BWD_Q}
        self.dev = {}
        for name, (part, kw) in ref.mutants().items():
            if name in EXEMPT:
                continue
            r = ref.forward(**kw) if part == "fwd" else ref.backward(**kw)
            self.dev[name] = {n: float(row_err(n, r[n], base[n]).max()) for n in r}
        self.tol = {}                                          # None: the quantity is not asserted in this case (see NOT_ASSERTED)
        for n in FWD_Q + BWD_Q:
            seen = [d[n] for d in self.dev.values() if n in d and d[n] >= DETECT * self.noise[n]]
            t = min(seen) / 4 if seen else None
            if t is not None and n != "lse2":                  # row-relative: a bar of 1 would pass an all-zero row
                t = min(t, REL_CAP)
            self.tol[n] = t if t is not None and t >= 8 * self.noise[n] else None

    def undetected(self):
        """mutants that no ASSERTED quantity of this case sees"""
        return [m for m, d in self.dev.items() if not any(self.tol[n] is not None and v >= DETECT * self.noise[n] for n, v in d.items())]


@functools.lru_cache(maxsize=None)
def bars(kind, family, L, hd, q_begin=0, B=2, H=2):
    return Bars(build_case(kind, family, L, hd, q_begin, B, H))


FAMILIES = ("flat", "planted", "ramp_rise", "ramp_fall", "ramp_wave", "random1", "random2")


def case_keys():
    """(kind, family, L, hd, q_begin, B, H) of every prefill case: every family at every length and every kept suffix; the one L = 1536
    shape (H = 1, head_dim 64) with flat and ramp_rise only (its float64 reference and mutants cost seconds per case on the CPU)."""
    keys = []
    for hd in (64, 32):
        keys += [("full", fam, L, hd, 0, 2, 2) for L in FULL_L for fam in FAMILIES]
        if hd == 64:
            keys += [("full", fam, 1536, hd, 0, 2, 1) for fam in ("flat", "ramp_rise")]
        keys += [("full", fam, L, hd, qb, 2, 2) for L, qb in ((129, 64), (129, 128), (193, 128), (193, 192), (333, 64), (333, 320)) for fam in FAMILIES]
    keys += [("causal", fam, L, 64, 0, 2, 2) for L in FULL_L for fam in FAMILIES]
    keys += [("causal", fam, 1536, 64, 0, 2, 1) for fam in ("flat", "ramp_rise")]
    return keys


def key_id(key):
    kind, fam, L, hd, qb, B, H = key
    return f"{kind}-{fam}-hd{hd}-L{L}" + (f"-q{qb}" if qb else "") + (f"-H{H}" if H != 2 else "")


# --------------------------------------------------------------------------------------------------------------------- decode
class DecodeCase:
    """q bf16 [B, H, 64]; caches bf16 [Bmax, H, Lmax, 64]; keys 0 .. n_keys - 1 of sequences 0 .. B - 1 are visible.  Everything else in
    the caches is poison where the family has one."""

    def __init__(self, family, n_keys, B=2, Bmax=3, H=2, Lmax=DECODE_LMAX, seed=0):
        g = _gen(77 * n_keys + seed + len(family))
        self.family, self.n_keys, self.B, self.Bmax, self.H, self.Lmax = family, n_keys, B, Bmax, H, Lmax
        q = torch.zeros(B, H, 64, dtype=torch.float64)
        kc = torch.randn(Bmax, H, Lmax, 64, generator=g, dtype=torch.float64)
        vc = _ints((Bmax, H, Lmax, 64), g)
        self.planted = None
        self._bars = None
        if family == "flat":
            pass                                               # q = 0; poison below has score 0 too and v = 1000: one counted key moves o by 1000 / n
        elif family == "planted":
            sp = [i for i in sorted({0, 6, 7, 8, 9, 31, 32, 62, 63, 64, n_keys - 2, n_keys - 1}) if 0 <= i < n_keys]
            self.planted = torch.zeros(B, H, dtype=torch.long)
            for b in range(B):
                for h in range(H):
                    for n, idx in enumerate(sp):
                        kc[b, h, idx] = 0.0
                        kc[b, h, idx, n] = 16.0
                    n = (len(sp) - 1 - (b * H + h)) % len(sp)           # (0, 0) targets the last visible key, the others walk back
                    q[b, h, n] = 16.0
                    self.planted[b, h] = sp[n]
        elif family == "ramp":                                 # the score rises by 0.36 log2 units per key: the last keys hold the weight
            q = 0.25 * torch.randn(B, H, 64, generator=g, dtype=torch.float64)
            kc = 0.25 * kc
            q[..., 0] = 4.0
            kc[..., 0] = torch.arange(Lmax, dtype=torch.float64) / 2
        else:
            q = 1.5 * torch.randn(B, H, 64, generator=g, dtype=torch.float64)
            vc = torch.randn(Bmax, H, Lmax, 64, generator=g, dtype=torch.float64)
        # poison: rows n_keys .. n_keys + 8 of the live sequences and the whole of the unused ones
        lo, hi = n_keys, min(Lmax, n_keys + POISON_ROWS + 1)
        pk = torch.zeros(Bmax, H, Lmax, 64, dtype=torch.float64)
        for b in range(Bmax):
            for h in range(H):
                if family == "planted":
                    a = int(torch.nonzero(q[min(b, B - 1), h])[0])
                    pk[b, h, :, a] = 32.0
                elif family == "ramp":
                    pk[b, h, :, 0] = Lmax
                else:
                    pk[b, h] = 4.0 * q[min(b, B - 1), h].sign() if family != "flat" else 3.0
        kc[:B, :, lo:hi], vc[:B, :, lo:hi] = pk[:B, :, lo:hi], POISON_V
        kc[B:], vc[B:] = pk[B:], POISON_V
        self.q, self.kc, self.vc = q.to(torch.bfloat16), kc.to(torch.bfloat16).contiguous(), vc.to(torch.bfloat16).contiguous()
        self.name = f"decode-{family}-n{n_keys}"

    def reference(self, drop=None, zero_key=False, dup_last=False, emulate=False):
        """o float64 [B, H, 64]; the mutants of the forward (a dropped key, a counted zero key, key n - 1 counted twice)"""
        n = self.n_keys
        q, k, v = self.q.double(), self.kc[: self.B, :, :n].double(), self.vc[: self.B, :, :n].double()
        s = torch.einsum("bhd,bhkd->bhk", q, k) * 0.125
        w = torch.ones(n, dtype=torch.float64)
        if drop is not None:
            w[drop] = 0.0
        if dup_last:
            w[n - 1] = 2.0
        if emulate:
            s = s.float().double()
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m) * w
        l = e.sum(-1, keepdim=True) + (torch.exp(-m) if zero_key else 0.0)
        p = e / l
        if emulate:
            p = p.to(torch.bfloat16).double()
        o = torch.einsum("bhk,bhkd->bhd", p, v)
        return o.to(torch.bfloat16).double() if emulate else o

    def mutants(self):
        """name -> kwargs of reference(); key n - 1 counted twice is left out at n = 1 (one key: o = v_0 whatever its weight)"""
        n = self.n_keys
        out = {"zero_key": dict(zero_key=True)}
        if n > 1:
            out["dup_last_key"] = dict(dup_last=True)
            for j in sorted({0, 6, 7, 8, 9, 31, 32, 62, 63, 64, n - 2, n - 1}):
                if 0 <= j < n:
                    out[f"drop_key_{j}"] = dict(drop=j)
        return out

    def bars(self):
        if self._bars is None:
            self._bars = self._compute_bars()
        return self._bars

    def _compute_bars(self):
        base = self.reference()
        noise = max(float(row_err("o", self.reference(emulate=True), base).max()), 2.0 ** -9)
        dev = {m: float(row_err("o", self.reference(**kw), base).max()) for m, kw in self.mutants().items()}
        seen = [d for d in dev.values() if d >= DETECT * noise]
        tol = min(min(seen) / 4, REL_CAP) if seen else None      # None: o is not asserted by tolerance in this case (DECODE_NOT_ASSERTED)
        return {"noise": noise, "dev": dev, "tol": tol if tol is not None and tol >= 8 * noise else None,
                "undetected": [m for m, d in dev.items() if d < DETECT * noise]}


@functools.lru_cache(maxsize=None)
def decode_case(family, n_keys):
    return DecodeCase(family, n_keys)


# the decode kernel returns o alone (no lse2) and rounds p / sum to bf16, 2^-9 relative, before the product with V
DECODE_NOT_ASSERTED = {("planted", 1): "one key: o = v_0 whatever is counted (the exact check against the planted integers remains)"}
_DW = "the key weighs too little for every query of the case (planted: not the target; ramp: 2^-10 and less of the last keys)"
DECODE_EXEMPT_MUTANTS = {
    ("flat", "zero_key"): "one zero key among n moves o by 1 / (n + 1) of itself: 32 x the bf16 rounding of p only up to n = 15",
    ("planted", "zero_key"): "a zero key weighs 2^-46 of the planted one", ("planted", "dup_last_key"): "o has no normaliser output: a target counted twice is the same o",
    ("planted", "drop_key"): _DW, ("ramp", "drop_key"): _DW, ("ramp", "zero_key"): "a zero key lies far below the ramp's maximum from 7 keys on",
    ("random", "drop_key"): "a key that weighs under 32 bf16 roundings of p", ("random", "dup_last_key"): "key n - 1 weighs too little (n = 63, 65, 66)",
    ("random", "zero_key"): "as flat, earlier: the scores spread the weight unevenly",
}


def decode_exempt(mutant, n_keys):
    """the one mutant no decode family sees at a shape: one zero key among n > 15 moves o by 1 / (n + 1) of itself, which is 32 x the bf16
    rounding of p / sum only up to n = 15"""
    return mutant == "zero_key" and n_keys > 15


def decode_keys():
    return [(fam, n) for fam in ("flat", "planted", "ramp", "random") for n in DECODE_N]


# ---------------------------------------------------------------------------------------------------------------------- table
def tolerance_table():
    groups = {}
    for key in case_keys():
        b = bars(*key)
        kind, fam, L, hd, qb, B, H = key
        kernel = "causal" if kind == "causal" else ("rows" if qb else "full")
        g = groups.setdefault((kernel, fam, hd), {n: [] for n in FWD_Q + BWD_Q})
        for n in FWD_Q + BWD_Q:
            if b.tol[n] is not None:
                g[n].append((b.tol[n], b.tol[n] / b.noise[n]))
    for fam, n in decode_keys():
        d = decode_case(fam, n).bars()
        g = groups.setdefault(("decode", fam, 64), {"o": []})
        if d["tol"] is not None:
            g["o"].append((d["tol"], d["tol"] / d["noise"]))
    lines = [f"{'kernel':7s} {'family':10s} {'hd':>2s} " + " ".join(f"{n + ' tol (min ratio)':>28s}" for n in FWD_Q + BWD_Q)]
    for (kernel, fam, hd), g in groups.items():
        cells = []
        for n in FWD_Q + BWD_Q:
            if not g.get(n):
                cells.append(f"{'-':>28s}")
                continue
            tols = [t for t, _ in g[n]]
            cells.append(f"{min(tols):9.2e}..{max(tols):8.2e} ({min(r for _, r in g[n]):6.0f})")
        lines.append(f"{kernel:7s} {fam:10s} {hd:2d} " + " ".join(cells))
    return "\n".join(lines)


if __name__ == "__main__":
    print(tolerance_table())
