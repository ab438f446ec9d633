"""Edge cases, float64 references and reference mutants of the packed variable-length attention kernels with grouped KV heads
(vt_attention_varlen_fwd / _bwd): n sequences one behind the other in [M, ...] operands, Hq query heads over Hkv KV heads, query head h on
KV head h // (Hq // Hkv).  Plain torch on the CPU: importing this module needs no GPU and no built library.

Exactly the bar rule of tests/attention_cases.py (its row_err, _ints, _unit, DETECT and REL_CAP are imported, its docstring has the rule): a
case is built from bf16 values, the reference evaluates the kernel's formula in float64 on those values, a MUTANT is the reference with one
key, query or head miscounted, noise is the distance of an evaluation that rounds where the kernel rounds, a mutant is detectable in a
quantity when it moves it by DETECT x noise, and the tolerance of a quantity is a quarter of the smallest detectable deviation, at most
REL_CAP row-relative; where that would be under 8 x noise, or nothing is detectable, the quantity is NOT ASSERTED in that case and
NOT_ASSERTED names the (family, quantity) with the reason.  Both numbers come from the reference alone, never from a kernel.

Mutants, per sequence b of a packing (names end in _b<seq>_<index>):
  leak_next / leak_prev   the first key of sequence b + 1 / the last key of sequence b - 1 counted by the queries of b: forward (lse2, o) and
                          backward (dQ of b, and what the foreign key's own dK / dV rows would receive)
  drop_key / drop_query   a key (forward, backward) or a query (backward: the dK/dV sweep streams the queries) dropped at each edges(L_b)
  dup_last_key / _query   the last key counted twice (forward, backward), the last query counted twice (backward)
and per case: wrong_kv_head (h % Hkv in place of h // g, forward and backward; absent at Hq == Hkv, where it is the reference itself) and
group_head_missing (the last query head of every group left out of the dK / dV sum).  Left out where they are the reference itself: a
dropped key and the backward's doubled key at L_b = 1.

Families, with the recipes of tests/cross_attention_cases.py per sequence: flat (q = 0: lse2 = log2(L_b), o the exact mean of V's integers),
planted (special keys 16 e_a at edges(L_b), query i = 16 e_a of special i mod n; neighbouring sequences use disjoint coordinate sets, and
the rows adjacent to a boundary -- the last row of b and the first row of b + 1, in sequences of 16 rows and more -- hold the NEIGHBOUR's
special coordinates twice as loud with v = 1000, so that a leaked row takes the whole softmax and o lands on 1000), ramp_rise (the lazy
rescale fires in every tile), random1 (N(0, 1)).  Poison rows (a loud key, v = 1000, a loud query, dO = 1000) sit behind every backing.

tests/test_varlen_attention_cases_cpu.py holds the tables and the detection power to account; tests/test_varlen_attention_gpu.py asserts
the kernels against these tolerances.
"""
import functools

import torch

from tests.attention_cases import DETECT, LOG2E, POISON_ROWS, POISON_V, REL_CAP, _gen, _ints, _unit, edges, row_err

HD = 64
PACKINGS = ((1, 193, 64, 65, 127, 128, 129, 333), (333, 129, 128, 127, 65, 64, 193, 1), (200,))
HEADS = ((2, 2), (4, 2), (6, 2))
FAMILIES = ("flat", "planted", "ramp_rise", "random1")
FWD_Q = ("lse2", "o")
BWD_Q = ("dq", "dk", "dv")

_DS0 = "o_i = v[target(i)], so dS = 0 in exact arithmetic: dQ and dK are rounding residue that no miscount moves"
_ILL = ("sum_j dS_ij = 0 meets a ramp coordinate |k_0| of 100 and more; delta comes from the bf16 o, so the row's own noise reaches 10 % and "
        "more and no single miscount stands 32 x above it (dV, o and lse2 carry these cases; flat and random1 carry dQ / dK)")
# (family, quantity) pairs that a case may leave unasserted (Bars.tol is None); the CPU test asserts that the table is exact
NOT_ASSERTED = {
    ("flat", "dk"): "q = 0: dK is identically 0 whatever is counted",
    ("planted", "dq"): _DS0, ("planted", "dk"): _DS0,
    ("ramp_rise", "dq"): _ILL, ("ramp_rise", "dk"): _ILL,
}


def cu_of(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return cu


class Case:
    """q is rows [0, M) of q_backing, bf16 [M + POISON_ROWS, 64 Hq]; k, v likewise with 64 Hkv columns; dO with 64 Hq"""

    def __init__(self, family, lengths, heads, q_backing, k_backing, v_backing, dO_backing):
        self.family, self.lengths, self.heads = family, tuple(lengths), tuple(heads)
        self.Hq, self.Hkv = heads
        self.cu = cu_of(lengths)
        self.M = self.cu[-1]
        self.q_backing, self.k_backing, self.v_backing, self.dO_backing = q_backing, k_backing, v_backing, dO_backing

    def heads64(self, backing, H):
        """float64 [H, M + POISON_ROWS, 64] of a backing (the poison rows included: a leak mutant reads the row behind a sequence)"""
        return backing.double().reshape(-1, H, HD).permute(1, 0, 2)


def build_case(family, lengths, heads, seed=0):
    Hq, Hkv = heads
    cu = cu_of(lengths)
    M, n = cu[-1], len(lengths)
    g = _gen(1000 * M + 100 * Hq + 10 * n + lengths[0] + seed + {"flat": 1, "planted": 2, "ramp_rise": 3, "random1": 6}[family])
    q = torch.zeros(Hq, M, HD, dtype=torch.float64)
    k = torch.zeros(Hkv, M, HD, dtype=torch.float64)
    v = _ints((Hkv, M, HD), g)
    dO = _ints((Hq, M, HD), g, 1, 4)
    tail_k = torch.zeros(Hkv, POISON_ROWS, HD, dtype=torch.float64)
    tail_q = torch.zeros(Hq, POISON_ROWS, HD, dtype=torch.float64)
    for b in range(n):
        dO[:, cu[b + 1] - 1] *= 8                             # the query a clamped load repeats: loud enough to show in dK / dV
    if family == "flat":
        k = _ints((Hkv, M, HD), g, 1, 3)
        for b in range(n):
            k[:, cu[b + 1] - 1] *= 32                         # the key a clamped load repeats: loud enough to show in dQ
        tail_k[:] = 3.0
        tail_q[:] = 3.0
    elif family == "planted":
        k = 0.5 * torch.randn(Hkv, M, HD, generator=g, dtype=torch.float64)
        lay = []
        for b, L in enumerate(lengths):
            sp = edges(L)
            if L >= 2 * POISON_ROWS:                          # the rows next to a boundary hold the neighbour's coordinates, not a special of their own
                sp = [i for i in sp if not (i == 0 and b > 0) and not (i == L - 1 and b < n - 1)]
            sp = sp[-14:]
            lay.append((sp, [c + (b % 2) * 14 for c in range(len(sp))]))
        for b, (L, (sp, co)) in enumerate(zip(lengths, lay)):
            a = cu[b]
            for idx, c in zip(sp, co):
                k[:, a + idx] = 0.0
                k[:, a + idx, c] = 16.0
            for i in range(L):
                q[:, a + i, co[i % len(sp)]] = 16.0
        for b, L in enumerate(lengths):                       # the neighbour's special coordinates, twice as loud, v = 1000
            if L < 2 * POISON_ROWS:
                continue
            if b > 0:
                k[:, cu[b]] = 0.0
                k[:, cu[b], lay[b - 1][1]] = 32.0
                v[:, cu[b]] = POISON_V
            if b < n - 1:
                k[:, cu[b + 1] - 1] = 0.0
                k[:, cu[b + 1] - 1, lay[b + 1][1]] = 32.0
                v[:, cu[b + 1] - 1] = POISON_V
        co = lay[n - 1][1]
        for r in range(POISON_ROWS):
            tail_k[:, r, co[len(co) - 1 - (r % len(co))]] = 64.0
            tail_q[:, r, co[r % len(co)]] = 16.0
    elif family == "ramp_rise":
        k = 0.25 * torch.randn(Hkv, M, HD, generator=g, dtype=torch.float64)
        q = 0.25 * torch.randn(Hq, M, HD, generator=g, dtype=torch.float64)
        top = 0.0
        for b, L in enumerate(lengths):
            j = torch.arange(L, dtype=torch.float64)
            r = (10.0 * (j // 64) + 0.05 * j) / (4.0 * HD ** -0.5 * LOG2E)
            k[:, cu[b]:cu[b + 1], 0] = r
            top = max(top, float(r.max()))
        q[..., 0] = 4.0
        q[:, 3::8, 0] = 0.0                                   # probe queries: every key weighs about 1 / L_b
        q[:, 3::8, 1:] *= 4.0
        tail_k[..., 0] = top + 64.0
        tail_q[..., 0] = 4.0
    else:
        q = torch.randn(Hq, M, HD, generator=g, dtype=torch.float64)
        k = torch.randn(Hkv, M, HD, generator=g, dtype=torch.float64)
        v = torch.randn(Hkv, M, HD, generator=g, dtype=torch.float64)
        dO = torch.randn(Hq, M, HD, generator=g, dtype=torch.float64)
        tail_k[:] = 4.0
        tail_q[:] = 4.0

    def rows(t, tail):
        return torch.cat([t, tail], 1).permute(1, 0, 2).reshape(M + POISON_ROWS, -1).to(torch.bfloat16).contiguous()
    tail_v = torch.full((Hkv, POISON_ROWS, HD), POISON_V, dtype=torch.float64)
    tail_d = torch.full((Hq, POISON_ROWS, HD), POISON_V, dtype=torch.float64)
    return Case(family, lengths, heads, rows(q, tail_q), rows(k, tail_k), rows(v, tail_v), rows(dO, tail_d))


class SeqRef:
    """One sequence in float64 with per-(query, key) multiplicities, as cross_attention_cases.Ref, for all Hq query heads at once.  The key
    axis holds the sequence's own L keys and behind them the two FOREIGN rows a leak would count (the row before the sequence and the row
    behind it: a neighbour's key, or the poison behind the allocation), whose multiplicity is 0 in the reference:
         forward   l_i = sum_j Wf_ij 2^(s_ij)   o_i = sum_j Wf_ij 2^(s_ij) v_j / l_i
         backward  P = 2^(s - lse2) from the TRUE lse2;  dS = P (dO v^T - delta),  delta_i = dO_i . o_i
                   dQ_i = scale sum_j Wq_ij dS_ij k_j;  dK_j = scale sum_h sum_i Wk_ij dS_ij q_i;  dV_j = sum_h sum_i Wk_ij P_ij dO_i
    with the sum over h running over the query heads of key j's group."""

    def __init__(self, q, k, v, dO, a, e, kv_of, Hkv):
        M = k.shape[1] - POISON_ROWS
        self.L = L = e - a
        self.Hkv, self.kv_of = Hkv, kv_of
        self.foreign = [a - 1 if a > 0 else None, e]          # global rows of the two foreign keys (None: nothing before row 0)
        cols = list(range(a, e)) + [r if r is not None else e for r in self.foreign]
        self.q, self.dO = q[:, a:e], dO[:, a:e]
        self.k, self.v = k[kv_of][:, cols], v[kv_of][:, cols]                      # [Hq, L + 2, 64]
        self.W0 = torch.cat([torch.ones(L, L, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)], 1)
        self.scale = HD ** -0.5
        self.raw = self.q @ self.k.transpose(-1, -2)
        self.s2 = self.raw * (self.scale * LOG2E)
        self.m = self.s2[..., :L].amax(-1, keepdim=True)
        self.E = torch.exp2(self.s2 - self.m)
        f = self.forward()
        self.lse, self.o = f["lse2"], f["o"]
        self.P = torch.exp2(self.s2 - self.lse.unsqueeze(-1))
        self.dS = self.P * (self.dO @ self.v.transpose(-1, -2) - (self.dO * self.o).sum(-1, keepdim=True))
        assert M >= e

    def forward(self, Wf=None):
        EW = self.E * (self.W0 if Wf is None else Wf)
        l = EW.sum(-1, keepdim=True)
        return {"lse2": (self.m + torch.log2(l)).squeeze(-1), "o": EW @ self.v / l}

    def group_sum(self, t, head_w=None):
        """[Hq, rows, 64] -> [Hkv, rows, 64]: the query heads of a group summed (head_w: a multiplicity per query head)"""
        if head_w is not None:
            t = t * head_w[:, None, None]
        out = torch.zeros(self.Hkv, *t.shape[1:], dtype=t.dtype)
        out.index_add_(0, torch.tensor(self.kv_of), t)
        return out

    def backward(self, Wq=None, Wk=None, head_w=None):
        """dk / dv come back for the L own keys AND the two foreign rows (zero in the reference)"""
        dSq = self.dS * (self.W0 if Wq is None else Wq)
        Wk = self.W0 if Wk is None else Wk
        dSk, Pk = self.dS * Wk, self.P * Wk
        return {"dq": self.scale * (dSq @ self.k), "dk": self.group_sum(self.scale * (dSk.transpose(-1, -2) @ self.q), head_w),
                "dv": self.group_sum(Pk.transpose(-1, -2) @ self.dO, head_w)}

    def emulate(self):
        """the same formula rounded where the kernel rounds: scores, exponentials, sums, lse2, dP and delta in fp32; P and dS to bf16 before
        their products; o, dQ to bf16; dK, dV summed over the group in fp32 and rounded to bf16 once; delta from the rounded o"""
        f32 = lambda t: t.float().double()
        b16 = lambda t: t.to(torch.bfloat16).double()
        L = self.L
        q, k, v, dO = self.q, self.k[:, :L], self.v[:, :L], self.dO
        s2 = f32(f32(self.raw[..., :L]) * float(torch.tensor(self.scale * LOG2E, dtype=torch.float32)))
        m = s2.amax(-1, keepdim=True)
        E = f32(torch.exp2(s2 - m))
        l = f32(E.sum(-1, keepdim=True))
        lse = f32(m + f32(torch.log2(l))).squeeze(-1)
        o = b16(b16(E) @ v / l)
        P = f32(torch.exp2(s2 - lse.unsqueeze(-1)))
        dP = (dO.float() @ v.float().transpose(-1, -2)).double()
        delta = (dO.float() * o.float()).sum(-1, keepdim=True).double()
        dS = b16(P * f32(dP - delta))
        return {"lse2": lse, "o": o, "dq": b16(self.scale * (dS @ k)), "dk": b16(self.scale * f32(self.group_sum(dS.transpose(-1, -2) @ q))),
                "dv": b16(f32(self.group_sum(b16(P).transpose(-1, -2) @ dO)))}


class Ref:
    """the whole case: base and emulate() as lse2 [Hq, M], o / dq [Hq, M, 64], dk / dv [Hkv, M, 64]; mutants as sparse changes of them"""

    def __init__(self, case, kv_of=None):
        self.c = case
        Hq, Hkv = case.heads
        g = Hq // Hkv
        self.kv_of = [h // g for h in range(Hq)] if kv_of is None else kv_of
        q, dO = case.heads64(case.q_backing, Hq), case.heads64(case.dO_backing, Hq)
        k, v = case.heads64(case.k_backing, Hkv), case.heads64(case.v_backing, Hkv)
        self.seqs = [SeqRef(q, k, v, dO, a, e, self.kv_of, Hkv) for a, e in zip(case.cu[:-1], case.cu[1:])]
        self.base = self.assemble([dict(s.forward(), **s.backward()) for s in self.seqs])

    def assemble(self, parts):
        out = {}
        for n in FWD_Q + BWD_Q:
            dim = 1
            out[n] = torch.cat([p[n][:, : s.L] for p, s in zip(parts, self.seqs)], dim)
        return out

    def emulate(self):
        return self.assemble([s.emulate() for s in self.seqs])

    def mutants(self):
        """name -> list of (quantity, row slice or index list into dim 1 of the base tensor, mutated rows): what the mutant changes"""
        cu, out = self.c.cu, {}
        Hq, Hkv = self.c.heads
        for b, s in enumerate(self.seqs):
            L, a = s.L, cu[b]
            own = slice(a, a + L)

            def put(rows, cols, val):
                W = s.W0.clone()
                W[rows, cols] = val
                return W

            def fwd(W):
                r = s.forward(Wf=W)
                return [("lse2", own, r["lse2"]), ("o", own, r["o"])]

            def bwd(Wq=None, Wk=None):
                r = s.backward(Wq=Wq, Wk=Wk)
                ch = [("dq", own, r["dq"]), ("dk", own, r["dk"][:, :L]), ("dv", own, r["dv"][:, :L])]
                for c, row in enumerate(s.foreign):          # what a foreign key's own gradient rows would receive on top of their own
                    if row is not None and row < self.c.M and Wk is not None and float(Wk[:, L + c].abs().sum()) > 0:
                        for n in ("dk", "dv"):
                            ch.append((n, slice(row, row + 1), self.base[n][:, row:row + 1] + r[n][:, L + c:L + c + 1]))
                return ch
            for name, c in (("leak_prev", 0), ("leak_next", 1)):
                if s.foreign[c] is None or not (0 <= s.foreign[c] < self.c.M):
                    continue                                  # only rows of a real neighbour (the poison behind the last sequence is what the packed-vs-separate test reads)
                W = put(slice(None), L + c, 1.0)
                out[f"fwd_{name}_b{b}"] = fwd(W)
                out[f"bwd_{name}_b{b}"] = bwd(Wq=W, Wk=W)
            if L > 1:
                for j in edges(L):
                    W = put(slice(None), j, 0.0)
                    out[f"fwd_drop_key_b{b}_{j}"] = fwd(W)
                    out[f"bwd_drop_key_b{b}_{j}"] = bwd(Wq=W, Wk=W)
                out[f"bwd_dup_last_key_b{b}"] = bwd(Wq=put(slice(None), L - 1, 2.0))
            out[f"fwd_dup_last_key_b{b}"] = fwd(put(slice(None), L - 1, 2.0))
            for i in edges(L):
                W = put(i, slice(None), 0.0) * s.W0
                out[f"bwd_drop_query_b{b}_{i}"] = bwd(Wq=W, Wk=W)
            out[f"bwd_dup_last_query_b{b}"] = bwd(Wk=put(L - 1, slice(0, L), 2.0))
        every = slice(0, self.c.M)
        if Hq != Hkv:
            wrong = Ref(self.c, kv_of=[h % Hkv for h in range(Hq)]).base
            out["wrong_kv_head"] = [(n, every, wrong[n]) for n in FWD_Q + BWD_Q]
        g = Hq // Hkv
        hw = torch.tensor([0.0 if h % g == g - 1 else 1.0 for h in range(Hq)], dtype=torch.float64)
        miss = self.assemble([dict(s.forward(), **s.backward(head_w=hw)) for s in self.seqs])
        out["group_head_missing"] = [(n, every, miss[n]) for n in ("dk", "dv")]
        return out


def _loudest_row(ref):
    """the reference row with the largest norm, [H, 1, 64]-shaped for every head: appended to a slice so that row_err's floor (a fraction of
    the largest row of the WHOLE tensor) is the same on the slice"""
    n = ref.norm(dim=-1)
    h, r = divmod(int(n.argmax()), n.shape[1])
    return ref[h:h + 1, r:r + 1].expand(ref.shape[0], 1, ref.shape[2])


def slice_err(name, rows, mutated, ref):
    """max row_err of a tensor that differs from the reference only in `rows` (dim 1)"""
    if name == "lse2":
        return float(row_err(name, mutated, ref[:, rows]).max())
    top = _loudest_row(ref)
    return float(row_err(name, torch.cat([mutated, top], 1), torch.cat([ref[:, rows], top], 1)).max())


class Bars:
    """noise, per-mutant deviations and the tolerances of one case: attention_cases.Bars on the packed, grouped reference"""

    def __init__(self, case):
        ref = Ref(case)
        self.case, self.ref = case, ref
        base = ref.base
        emu = ref.emulate()
        self.noise = {n: max(float(row_err(n, emu[n], base[n]).max()), _unit(n, base[n])) for n in FWD_Q + BWD_Q}
        self.dev = {}
        for name, changes in ref.mutants().items():
            d = {}
            for n, rows, t in changes:
                d[n] = max(d.get(n, 0.0), slice_err(n, rows, t, base[n]))
            self.dev[name] = d
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
def bars(family, lengths, heads):
    return Bars(build_case(family, lengths, heads))


def case_keys():
    return [(fam, lengths, heads) for lengths in PACKINGS for heads in HEADS for fam in FAMILIES]


def key_id(key):
    return f"{key[0]}-n{len(key[1])}first{key[1][0]}-h{key[2][0]}_{key[2][1]}"


if __name__ == "__main__":
    import time
    for key in case_keys():
        t0 = time.time()
        b = bars(*key)
        und = sorted({m.split("_b")[0] for m in b.undetected()})
        print(f"{key_id(key):32s} " + " ".join(f"{n} {'-' if b.tol[n] is None else format(b.tol[n], '.2e'):>9s} ({b.noise[n]:.1e})" for n in FWD_Q + BWD_Q),
              f"mutants {len(b.dev)} undetected: {und} {time.time() - t0:.1f}s")
