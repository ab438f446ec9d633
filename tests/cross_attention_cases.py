"""Edge cases, float64 references and reference mutants of the cross-attention kernels (vt_attention_cross_fwd / _bwd): Lq queries from
one operand, Lk keys and values from two others.  Plain torch on the CPU: importing this module needs no GPU and no built library.

Exactly the bar rule of tests/attention_cases.py (its row_err, _ints, _unit, DETECT and REL_CAP are imported, its docstring has the
rule): a case is built from bf16 values, the reference evaluates the kernel's formula in float64 on those values, a MUTANT is the
reference with one key or query miscounted, noise is the distance of an evaluation that rounds where the kernel rounds, a mutant is
detectable in a quantity when it moves it by DETECT x noise, and the tolerance of a quantity is a quarter of the smallest detectable
deviation, at most REL_CAP row-relative; where that would be under 8 x noise, or nothing is detectable, the quantity is NOT ASSERTED in
that case and NOT_ASSERTED names the (family, quantity) with the reason.  Both numbers come from the reference alone, never from a kernel.

Mutants: a dropped key at each edge index of Lk (forward, backward); one zero key counted (forward); the last key counted twice
(forward, backward); a dropped query at each edge index of Lq and the last query counted twice (backward: the dK / dV sweep streams
the queries).  Left out where they are the reference itself: a dropped key and the backward's doubled key at Lk = 1.

Families, with the recipes of the packed module's generators (B = 2, H = 2, so that a wrong batch or head stride reads a neighbour):
  flat       q = 0: lse2 = log2(Lk), o = the exact mean of V's integers; key Lk - 1 and query Lq - 1 (the rows a clamped load repeats) loud
  planted    special keys 16 e_a at edges(Lk), query i = 16 e_a of special i mod n: o_i = v[target(i)], an integer, to 1e-9; the two
             batches use disjoint coordinate sets and the first rows of batch 1 hold poison on batch 0's coordinates (Lk >= 16)
  ramp_rise  one coordinate of k grows by more than 8 log2 units per 64-key tile: the lazy rescale fires in every tile; probe queries
  random1    N(0, 1) operands
Poison rows (a loud key, v = 1000, a loud query, dO = 1000) sit behind every operand: q, k, v and dO are views of larger allocations.

tests/test_cross_attention_cases_cpu.py holds the tables and the detection power to account; tests/test_cross_attention_gpu.py
asserts the kernels against these tolerances.
"""
import functools

import torch

from tests.attention_cases import DETECT, LOG2E, POISON_ROWS, POISON_V, REL_CAP, _gen, _ints, _unit, edges, row_err

H, HD, B = 2, 64, 2
# tile, half-tile and 128-row block edges on each side independently; 320 x 64 is the design's 2048 x 256 reduced
SHAPES = ((1, 1), (1, 193), (129, 1), (64, 65), (65, 64), (127, 128), (128, 127), (200, 63), (333, 129), (320, 64))
FAMILIES = ("flat", "planted", "ramp_rise", "random1")
FWD_Q = ("lse2", "o")
BWD_Q = ("dq", "dk", "dv")

_ONE = "Lk = 1 only: one key, the softmax is constant and dS = 0"
_DS0 = "o_i = v[target(i)], so dS = 0 in exact arithmetic: dQ and dK are rounding residue that no miscount moves"
_ILL = ("sum_j dS_ij = 0 meets a ramp coordinate |k_0| of 100 and more; delta comes from the bf16 o, so the row's own noise reaches 10 % and "
        "more and no single miscount stands 32 x above it (dV, o and lse2 carry these cases; flat and random1 carry dQ / dK)")
# (family, quantity) pairs that a case may leave unasserted (Bars.tol is None); the CPU test asserts that the table is exact
NOT_ASSERTED = {
    ("flat", "dk"): "q = 0: dK is identically 0 whatever is counted",
    ("flat", "dq"): _ONE,
    ("planted", "dq"): _DS0, ("planted", "dk"): _DS0,
    ("planted", "o"): "Lk = 1 only: o = v_0 whatever is counted",
    ("ramp_rise", "dq"): "Lk = 1 (dS = 0), and at some shapes: " + _ILL, ("ramp_rise", "dk"): "Lk = 1 (dS = 0), and at some shapes: " + _ILL,
    ("random1", "dq"): _ONE, ("random1", "dk"): _ONE,
}


class Case:
    """q is rows [0, B * Lq) of q_backing, bf16 [B * Lq + POISON_ROWS, H * 64]; k, v likewise with Lk; dO likewise with Lq"""

    def __init__(self, family, Lq, Lk, q_backing, k_backing, v_backing, dO_backing, planted=None):
        self.family, self.Lq, self.Lk, self.B, self.H, self.hd = family, Lq, Lk, B, H, HD
        self.q_backing, self.k_backing, self.v_backing, self.dO_backing, self.planted = q_backing, k_backing, v_backing, dO_backing, planted

    def heads64(self, backing, L):
        """float64 [B, H, L, 64] of the first B * L rows"""
        return backing[: B * L].double().reshape(B, L, H, HD).permute(0, 2, 1, 3)


def build_case(family, Lq, Lk, seed=0):
    g = _gen(100000 * Lq + 10 * Lk + seed + {"flat": 1, "planted": 2, "ramp_rise": 3, "random1": 6}[family])
    q = torch.zeros(B, H, Lq, HD, dtype=torch.float64)
    k = torch.zeros(B, H, Lk, HD, dtype=torch.float64)
    v = _ints((B, H, Lk, HD), g)
    dO = _ints((B, H, Lq, HD), g, 1, 4)
    dO[:, :, Lq - 1] *= 8                                    # the query a clamped load repeats: loud enough to show in dK / dV
    tail_k = torch.zeros(POISON_ROWS, H, HD, dtype=torch.float64)
    tail_q = torch.zeros_like(tail_k)
    if family == "flat":
        k = _ints((B, H, Lk, HD), g, 1, 3)
        k[:, :, Lk - 1] *= 32                                # the key a clamped load repeats: loud enough to show in dQ
        tail_k[:] = 3.0
        tail_q[:] = 3.0
    elif family == "planted":
        interseq = Lk >= 2 * POISON_ROWS
        lay = []
        for b in range(B):
            sp = edges(Lk)
            if interseq and b > 0:
                sp = [i for i in sp if i >= POISON_ROWS]     # rows 0..7 of the following batch hold the poison
            sp = sp[-14:]
            lay.append((sp, [n + (b % 2) * 14 for n in range(len(sp))]))
        k = 0.5 * torch.randn(B, H, Lk, HD, generator=g, dtype=torch.float64)
        for b, (sp, co) in enumerate(lay):
            for idx, a in zip(sp, co):
                k[b, :, idx] = 0.0
                k[b, :, idx, a] = 16.0
            for i in range(Lq):
                q[b, :, i, co[i % len(sp)]] = 16.0
            if interseq and b > 0:                           # poison for batch b - 1: its own special coordinates, twice as loud
                pco = lay[b - 1][1]
                for r in range(POISON_ROWS):
                    k[b, :, r] = 0.0
                    k[b, :, r, pco[len(pco) - 1 - (r % len(pco))]] = 32.0
                    v[b, :, r] = POISON_V
        co = lay[B - 1][1]
        for r in range(POISON_ROWS):
            tail_k[r, :, co[len(co) - 1 - (r % len(co))]] = 64.0
            tail_q[r, :, co[r % len(co)]] = 16.0
    elif family == "ramp_rise":
        j = torch.arange(Lk, dtype=torch.float64)
        up = 10.0 * (j // 64) + 0.05 * j
        r = up / (4.0 * HD ** -0.5 * LOG2E)
        k = 0.25 * torch.randn(B, H, Lk, HD, generator=g, dtype=torch.float64)
        q = 0.25 * torch.randn(B, H, Lq, HD, generator=g, dtype=torch.float64)
        k[..., 0] = r
        q[..., 0] = 4.0
        q[:, :, 3::8, 0] = 0.0                               # probe queries: every key weighs about 1 / Lk
        q[:, :, 3::8, 1:] *= 4.0
        tail_k[:, :, 0] = float(r.max()) + 64.0
        tail_q[:, :, 0] = 4.0
    else:
        q = torch.randn(B, H, Lq, HD, generator=g, dtype=torch.float64)
        k = torch.randn(B, H, Lk, HD, generator=g, dtype=torch.float64)
        v = torch.randn(B, H, Lk, HD, generator=g, dtype=torch.float64)
        dO = torch.randn(B, H, Lq, HD, generator=g, dtype=torch.float64)
        tail_k[:] = 4.0
        tail_q[:] = 4.0
    tail_v = torch.full((POISON_ROWS, H, HD), POISON_V, dtype=torch.float64)

    def rows(t, L, tail):
        return torch.cat([t.permute(0, 2, 1, 3).reshape(B * L, H * HD), tail.reshape(POISON_ROWS, H * HD)], 0).to(torch.bfloat16).contiguous()
    case = Case(family, Lq, Lk, rows(q, Lq, tail_q), rows(k, Lk, tail_k), rows(v, Lk, tail_v), rows(dO, Lq, tail_v))
    if family == "planted":                                  # target(i): the key with the largest score
        s = case.heads64(case.q_backing, Lq) @ case.heads64(case.k_backing, Lk).transpose(-1, -2)
        case.planted = s.argmax(-1)
    return case


class Ref:
    """float64 evaluation of one case with per-(query, key) multiplicities, as attention_cases.Ref without mask and kept suffix:
         forward   l_i = sum_j Wf_ij 2^(s_ij)   o_i = sum_j Wf_ij 2^(s_ij) v_j / l_i   (+ `extra` zero keys: score 0, v = 0)
         backward  P = 2^(s - lse2) from the TRUE lse2;  dS = P (dO v^T - delta),  delta_i = dO_i . o_i
                   dQ_i = scale sum_j Wq_ij dS_ij k_j;  dK_j = scale sum_i Wk_ij dS_ij q_i;  dV_j = sum_i Wk_ij P_ij dO_i"""

    def __init__(self, case):
        self.c = case
        self.q, self.k, self.v = case.heads64(case.q_backing, case.Lq), case.heads64(case.k_backing, case.Lk), case.heads64(case.v_backing, case.Lk)
        self.dO = case.heads64(case.dO_backing, case.Lq)
        self.scale = HD ** -0.5
        self.raw = self.q @ self.k.transpose(-1, -2)
        self.s2 = self.raw * (self.scale * LOG2E)
        self.m = self.s2.amax(-1, keepdim=True)
        self.E = torch.exp2(self.s2 - self.m)
        self.base = self.forward()
        lse, o = self.base["lse2"], self.base["o"]
        self.P = torch.exp2(self.s2 - lse.unsqueeze(-1))
        self.dS = self.P * (self.dO @ self.v.transpose(-1, -2) - (self.dO * o).sum(-1, keepdim=True))
        self.base.update(self.backward())

    def forward(self, Wf=None, extra=0):
        EW = self.E if Wf is None else self.E * Wf
        l = EW.sum(-1, keepdim=True) + extra * torch.exp2(-self.m)
        return {"lse2": (self.m + torch.log2(l)).squeeze(-1), "o": EW @ self.v / l}

    def backward(self, Wq=None, Wk=None):
        dSq = self.dS if Wq is None else self.dS * Wq
        dSk, Pk = (self.dS, self.P) if Wk is None else (self.dS * Wk, self.P * Wk)
        return {"dq": self.scale * (dSq @ self.k), "dk": self.scale * (dSk.transpose(-1, -2) @ self.q), "dv": Pk.transpose(-1, -2) @ self.dO}

    def emulate(self):
        """the same formula rounded where the kernel rounds: scores, exponentials, sums, lse2, dP and delta in fp32; P and dS to bf16 before
        their products; o, dQ, dK, dV to bf16; delta from the rounded o"""
        f32 = lambda t: t.float().double()
        b16 = lambda t: t.to(torch.bfloat16).double()
        s2 = f32(f32(self.raw) * float(torch.tensor(self.scale * LOG2E, dtype=torch.float32)))
        m = s2.amax(-1, keepdim=True)
        E = f32(torch.exp2(s2 - m))
        l = f32(E.sum(-1, keepdim=True))
        lse = f32(m + f32(torch.log2(l))).squeeze(-1)
        o = b16(b16(E) @ self.v / l)
        P = f32(torch.exp2(s2 - lse.unsqueeze(-1)))
        dP = (self.dO.float() @ self.v.float().transpose(-1, -2)).double()
        delta = (self.dO.float() * o.float()).sum(-1, keepdim=True).double()
        dS = b16(P * f32(dP - delta))
        return {"lse2": lse, "o": o, "dq": b16(self.scale * (dS @ self.k)), "dk": b16(self.scale * (dS.transpose(-1, -2) @ self.q)),
                "dv": b16(b16(P).transpose(-1, -2) @ self.dO)}

    def mutants(self):
        """name -> ("fwd" | "bwd", kwargs of forward() / backward())"""
        Lq, Lk = self.c.Lq, self.c.Lk
        ones = torch.ones(Lq, Lk, dtype=torch.float64)
        out = {}

        def put(rows, cols, val):
            W = ones.clone()
            W[rows, cols] = val
            return W

        if Lk > 1:
            for j in edges(Lk):
                W = put(slice(None), j, 0.0)
                out[f"fwd_drop_key_{j}"] = ("fwd", dict(Wf=W))
                out[f"bwd_drop_key_{j}"] = ("bwd", dict(Wq=W, Wk=W))
            out["bwd_dup_last_key"] = ("bwd", dict(Wq=put(slice(None), Lk - 1, 2.0)))
        out["fwd_zero_key"] = ("fwd", dict(extra=1))
        out["fwd_dup_last_key"] = ("fwd", dict(Wf=put(slice(None), Lk - 1, 2.0)))
        for i in edges(Lq):
            W = put(i, slice(None), 0.0)
            out[f"bwd_drop_query_{i}"] = ("bwd", dict(Wq=W, Wk=W))
        out["bwd_dup_last_query"] = ("bwd", dict(Wk=put(Lq - 1, slice(None), 2.0)))
        return out


class Bars:
    """noise, per-mutant deviations and the tolerances of one case: attention_cases.Bars on the cross reference"""

    def __init__(self, case):
        ref = Ref(case)
        self.case, self.ref = case, ref
        base = ref.base
        emu = ref.emulate()
        self.noise = {n: max(float(row_err(n, emu[n], base[n]).max()), _unit(n, base[n])) for n in FWD_Q + BWD_Q}
        self.dev = {}
        for name, (part, kw) in ref.mutants().items():
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
def bars(family, Lq, Lk):
    return Bars(build_case(family, Lq, Lk))


def case_keys():
    return [(fam, Lq, Lk) for Lq, Lk in SHAPES for fam in FAMILIES]


def key_id(key):
    return f"{key[0]}-q{key[1]}-k{key[2]}"


if __name__ == "__main__":
    for key in case_keys():
        b = bars(*key)
        print(f"{key_id(key):22s} " + " ".join(f"{n} {'-' if b.tol[n] is None else format(b.tol[n], '.2e'):>9s} ({b.noise[n]:.1e})" for n in FWD_Q + BWD_Q),
              "undetected:", sorted({m.rsplit('_', 1)[0] if m.rsplit('_', 1)[-1].isdigit() else m for m in b.undetected()}))
