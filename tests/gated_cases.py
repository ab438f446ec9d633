"""Edge cases, float64 references, fp32 replays and reference mutants of the row passes of csrc/vt_gated.hip (vt_qknorm_rope_*,
vt_sigmoid_gate_*, vt_sigmoid_gate_cols_*, vt_geglu_*) and csrc/vt_stat.hip (vt_stat_gate_forward / _backward).  Plain torch on the CPU:
it needs no GPU and no built library.  Building a qknorm case imports video_tokenizer_amd.titok for the project's own rotary tables
(rope_tables_from_positions), so the package itself must import; nothing in it is loaded from libvt_hip.so.  The pattern is that of
tests/attention_cases.py.

A case is built from bf16 values and fp32 parameters drawn from a seed.  Its REFERENCE evaluates the kernel's formula in float64 on exactly
those values and rounds to bf16 where the kernel's header comment says a bf16 tensor is materialised (LayerNorm output, the transposed
rotation of the gradient, sigmoid, gelu, every product of two bf16 tensors, `logit`, `p`); the final rounding of an output is NOT applied --
it is part of the bar.  The REPLAY is the same function in float32: what an honest fp32 kernel may give.  A MUTANT is the reference with
one thing miscounted: the errors a lane, stride, tail or cap bug makes.

Every output is a whole backing buffer: the documented region holds the result, everything else (row padding, the other column blocks,
rows behind the tensor) holds POISON, and the bar there is 0.  A quantity Q carries
    cands   the accepted float64 values (more than one where the reference alone shows that an fp32 evaluation may round an intermediate
            to either neighbour: see `_either`)
    bar     per element (column sums: one scalar).  0 = the bf16 / fp32 bits of a candidate are required
    tight   the bar without the allowance for a flipped intermediate rounding; at most SHARE of a case's elements may need more
    ratio   max over elements of (distance to the nearest candidate) / bar     -- passes at <= 1
Elementwise bars are analytic, from the reference's own operands:  one final rounding (2^-8 |want| for bf16, since the half step of a value
is at most 2^-8 of it), plus one bf16 step (2^-7) of every rounded intermediate that feeds the element, plus a floor of fp32 arithmetic
(2^-20 of the operands' magnitudes; for LayerNorm that floor grows with 2^-22 max|x| rstd, the relative error fp32 statistics leave in
(x - mean) rstd; for gelu / gelu' the bound of test_gelu_grad_bits_on_every_bf16_magnitude, 4e-7 max(|u|, 1), times the other factor).
A mutant is CAUGHT by an elementwise quantity when its ratio is >= 4: the bar is at most 1/4 of what it has to catch.
Column sums (dq_w, dq_b, dk_w, dk_b, dw2, db2) follow the rule of tests/attention_cases.py with its constants: noise = `_sum_bound` of
tests/test_rows_edges_gpu.py on the float64 terms (plus, for the qknorm sums, two flipped roundings of g: 2^-6 of the largest term outside the last row), floored
at 2^-23 of the largest sum; a mutant is detectable at dev >= DETECT * noise; bar = 1/4 of the smallest detectable dev, and the quantity
is not asserted (NOT_ASSERTED) where nothing is detectable or the bar would be under 8 * noise.  No bar comes from a kernel's output.
The replay must pass every bar and every share (tests/test_gated_cases_cpu.py): the check that the reference alone stays inside them.

Mutants that are provably the reference in a case are left out there (a wider stride where the buffer is dense, a dropped tail beyond
the case's size, the STE term with ste = 0, a chunk permutation at W = 128).  The two large qknorm shapes carry only the mutants tied to size
and position (their float64 evaluation costs seconds each); every other mutant is caught at the small shapes."""
import functools
import math

import numpy as np
import torch

from tests.test_rows_edges_gpu import _sum_bound

DETECT = 32.0
SHARE = 0.01
INF = float("inf")
POISON16, POISON32 = 0x4B4B, 0x4B4B4B4B
P16 = float(torch.tensor([POISON16], dtype=torch.int16).view(torch.bfloat16))
EPS_LN = float(np.float32(1e-5))
TAIL = 3                      # rows behind every tensor: it is a view of a larger allocation


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def b16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ident(t):
    return t


def _bf(shape, g, std=1.0):
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16)


class Q:
    def __init__(self, cands, bar, tight=None, col=False, exact=False):
        self.cands = cands if isinstance(cands, (list, tuple)) else [cands]
        self.bar, self.tight, self.col, self.exact = bar, tight, col, exact

    @property
    def want(self):
        return self.cands[0]

    def dist(self, got):
        got = got.double()
        if self.exact:
            got = b16(got)
        best = None
        for w in self.cands:
            d = (got - w).abs()
            d = torch.where((torch.isnan(got) & torch.isnan(w)) | (got == w), torch.zeros_like(d), d)
            d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
            best = d if best is None else torch.minimum(best, d)
        return best

    def ratio(self, got):
        """None for a column sum that is not asserted"""
        if self.bar is None:
            return None
        d = self.dist(got)
        bar = self.bar if torch.is_tensor(self.bar) else torch.full_like(d, float(self.bar))
        r = torch.where(d == 0, torch.zeros_like(d), d / bar)
        return float(r.max())

    def share(self, got):
        """share of the elements that need more than the tight bar"""
        if self.tight is None:
            return 0.0
        return float((self.dist(got) > self.tight).double().mean())


def _either(v, reach):
    """the bf16 roundings of v - reach and v + reach: equal unless v lies within reach of a rounding boundary"""
    return b16(v - reach), b16(v + reach)


def _buf(rows, cols, fill=P16):
    return torch.full((rows, cols), fill, dtype=torch.float64)


class Case:
    kernel = ""
    name = ""

    def mutant_names(self):
        return []


# ---------------------------------------------------------------------------------------------------------------- qknorm_rope
QK_SHAPES = [(1, 1, 1), (3, 7, 5), (2, 100, 3), (2, 513, 16), (5, 1100, 12)]
QK_COLS = ("dq_w", "dq_b", "dk_w", "dk_b")
QK_SIZE_MUTANTS = ("pos_row", "pos_next", "v_not_copied", "gate_written", "drop_last", "drop_last32", "drop_ge16384", "drop_ge65536")
QK_ALL_MUTANTS = ("pos_row", "pos_next", "swap_qk_params", "lane_plus_1", "head_plus_1", "unbiased_var", "no_eps", "half_split", "unconj_bwd",
                  "v_not_copied", "gate_written", "drop_last", "drop_last32", "drop_ge16384", "drop_ge65536")


def rope_tables(n):
    """the project's own rotary tables at positions that differ in every row and axis"""
    from video_tokenizer_amd.titok import rope_tables_from_positions
    r = np.arange(n, dtype=np.float64)
    return rope_tables_from_positions(np.stack([r, r // 3, r % 5], axis=1))


class QKCase(Case):
    kernel = "qknorm_rope"

    def __init__(self, B, L, H, const=False):
        g = _gen(7000 + 100 * L + 10 * H + B + const)
        self.B, self.L, self.H, self.const = B, L, H, const
        self.M, self.D = B * L, 64 * H
        M, D = self.M, self.D
        back = _bf((M + TAIL, 4 * D), g, 1.5)
        self.special = {}
        if const:
            x = back[:M].reshape(M, 4, H, 64)
            nv = M * H
            for i, vec in enumerate((0, 5, 20, 7, 33, nv - 1)):
                x[vec // H, :2, vec % H] = 1.5 if i < 3 else -0.75
                self.special[vec] = "const"
            for vec in (2, 11, 40):
                x[vec // H, :2, vec % H] = (1.0 + 2.0 ** -7 * torch.randint(0, 2, (2, 64), generator=g)).to(torch.bfloat16)
                self.special[vec] = "spread"
        back[:M, 3 * D:] = float("nan")          # the gate columns are no operand of this pass
        back[M:] = float("nan")
        self.backing = back
        up = _bf((M + TAIL, 3 * D), g)
        up[M - 1] *= 4                            # the last vectors: loud enough to show in the parameter sums when dropped
        up[M:] = float("nan")
        self.up_backing = up
        n = torch.arange(64, dtype=torch.float32)
        self.params = [1 + 0.1 * n, 0.1 * n, 1 + 0.1 * (63 - n), 0.1 * (n - 32)]       # q_w, q_b, k_w, k_b
        self.cos_ext, self.sin_ext = rope_tables(M + 1)                                # rows [0, L) are the kernel's table
        self.eps = EPS_LN

    @property
    def qkvg(self):
        return self.backing[: self.M]

    @property
    def up(self):
        return self.up_backing[: self.M]

    def mutant_names(self):
        names = QK_SIZE_MUTANTS if self.M * self.H > 4096 else QK_ALL_MUTANTS
        nv = self.M * self.H
        out = []
        for m in names:
            if (m == "pos_row" and self.B == 1) or (m == "pos_next" and self.L == 1):
                continue
            if (m == "drop_ge16384" and nv <= 16384) or (m == "drop_ge65536" and nv <= 65536) or (m == "drop_last32" and nv <= 1):
                continue
            out.append(m)
        return out

    def evaluate(self, dt=torch.float64, rb=b16, mut="", x=None, params=None):
        """everything the two kernels compute, as tensors [2 (q|k), M, H, 64] of dtype dt"""
        M, L, H, D = self.M, self.L, self.H, self.D
        row = self.qkvg.to(dt) if x is None else x
        P = [p.to(dt) for p in self.params] if params is None else list(params)
        if mut == "swap_qk_params":
            P = [P[2], P[3], P[0], P[1]]
        if mut == "lane_plus_1":
            P = [p.roll(-8) for p in P]
        w = torch.stack([P[0], P[2]])[:, None, None, :]
        b = torch.stack([P[1], P[3]])[:, None, None, :]
        off = 64 if mut == "head_plus_1" else 0
        xs = torch.stack([row[:, off + i * D: off + (i + 1) * D].reshape(M, H, 64) for i in (0, 1)])
        mean = xs.mean(-1, keepdim=True)
        xc = xs - mean
        var = (xc * xc).sum(-1, keepdim=True) / (63 if mut == "unbiased_var" else 64)
        rstd = 1.0 / torch.sqrt(var + (0.0 if mut == "no_eps" else self.eps))
        xh = xc * rstd
        n = rb(xh * w + b)
        r = torch.arange(M)
        pos = r if mut == "pos_row" else ((r + 1) % L if mut == "pos_next" else r % L)
        cs = self.cos_ext.to(dt)[pos][None, :, None, :]
        sn = self.sin_ext.to(dt)[pos][None, :, None, :]
        half = mut == "half_split"

        def pairs(t):
            return (t[..., :32], t[..., 32:]) if half else (t[..., 0::2], t[..., 1::2])

        def join(t0, t1):
            return torch.cat([t0, t1], -1) if half else torch.stack([t0, t1], -1).reshape(2, M, H, 64)

        a, bb = pairs(n)
        y = join(a * cs - bb * sn, a * sn + bb * cs)
        mag = join(a.abs() + bb.abs(), a.abs() + bb.abs())
        gy = torch.stack([self.up.to(dt)[:, i * D:(i + 1) * D].reshape(M, H, 64) for i in (0, 1)])
        g0, g1 = pairs(gy)
        sg = -1.0 if mut == "unconj_bwd" else 1.0
        g = join(rb(g0 * cs + sg * g1 * sn), rb(g1 * cs - sg * g0 * sn))
        gw = g * w
        m1 = gw.mean(-1, keepdim=True)
        m2 = (gw * xh).mean(-1, keepdim=True)
        dx = rstd * (gw - m1 - xh * m2)
        S = rstd * (gw.abs() + gw.abs().mean(-1, keepdim=True) + xh.abs() * (gw * xh).abs().mean(-1, keepdim=True))
        kappa = 2.0 ** -22 * xs.abs().amax(-1, keepdim=True) * rstd
        return dict(y=y, mag=mag, dx=dx, S=S, kappa=kappa, tw=g * xh, tb=g, xh=xh, g=g)

    def _assemble(self, e, mut=""):
        """the two output buffers [M + TAIL, 3D] and [M + TAIL, 4D] and the four sums from an evaluation"""
        M, D = self.M, self.D
        out, dq = _buf(M + TAIL, 3 * D), _buf(M + TAIL, 4 * D)
        for i in (0, 1):
            out[:M, i * D:(i + 1) * D] = e["y"][i].reshape(M, D).double()
            dq[:M, i * D:(i + 1) * D] = e["dx"][i].reshape(M, D).double()
        if mut != "v_not_copied":
            out[:M, 2 * D:] = self.qkvg[:, 2 * D:3 * D].double()
            dq[:M, 2 * D:3 * D] = self.up[:, 2 * D:].double()
        if mut == "gate_written":
            dq[:M, 3 * D:] = 0.0
        nv = M * self.H
        keep = torch.ones(nv, dtype=torch.float64)
        first = {"drop_last": nv - 1, "drop_last32": max(nv - 32, 0), "drop_ge16384": 16384, "drop_ge65536": 65536}.get(mut)
        if first is not None:
            keep[first:] = 0.0
        res = {"out": out, "dqkvg": dq}
        for i, nm in enumerate(QK_COLS):
            t = e["tw" if i % 2 == 0 else "tb"][i // 2].reshape(nv, 64).double()
            res[nm] = (t * keep[:, None]).sum(0)
        return res

    def reference(self):
        e = self.evaluate()
        r = self._assemble(e)
        M, D = self.M, self.D

        def region(vals, rows_cols):
            t = torch.zeros_like(rows_cols)
            for i in (0, 1):
                t[:M, i * D:(i + 1) * D] = vals[i].reshape(M, D)
            return t

        want = r["out"]
        mag = region(e["mag"], want)
        fin = region(torch.ones_like(e["mag"]), want) * 2.0 ** -8 * want.abs()
        qs = {"out": Q(want, fin + (2.0 ** -7 + 2.0 ** -20) * mag, fin + 2.0 ** -20 * mag)}
        want = r["dqkvg"]
        S = region(e["S"], want)
        fl = region((2.0 ** -18 + 4 * e["kappa"]).expand_as(e["S"]) * e["S"], want)
        fin = region(torch.ones_like(e["S"]), want) * 2.0 ** -8 * want.abs()
        qs["dqkvg"] = Q(want, fin + fl + 2.0 ** -7 * S, fin + fl)
        nv = M * self.H
        self.col_noise = {}
        for i, nm in enumerate(QK_COLS):
            t = e["tw" if i % 2 == 0 else "tb"][i // 2].reshape(nv, 64)
            tol = float(((2.0 ** -20 + 4 * e["kappa"][i // 2]).expand(M, self.H, 64).reshape(nv, 64) * t.abs()).max()) if i % 2 == 0 else 0.0
            quiet = t[: nv - self.H] if M > 1 else t          # (the loud last row is H vectors in 10^2 .. 10^5: its own flips are not counted)
            noise = _sum_bound(t, tol) + 2.0 ** -6 * float(quiet.abs().max())
            self.col_noise[nm] = max(noise, 2.0 ** -23 * float(r[nm].abs().max()))
            qs[nm] = Q(r[nm], None, col=True)
        self.e = e
        return qs

    def replay(self):
        r = self._assemble(self.evaluate(torch.float32))
        return {k: (v if k in QK_COLS else b16(v)) for k, v in r.items()}

    def mutant(self, m):
        e = self.e if m in ("v_not_copied", "gate_written") or m.startswith("drop_") else self.evaluate(mut=m)
        return self._assemble(e, m)


# ------------------------------------------------------------------------------------------------------ sigmoid_gate and geglu
CAP_UNITS = 4096 * 256
GATE_VALUES = (1.0, -1.0, 3.140625, -3.140625, 2.0 ** -20, 2.0 ** 20)


def _sigma_reach(g, s):
    """reach of an fp32 sigmoid 1 / (1 + E), E = exp2(-x log2 e): the argument's rounding alone moves E by |x| 2^-24 of itself (taken
    twice, plus 4 units for exp2, the sum and the division), and d sigma = sigma (1 - sigma) dE / E; beyond |x| = 128 E is 0 or inf"""
    return s * ((1.0 - s) * (g.abs().clamp(max=128.0) + 4.0) * 2.0 ** -23 + 2.0 ** -23) + 2.0 ** -148


class GateCase(Case):
    """o, dog bf16 [M, D]; the gate is columns [col, col + D) of a bf16 buffer [M, gate_rs]; its gradient goes to columns [dcol, dcol + D)
    of a buffer [M, dgate_rs].  entry 'block': vt_sigmoid_gate_* (the buffers are [M, 4D], col = 3D); 'cols': vt_sigmoid_gate_cols_*"""
    kernel = "sigmoid_gate"

    def __init__(self, entry, M, D, gate_rs=None, col=0, dgate_rs=None, dcol=0, exhaustive=False):
        self.entry, self.M, self.D, self.exhaustive = entry, M, D, exhaustive
        if entry == "block":
            gate_rs, col, dgate_rs, dcol = 4 * D, 3 * D, 4 * D, 3 * D
        self.gate_rs, self.col = gate_rs or D, col
        self.dgate_rs, self.dcol = dgate_rs or self.gate_rs, dcol
        self.kernel = "sigmoid_gate" if entry == "block" else "sigmoid_gate_cols"
        g = _gen(8000 + M + D + self.gate_rs)
        gb = torch.full((M + TAIL, self.gate_rs), float("nan"), dtype=torch.bfloat16)
        if exhaustive:
            assert M * D == 65536
            gate = torch.arange(65536, dtype=torch.int32).to(torch.int16)[torch.randperm(65536, generator=g)].view(torch.bfloat16).reshape(M, D)
            vals = torch.tensor(GATE_VALUES, dtype=torch.float32)
            o = vals[torch.randint(0, 6, (M, D), generator=g)].to(torch.bfloat16)
            dog = vals[torch.randint(0, 6, (M, D), generator=g)].to(torch.bfloat16)
        else:
            gate, o, dog = _bf((M, D), g, 2.0), _bf((M, D), g), _bf((M, D), g)
            if col >= D:
                gb[:M, col - D:col] = _bf((M, D), g, 2.0)          # a neighbour's block: real values, so that reading it is a wrong answer
        gb[:M, col:col + D] = gate
        self.gate_backing = gb
        self.o = torch.cat([o, torch.full((TAIL, D), float("nan"), dtype=torch.bfloat16)])
        self.dog = torch.cat([dog, torch.full((TAIL, D), float("nan"), dtype=torch.bfloat16)])

    def mutant_names(self):
        out = ["sigmoid_unrounded", "dsig_unrounded"]
        if self.col >= self.D:
            out.append("gate_col_minus_D")
        if self.gate_rs != self.D:
            out.append("gate_stride_D")
        if self.dgate_rs != self.gate_rs:
            out.append("dgate_at_gate_rs")
        if self.M * self.D // 8 > CAP_UNITS:
            out.append("cap_dropped")
        return out

    def evaluate(self, dt=torch.float64, rb=b16, mut="", o=None, gate=None):
        M, D = self.M, self.D
        if gate is None:
            if mut == "gate_stride_D":
                flat = self.gate_backing.reshape(-1)[self.col:]
                gate = torch.stack([flat[m * D: m * D + D] for m in range(M)])
            else:
                c = self.col - D if mut == "gate_col_minus_D" else self.col
                gate = self.gate_backing[:M, c:c + D]
            gate = gate.to(dt)
        a = self.o[:M].to(dt) if o is None else o
        dy = self.dog[:M].to(dt)
        s = torch.sigmoid(gate)
        if dt == torch.float64 and rb is b16:
            reach = _sigma_reach(gate, s)
            reach = torch.where(torch.isfinite(gate), reach, torch.zeros_like(reach))
            sA, sB = _either(s, reach)
            # below 2^-126 the fp32 quotient is a denormal, and from -x = 88.73 on E itself is inf: an fp32 evaluation may give 0
            cands = (sA, sB, torch.where(s < 2.0 ** -126, torch.zeros_like(s), sA))
        else:
            cands = (rb(s),) * 3
        res = []
        for sg in cands:
            sf = s if mut == "sigmoid_unrounded" else sg
            sd = s if mut == "dsig_unrounded" else sg
            res.append(dict(og=a * sf, d_o=dy * sg, dgate=rb(dy * a) * ((1.0 - sd) * sd), sg=sg))
        return res, a, dy, gate

    def _assemble(self, r, mut=""):
        M, D = self.M, self.D
        og, d_o = _buf(M + TAIL, D), _buf(M + TAIL, D)
        og[:M], d_o[:M] = r["og"].double(), r["d_o"].double()
        rs = self.gate_rs if mut == "dgate_at_gate_rs" else self.dgate_rs
        n = (M + TAIL) * self.dgate_rs
        flat = torch.full((max(n, self.dcol + M * rs + D),), P16, dtype=torch.float64)     # (a wrong stride may run past the buffer)
        for m in range(M):
            flat[self.dcol + m * rs: self.dcol + m * rs + D] = r["dgate"][m].double()
        db = flat[:n].reshape(M + TAIL, self.dgate_rs)
        if mut == "cap_dropped":
            late = torch.arange(M * D).reshape(M, D) >= CAP_UNITS * 8
            p = torch.full((M, D), P16, dtype=torch.float64)
            og[:M], d_o[:M] = torch.where(late, p, og[:M]), torch.where(late, p, d_o[:M])
            db[:M, self.dcol:self.dcol + D] = torch.where(late, p, db[:M, self.dcol:self.dcol + D])
        return {"og": og, "d_o": d_o, "dgate": db}

    def reference(self):
        (rA, rB, rC), a, dy, gate = self.evaluate()
        A, B, C = self._assemble(rA), self._assemble(rB), self._assemble(rC)
        M, D = self.M, self.D
        self.ambiguous = (rA["sg"] != rB["sg"]) | (rA["sg"] != rC["sg"])
        self.finite = torch.isfinite(gate)
        qs = {}
        for nm in ("og", "d_o", "dgate"):
            if self.exhaustive and nm != "dgate":
                qs[nm] = Q([b16(A[nm]), b16(B[nm]), b16(C[nm])], 0.0, exact=True)
                continue
            want = A[nm]
            reg = torch.zeros_like(want, dtype=torch.bool)
            if nm == "dgate":
                reg[:M, self.dcol:self.dcol + D] = True
            else:
                reg[:M] = True
            fin = torch.where(reg, (2.0 ** -8 + 2.0 ** -20) * torch.maximum(A[nm].abs(), B[nm].abs()) + 2.0 ** -133, torch.zeros_like(want))
            fin = torch.where(torch.isfinite(fin), fin, torch.zeros_like(fin))
            step = torch.zeros_like(want)
            if not self.exhaustive:                 # one bf16 step of the rounded sigmoid, through the factor it multiplies
                k = {"og": a.abs() * rA["sg"], "d_o": dy.abs() * rA["sg"], "dgate": b16(dy * a).abs() * rA["sg"]}[nm] * 2.0 ** -7
                step[reg] = k.reshape(-1)
            qs[nm] = Q([A[nm], B[nm], C[nm]] if self.exhaustive else A[nm], fin + step, fin)
        return qs

    def replay(self):
        (rA, _, _), _, _, _ = self.evaluate(torch.float32)
        return {k: b16(v) for k, v in self._assemble(rA).items()}

    def mutant(self, m):
        (rA, _, _), _, _, _ = self.evaluate(mut=m)
        return self._assemble(rA, m)


SQRT2, SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def gelu(x):
    return x * (0.5 * (1.0 + torch.erf(x / SQRT2)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / SQRT2)) + x * torch.exp(-0.5 * x * x) / SQRT2PI


def gelu_reach(x):
    """the bound form of test_gelu_grad_bits_on_every_bf16_magnitude for gelu': the erf approximation's 1.5e-7 and fp32, as 4e-7"""
    return 4e-7 * x.abs().clamp(min=1.0)


def every_bf16_magnitude(M, K):
    """the generator of tests/test_gemm_gelu_grad_gpu.py (shared, not restated), extended with +-inf"""
    from tests.test_gemm_gelu_grad_gpu import _every_bf16_magnitude_cpu
    vals = _every_bf16_magnitude_cpu(M, K)
    vals[7, :4] = torch.tensor([INF, -INF, INF, -INF], dtype=torch.bfloat16)
    return vals


class GegluCase(Case):
    """h bf16 [M, 2I] = [x | gate]; a bf16 [M, lda]; da bf16 [M, lda] (pad columns NaN); dh bf16 [M, 2I]"""
    kernel = "geglu"

    def __init__(self, M, I, lda, every=False):
        self.M, self.I, self.lda, self.every = M, I, lda, every
        g = _gen(9000 + M + I + lda)
        h = _bf((M + TAIL, 2 * I), g, 1.5)
        da = _bf((M + TAIL, lda), g)
        if every:
            h[:M, I:] = every_bf16_magnitude(M, I)
            h[:M:3, 0:I:4] = 0.0                     # x = 0 against every gelu, the large ones included
            h[7, :4] = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.bfloat16)
        h[M:] = float("nan")
        da[M:] = float("nan")
        da[:, I:] = float("nan")
        self.h, self.da = h, da

    def mutant_names(self):
        out = ["halves_swapped", "gelu_unrounded"]
        if self.lda != self.I:
            out += ["out_stride_I", "da_stride_I"]
        if self.M * self.I // 8 > CAP_UNITS:
            out.append("cap_dropped")
        return out

    def evaluate(self, dt=torch.float64, rb=b16, mut="", h=None):
        M, I = self.M, self.I
        hh = self.h[:M].to(dt) if h is None else h
        x, gt = hh[:, :I], hh[:, I:]
        if mut == "halves_swapped":
            x, gt = gt, x
        if mut == "da_stride_I":
            flat = self.da.reshape(-1)
            dy = torch.stack([flat[m * I: m * I + I] for m in range(M)]).to(dt)
        else:
            dy = self.da[:M, :I].to(dt)
        ge = gelu(gt)
        if dt == torch.float64 and rb is b16:
            reach = 4e-7 * gt.abs() + 2.0 ** -21 * ge.abs()
            reach = torch.where(torch.isfinite(reach), reach, torch.zeros_like(reach))
            gA, gB = _either(ge, reach)
        else:
            gA = gB = rb(ge)
        res = []
        for gr in (gA, gB):
            gf = ge if mut == "gelu_unrounded" else gr
            res.append(dict(a=gf * x, dx=dy * gr, dg=rb(dy * x) * gelu_grad(gt), gr=gr))
        return res, x, gt, dy

    def _assemble(self, r, mut=""):
        M, I = self.M, self.I
        a, dh = _buf(M + TAIL, self.lda), _buf(M + TAIL, 2 * I)
        rs = I if mut == "out_stride_I" else self.lda
        if rs == self.lda:
            a[:M, :I] = r["a"].double()
        else:
            flat = a.reshape(-1)
            for m in range(M):
                flat[m * rs: m * rs + I] = r["a"][m].double()
        dh[:M, :I], dh[:M, I:] = r["dx"].double(), r["dg"].double()
        if mut == "cap_dropped":
            idx = torch.arange(M * I).reshape(M, I) >= CAP_UNITS * 8
            p = torch.full((M, I), P16, dtype=torch.float64)
            a[:M, :I] = torch.where(idx, p, a[:M, :I])
            dh[:M, :I], dh[:M, I:] = torch.where(idx, p, dh[:M, :I]), torch.where(idx, p, dh[:M, I:])
        return {"a": a, "dh": dh}

    def reference(self):
        (rA, rB), x, gt, dy = self.evaluate()
        A, B = self._assemble(rA), self._assemble(rB)
        M, I = self.M, self.I
        self.ambiguous = rA["gr"] != rB["gr"]
        z = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
        # the rounded gelu may be any bf16 value between the two candidates: its allowance is their distance, and one step where they agree
        spread = z((rA["gr"] - rB["gr"]).abs()) + (0.0 if self.every else 2.0 ** -7 * z(rA["gr"]).abs())
        fin = lambda t: z((2.0 ** -8 + 2.0 ** -20) * t.abs() + 2.0 ** -133)
        bar_a, bar_dh = torch.zeros_like(A["a"]), torch.zeros_like(A["dh"])
        bar_a[:M, :I] = fin(torch.maximum(rA["a"].abs(), rB["a"].abs())) + z(x.abs() * spread)
        bar_dh[:M, :I] = fin(torch.maximum(rA["dx"].abs(), rB["dx"].abs())) + z(dy.abs() * spread)
        bar_dh[:M, I:] = fin(rA["dg"]) + z(b16(dy * x).abs() * gelu_reach(gt)) + z(2.0 ** -20 * rA["dg"].abs())
        if self.every:                               # where the rounded gelu is unambiguous the product of two bf16 values has one rounding
            sure = ~self.ambiguous
            qa = Q([torch.where(torch.nn.functional.pad(sure, (0, self.lda - I, 0, TAIL), value=True), b16(A["a"]), A["a"]), B["a"]],
                   torch.where(torch.nn.functional.pad(sure, (0, self.lda - I, 0, TAIL), value=True), torch.zeros_like(bar_a), bar_a))
            sure2 = torch.nn.functional.pad(sure, (0, I, 0, TAIL), value=False)
            sure2[M:] = True
            qd = Q([torch.where(sure2, b16(A["dh"]), A["dh"]), B["dh"]], torch.where(sure2, torch.zeros_like(bar_dh), bar_dh))
            return {"a": qa, "dh": qd}
        t_a, t_dh = bar_a.clone(), bar_dh.clone()
        t_a[:M, :I] -= z(x.abs() * 2.0 ** -7 * z(rA["gr"]).abs())
        t_dh[:M, :I] -= z(dy.abs() * 2.0 ** -7 * z(rA["gr"]).abs())
        return {"a": Q(A["a"], bar_a, t_a), "dh": Q(A["dh"], bar_dh, t_dh)}

    def replay(self):
        (rA, _), _, _, _ = self.evaluate(torch.float32)
        return {k: b16(v) for k, v in self._assemble(rA).items()}

    def mutant(self, m):
        (rA, _), _, _, _ = self.evaluate(mut=m)
        return self._assemble(rA, m)


# ------------------------------------------------------------------------------------------------------------------- stat_gate
THRESHOLD, ONES, FORCED = 1, 2, 3
STAT_LEVELS = ([5], [8, 8, 8, 5, 5, 5], [2] * 16, [3, 2] * 4)
STAT_COLS = ("dw2", "db2")


class Fsq:
    """vt_fsq_device.h in torch: fp32 constants and operation order (the power proofs need a CPU FSQ; the GPU test compares the gate's codes
    with vt_fsq_forward / _backward bit for bit)"""

    def __init__(self, levels):
        f = np.float32
        lv = np.array(levels)
        self.d = len(levels)
        self.half_l = torch.tensor([f(f(l - 1) * f(1.0 + 1e-3)) / f(2.0) for l in levels], dtype=torch.float32)
        self.offset = torch.tensor([0.5 if l % 2 == 0 else 0.0 for l in levels], dtype=torch.float32)
        self.shift = torch.atanh((self.offset / self.half_l).double()).float()
        self.hw = torch.tensor([float(l // 2) for l in levels], dtype=torch.float32)
        self.basis = torch.tensor(np.concatenate([[1], np.cumprod(lv)[:-1]]), dtype=torch.float32)

    def tanh(self, z32):
        return torch.tanh((z32 + self.shift).double()).float()

    def codes(self, z32):
        return torch.round(self.tanh(z32) * self.half_l - self.offset) / self.hw

    def index(self, codes):
        return ((codes * self.hw + self.hw) * self.basis).sum(-1)

    def grad(self, z32, dcodes, dt=torch.float64, pure=False):
        """pure: no fp32 rounding of the argument or of tanh (the autograd comparison)"""
        t = torch.tanh(z32.double() + self.shift.double()) if pure else self.tanh(z32).to(dt)
        return (dcodes.to(dt) / self.hw.to(dt) * self.half_l.to(dt)) * (1.0 - t * t)


class StatCase(Case):
    kernel = "stat_gate"

    def __init__(self, W, M, pad, lv, mode, z=True, idx=True, dprobs=True, dmask=True, ste=1):
        self.W, self.M, self.ld, self.levels, self.mode = W, M, W + pad, list(STAT_LEVELS[lv]), mode
        self.has_z, self.has_idx, self.has_dprobs, self.has_dmask, self.ste = z, idx, dprobs, dmask, ste
        self.d = len(self.levels)
        g = _gen(11000 + W + M + pad + lv)
        # no cancellation in the dot product: |g| with one sign per row against positive weights, so that the logit is as large as the
        # sum of the magnitudes and an fp32 sum lies within reach of a bf16 boundary of it on well under 2 % of the rows
        sign = torch.randint(0, 2, (M, 1), generator=g) * 2.0 - 1.0
        size = 0.1 + 1.9 * torch.rand((M, 1), generator=g)
        gb = torch.full((M + TAIL, self.ld), float("nan"), dtype=torch.bfloat16)
        gb[:M, :W] = (torch.randn((M, W), generator=g).abs() * sign * size).to(torch.bfloat16)
        ub = torch.full((M + TAIL, self.ld), float("nan"), dtype=torch.bfloat16)
        ub[:M, :W] = _bf((M, W), g, 1.5)
        self.g_backing, self.u_backing = gb, ub
        self.w2 = (0.5 + torch.rand(W, generator=g)) * (1.25 / W)
        self.b2 = torch.tensor([0.0625])
        self.z = torch.randn((M, self.d), generator=g) * 1.5
        self.mask_in = torch.randint(0, 2, (M,), generator=g).float()
        self.dcodes = torch.randn((M, self.d), generator=g)
        self.dprobs = torch.randn((M,), generator=g)
        self.dmask = torch.randn((M,), generator=g)
        self.dcodes[M - 1] *= 8
        self.dprobs[M - 1] *= 8
        self.fsq = Fsq(self.levels)
        groups = (M + 15) // 16
        per = (groups + 511) // 512 * 16
        self.last_block_first_row = (M - 1) // per * per

    def mutant_names(self):
        out = ["b2_dropped", "logit_unrounded", "p_unrounded", "dp_unrounded", "drop_last_row", "drop_last_group", "drop_last_block"]
        if self.W > 128:
            out.append("w2_chunks_permuted")
        if self.ld != self.W:
            out.append("stride_W")
        if self.has_z:
            if self.d < 16:
                out.append("extra_channel")
            if self.mode != ONES:
                out += ["z_unmasked", "dz_unmasked"]
            if self.ste:
                out.append("no_ste_term")
        if self.ste and self.has_dmask:
            out.append("no_dmask")
        if self.has_dprobs:
            out.append("no_dprobs")
        return out

    def rows(self, backing, mut=""):
        M, W = self.M, self.W
        if mut == "stride_W":
            flat = backing.reshape(-1)
            return torch.stack([flat[m * W: m * W + W] for m in range(M)])
        return backing[:M, :W]

    def w_used(self, mut=""):
        if mut != "w2_chunks_permuted":
            return self.w2
        ch = self.W // 128
        used = torch.empty(self.W // 8, dtype=torch.long)
        for lane in range(16):
            for i in range(ch):
                used[lane + 16 * i] = lane * ch + i
        return self.w2.reshape(-1, 8)[used].reshape(-1)

    def forward(self, dt=torch.float64, rb=b16, mut="", gin=None, w2=None, b2=None):
        g = self.rows(self.g_backing, mut).to(dt) if gin is None else gin
        w = self.w_used(mut).to(dt) if w2 is None else w2
        b = (torch.zeros(1) if mut == "b2_dropped" else self.b2).to(dt) if b2 is None else b2
        logit = g @ w + b
        reach = ((self.W // 16 + 5) * 2.0 ** -24) * (g.abs() @ w.abs() + b.abs()) + 2.0 ** -23 * logit.abs()
        if dt == torch.float64 and rb is b16 and mut != "logit_unrounded":
            ls = _either(logit, reach)
        else:
            ls = (logit if mut == "logit_unrounded" else rb(logit),) * 2
        ps, su, sig_amb = [], [], torch.zeros_like(logit, dtype=torch.bool)
        for l in ls:
            s = torch.sigmoid(l)
            su.append(s)
            if mut == "p_unrounded":
                ps.append(s)
            elif dt == torch.float64 and rb is b16:
                lo, hi = _either(s, 2.0 ** -21 * s)          # an fp32 sigmoid of the bf16 l, within 4 units of a rounding boundary of p
                ps += [lo, hi]
                sig_amb |= lo != hi
            else:
                ps.append(rb(s))
        return dict(logit=logit, ls=ls, ps=ps, s_unrounded=su[0], sig_amb=sig_amb)

    def ambiguity_ok(self):
        """at most 2 % of the rows may accept a second value of probs (either neighbour of l, or of sigma(l)); below 50 rows, where 2 %
        is less than one row, one row may"""
        n = int(self.ambiguous_rows.sum())
        return n <= 0.02 * self.M or (self.M < 50 and n <= 1)

    def masks(self, p):
        if self.mode == THRESHOLD:
            return (p > 0.5).to(p.dtype)
        return torch.ones_like(p) if self.mode == ONES else self.mask_in.to(p.dtype)

    def fsq_forward(self, mask, mut=""):
        zm = self.z if mut == "z_unmasked" else self.z * mask.float()[:, None]
        codes = self.fsq.codes(zm)
        idx = self.fsq.index(codes)
        if mut == "extra_channel":                          # lane d reads the next row's first element with channel 0's constants
            nxt = torch.cat([zm[1:, 0], torch.zeros(1)])
            idx = idx + (torch.round(torch.tanh((nxt + self.fsq.shift[0]).double()).float() * self.fsq.half_l[0]) + self.fsq.hw[0]) * float(np.prod(self.levels))
        return codes.double(), idx.double()

    def backward(self, probs, mask, dt=torch.float64, mut="", p_unrounded=None, g=None, pure=False):
        """from the operands the kernel is given: probs and mask fp32 [M]"""
        M, W = self.M, self.W
        p, m = probs.to(dt), mask.to(dt)
        term = torch.zeros(M, dtype=dt)
        dz = None
        absum = torch.zeros(M, dtype=dt)
        if self.has_z:
            dzm = self.fsq.grad(self.z * mask.float()[:, None], self.dcodes, dt, pure)
            dz = dzm if mut == "dz_unmasked" else dzm * m[:, None]
            if mut != "no_ste_term":
                term = (dzm * self.z.to(dt)).sum(-1)
                hl = (self.dcodes.to(dt) / self.fsq.hw.to(dt) * self.fsq.half_l.to(dt)).abs()       # (1 - t^2) of an fp32 t is off by 2^-23 absolute
                absum = ((dzm.abs() + 0.25 * hl) * self.z.to(dt).abs()).sum(-1)
            if mut == "extra_channel":
                term = term + torch.cat([self.z[1:, 0], torch.zeros(1)]).to(dt) * dzm[:, 0]
        dp = torch.zeros(M, dtype=dt)
        if self.ste:
            dp = term + (self.dmask.to(dt) if self.has_dmask and mut != "no_dmask" else 0.0)
            absum = absum + (self.dmask.abs().to(dt) if self.has_dmask else 0.0)
        if self.has_dprobs and mut != "no_dprobs":
            dp = dp + self.dprobs.to(dt)
        if self.has_dprobs:
            absum = absum + self.dprobs.abs().to(dt)
        pp = p_unrounded.to(dt) if mut == "dp_unrounded" else p
        dlogit = dp * pp * (1.0 - pp)
        dl_err = 2.0 ** -20 * absum * (p * (1.0 - p)).abs()
        u = self.rows(self.u_backing, mut).to(dt)
        gg = self.rows(self.g_backing, mut).to(dt) if g is None else g
        w = self.w_used(mut).to(dt)
        gp = gelu_grad(u)
        dU = dlogit[:, None] * w * gp
        bar = 2.0 ** -8 * dU.abs() + (dlogit[:, None] * w).abs() * gelu_reach(u) + dl_err[:, None] * (w * gp).abs() + 2.0 ** -20 * dU.abs()
        keep = torch.ones(M, dtype=dt)
        first = {"drop_last_row": M - 1, "drop_last_group": (M - 1) // 16 * 16, "drop_last_block": self.last_block_first_row}.get(mut)
        if first is not None:
            keep[first:] = 0.0
        terms = dlogit[:, None] * gg
        return dict(dU=dU, dU_bar=bar, dz=dz, dw2=(terms * keep[:, None]).sum(0), db2=(dlogit * keep).sum().reshape(1), terms=terms, dlogit=dlogit,
                    dl_err=dl_err)

    def operands(self):
        """probs and mask handed to the backward: the reference forward's own (first candidate)"""
        f = self.forward()
        p = f["ps"][0].float()
        return p, self.masks(p).float(), f

    def _assemble(self, f, bw, mask, mut=""):
        M, W, d = self.M, self.W, self.d
        dU = _buf(M + TAIL, self.ld)
        dU[:M, :W] = bw["dU"].double()
        res = {"probs": f["ps"][0].double(), "dU": dU, "dw2": bw["dw2"].double(), "db2": bw["db2"].double()}
        if self.has_z:
            codes, idx = self.fsq_forward(mask, mut)
            res.update(codes=codes, dz=bw["dz"].double())
            if self.has_idx:
                res["indices"] = idx
        return res

    def reference(self):
        p, mask, f = self.operands()
        bw = self.backward(p, mask)
        r = self._assemble(f, bw, mask)
        self.f, self.p, self.mask = f, p, mask
        self.ambiguous_rows = (f["ls"][0] != f["ls"][1]) | f["sig_amb"]       # rows that accept more than one value of probs
        M, W = self.M, self.W
        qs = {"probs": Q([c.double() for c in f["ps"]], 0.0)}          # fp32 holding bf16 values: the kernel's own bits are compared
        bar = torch.zeros_like(r["dU"])
        bar[:M, :W] = bw["dU_bar"]
        qs["dU"] = Q(r["dU"], bar)
        if self.has_z:
            qs["codes"] = Q(r["codes"], 0.0)
            if self.has_idx:
                qs["indices"] = Q(r["indices"], 0.0)
            hl = (self.dcodes.double() / self.fsq.hw.double() * self.fsq.half_l.double()).abs()
            qs["dz"] = Q(r["dz"], 2.0 ** -21 * (r["dz"].abs() + hl) + 1e-45)
        self.col_noise = {}
        tol = float((bw["dl_err"][:, None] * self.rows(self.g_backing).double().abs() + 2.0 ** -22 * bw["terms"].abs()).max())
        for nm, t, tl in (("dw2", bw["terms"], tol), ("db2", bw["dlogit"][:, None], float((bw["dl_err"] + 2.0 ** -22 * bw["dlogit"].abs()).max()))):
            self.col_noise[nm] = max(_sum_bound(t, tl), 2.0 ** -23 * float(r[nm].abs().max()))
            qs[nm] = Q(r[nm], None, col=True)
        return qs

    def replay(self):
        f = self.forward(torch.float32)
        bw = self.backward(self.p, self.mask, torch.float32)
        r = self._assemble(f, bw, self.mask)
        r["dU"] = b16(r["dU"])
        return r

    def mutant(self, m):
        f = self.forward(mut=m)
        p = f["ps"][0].float()
        # a forward mutant changes probs (and through THRESHOLD the mask); the backward mutants are judged on the reference's operands
        fwd = m in ("b2_dropped", "logit_unrounded", "p_unrounded", "w2_chunks_permuted", "stride_W")
        bw = self.backward(self.p, self.mask, mut=m, p_unrounded=self.f["s_unrounded"])
        return self._assemble(f, bw, self.masks(p).float() if fwd else self.mask, m)


# ------------------------------------------------------------------------------------------------------------------- the cases
def stat_keys():
    """every value of every axis at least once; every W at M = 33 with each (ld, d) pair; every tail M at W = 128 and 768"""
    keys = []
    for i, W in enumerate(range(128, 1025, 128)):
        keys.append((W, 33, 8 * (i % 2), (i // 2) % 4, (THRESHOLD, FORCED, ONES)[i % 3], True, True, True, True, 1))
    for j, (W, M) in enumerate([(W, M) for W in (128, 768) for M in (1, 15, 17, 8193)]):
        keys.append((W, M, 8 * ((j + 1) % 2), (j + 1) % 4, (FORCED, THRESHOLD, ONES)[j % 3], j != 2, j != 5, j != 3, j != 4, 0 if j in (1, 6) else 1))
    return keys


SPECS = {}


def _add(cls, *a, **k):
    name = "-".join([cls.kernel] + [str(v) for v in a] + [f"{n}{v}" for n, v in k.items()])
    SPECS[name] = (cls, a, k)


for _s in QK_SHAPES:
    _add(QKCase, *_s)
_add(QKCase, 2, 9, 3, const=True)
for _e in ("block", "cols"):
    for _M, _D in ((1, 8), (3, 24), (257, 40)):
        _add(GateCase, _e, _M, _D, gate_rs=None if _e == "block" else _D + 8)
    _add(GateCase, _e, 128, 512, gate_rs=None if _e == "block" else 512, exhaustive=True)
_add(GateCase, "cols", 67, 256, gate_rs=512, col=256, dgate_rs=264)
_add(GateCase, "cols", 4100, 2048, gate_rs=2056)
for _M, _I, _l in ((1, 8, 8), (5, 24, 40), (130, 1376, 1408), (4100, 2048, 2048)):
    _add(GegluCase, _M, _I, _l)
_add(GegluCase, 384, 192, 200, every=True)
for _k in stat_keys():
    _add(StatCase, *_k)


@functools.lru_cache(maxsize=None)
def case(name):
    cls, a, k = SPECS[name]
    c = cls(*a, **k)
    c.name = name
    return c


def names(kernel_prefix):
    return [n for n in SPECS if n.startswith(kernel_prefix + "-")]


# (case, quantity): column sums no mutant of the case moves by DETECT x noise, or whose bar would be under 8 x noise
NOT_ASSERTED = {}
# (case, mutant): not caught by any asserted quantity of that case; every one is caught by another case of its kernel
_ROUND = "a missing intermediate rounding moves the output by less than the final rounding; the case that demands bits on every pattern / magnitude sees it"
_ONE = "one row: no row stride is used, and position 0 rotates by the identity"
_EPS = "eps = 1e-5 against a variance of order 1 moves nothing by a bf16 step: the constant-vector case is there for it"
_FEW = "no logit / p of these few rows lands where the missing rounding changes the rounded p; the larger cases see it"
EXEMPT_MUTANTS = {("qknorm_rope-1-1-1", "unbiased_var"): "64 / 63 of one variance: under the bar of one vector; every other shape sees it",
                  ("qknorm_rope-1-1-1", "half_split"): _ONE, ("qknorm_rope-1-1-1", "unconj_bwd"): _ONE,
                  ("stat_gate-768-1-8-1-1-True-True-True-False-1", "z_unmasked"): "one row, and its mask is 1",
                  ("stat_gate-768-1-8-1-1-True-True-True-False-1", "dz_unmasked"): "one row, and its mask is 1"}
EXEMPT_MUTANTS.update({(n, "no_eps"): _EPS for n in ("qknorm_rope-1-1-1", "qknorm_rope-3-7-5", "qknorm_rope-2-100-3")})
EXEMPT_MUTANTS.update({(n, m): _ROUND for n in SPECS if n.startswith("sigmoid_gate") and "exhaustive" not in n for m in ("sigmoid_unrounded", "dsig_unrounded")})
EXEMPT_MUTANTS.update({(n, "gelu_unrounded"): _ROUND for n in SPECS if n.startswith("geglu") and "every" not in n})
EXEMPT_MUTANTS.update({(n, m): _ONE for n in ("sigmoid_gate-block-1-8-gate_rsNone", "sigmoid_gate-cols-1-8-gate_rs16") for m in ("gate_stride_D",)})
EXEMPT_MUTANTS.update({(n, "stride_W"): _ONE for n in ("stat_gate-128-1-8-1-3-True-True-True-True-1", "stat_gate-768-1-8-1-1-True-True-True-False-1")})
EXEMPT_MUTANTS.update({(n, "logit_unrounded"): _FEW for n in ("stat_gate-128-1-8-1-3-True-True-True-True-1", "stat_gate-128-17-8-3-2-False-True-True-True-1",
                                                              "stat_gate-768-1-8-1-1-True-True-True-False-1", "stat_gate-768-17-8-3-3-True-True-True-True-0")})
EXEMPT_MUTANTS[("stat_gate-128-1-8-1-3-True-True-True-True-1", "dp_unrounded")] = _FEW


class Bars:
    """the reference quantities of one case with every bar in place, and what each mutant does to them"""

    def __init__(self, case):
        self.case = case
        self.q = case.reference()
        self.mut = {m: case.mutant(m) for m in case.mutant_names()}
        self.noise = getattr(case, "col_noise", {})
        self._caught = {}
        for nm, q in self.q.items():
            if not q.col:
                continue
            devs = [float((r[nm] - q.want).abs().max()) for r in self.mut.values()]
            seen = [d for d in devs if d >= DETECT * self.noise[nm]]
            q.bar = min(seen) / 4 if seen and min(seen) / 4 >= 8 * self.noise[nm] else None

    def ratios(self, got):
        return {nm: q.ratio(got[nm]) for nm, q in self.q.items() if nm in got}

    def caught(self, m):
        if m not in self._caught:
            self._caught[m] = any(r is not None and r >= 4.0 for r in self.ratios(self.mut[m]).values())
        return self._caught[m]

    def undetected(self):
        return [m for m in self.mut if not self.caught(m)]


@functools.lru_cache(maxsize=None)
def bars(name):
    return Bars(case(name))
