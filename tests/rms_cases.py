"""Edge cases, float64 references, fp32 replays and reference mutants of the row passes of the three newest model families: the whole-row
RMSNorm (csrc/vt_rmsnorm.h: vt_rmsnorm_*, vt_rmsnorm_any_*, vt_rmsnorm_any_f32_*), the per-head RMSNorm (csrc/vt_cross.hip:
vt_head_rmsnorm_*), the fused q/k RMS-norm + rotary pass and the scaled residual (csrc/vt_design.hip: vt_qkrms_rope_*, vt_residual_scale_*),
the rotary pass of the plain stack (csrc/vt_rope.hip: vt_rope_rotate) and SwiGLU (csrc/vt_ar.hip: vt_swiglu_*).  Plain torch on the CPU: no
GPU and no built library (the rotary tables are the project's own, through tests/gated_cases.rope_tables).  The pattern, the classes Q and
Bars and every constant (DETECT, SHARE, POISON, TAIL) are those of tests/gated_cases.py: read its docstring first.

REFERENCE: the formula of the kernel's header comment in float64 on the exact bf16 / fp32 inputs, rounded to bf16 where the header says a
bf16 tensor is materialised (bf16(x rstd) of the head norm, the normalised q / k before the rotation, the conjugate-rotated gradient before
the norm backward, bf16(silu(g)), bf16(dy x), bf16(scale), bf16(y), bf16(dout)); the final rounding of an output is part of the bar.
REPLAY: the same function in float32.  MUTANT: the reference with one thing miscounted.

Elementwise bar = one final rounding (2^-8 |want| for a bf16 output, nothing for an fp32 one) + one bf16 step (2^-7) of every rounded
intermediate that feeds the element + the fp32 floor:
    FLOOR    2^-20 of the operands' magnitudes (a handful of fp32 operations)
    DOT      2^-18 of sum |x g|: the dot product of the norm backward is a chain of at most dim / 64 fused multiply-adds per lane and a
             six-step butterfly, under 48 roundings of 2^-24 each at the widest row
    RSQ_REL  the relative error of an fp32 rstd (sum of squares, reciprocal square root): see the constant
    silu     the reach of an fp32 x / (1 + exp(-x)): see `silu_reach`
The `tight` bar leaves out the 2^-7 steps; at most SHARE of a case's elements may need more.  Outputs that are exact in fp32 by
construction carry bar 0: the scaled residual (the product of two bf16 values is exact, one rounding, one fp32 addition), the v copies,
everything vt_rope_rotate leaves alone, and everything outside the documented output region (POISON).  Column sums follow the rule of
tests/gated_cases.py (noise = `_sum_bound`, detectable at DETECT x noise, bar = 1/4 of the smallest detectable deviation, NOT_ASSERTED where
nothing is detectable or the bar would be under 8 x noise).  No constant here comes from a kernel's output.

The backward of the whole-row norm is given the reference's own rstd, rounded to fp32 (its saved operand), so that it is judged apart from
the forward.  A large shape carries only the mutants tied to size and position."""
import functools

import torch

from tests.gated_cases import DETECT, P16, POISON32, SHARE, TAIL, Bars, Case, Q, _bf, _buf, _either, _gen, b16, ident, rope_tables    # noqa: F401 (the tests' too)
from tests.test_rows_edges_gpu import _sum_bound

P32 = float(torch.tensor([POISON32], dtype=torch.int32).view(torch.float32))
NAN = float("nan")
FLOOR = 2.0 ** -20
DOT = 2.0 ** -18
# Relative error allowed to an fp32 rstd = rsq(sum x^2 / n + eps).  Obtained from the reference and the replay alone: the largest relative
# distance between the replay's fp32 rstd (torch.float32 sum, division, rsqrt) and the float64 one over every case of this file is
# 1.73e-7 = 1.45 x 2^-23 (tests/test_rms_cases_cpu.py::test_the_derived_floors_keep_their_margin measures it again and holds the margin);
# margin 4 -> 2^-20.  The margin is for v_rsq_f32 (1 ulp) and for a summation order other than torch's.
RSQ_REL = 2.0 ** -20
RSQ_MARGIN = 4.0
# Reach of an fp32 silu and silu', in units of `silu_unit` (below).  The largest distance between the replay's fp32 values (torch.exp in fp32,
# the kernel's formulas) and the float64 ones over the SwiGLU cases is 0.92 unit (the same test measures it again and holds the margin);
# margin 3 for the fast exponential, which is exp2 of a rounded product -> 3 units.
SILU_UNITS = 3.0
SILU_MARGIN = 3.0
SILU_OVERFLOW = -88.75          # bf16 values below it: exp(-x) is past the fp32 range (e^89 > 3.4e38), and x / inf = -0


def _noise(terms, tol, total):
    return max(_sum_bound(terms, tol), 2.0 ** -23 * float(total.abs().max()))


def _flat_rows(backing, M, width, rs, col=0):
    """rows of `width` read at row stride rs from a backing buffer, whatever its own stride is (a wrong stride may run past the end: NaN)"""
    flat = backing.reshape(-1)
    need = col + (M - 1) * rs + width
    if need > flat.numel():
        flat = torch.cat([flat, torch.full((need - flat.numel(),), NAN, dtype=flat.dtype)])
    return torch.stack([flat[col + m * rs: col + m * rs + width] for m in range(M)])


# ---------------------------------------------------------------------------------------------------------------- whole-row RMSNorm
RMS_WIDTHS = (128, 256, 384, 512, 768, 1024, 1280, 1536, 2560)
RMS_FAMILIES = {"rmsnorm": ((384, 768, 1024, 1280, 1536, 2560), True, 1e-5), "rmsnorm_any": (RMS_WIDTHS, True, 1e-6),
                "rmsnorm_any_f32": (RMS_WIDTHS, False, 1e-6)}
RMS_ROWS, RMS_LARGE, RMS_LARGE_WIDTHS = (1, 3, 5, 1029), 8197, (128, 768, 2560)
RMS_SIZE_MUTANTS = ("drop_last", "drop_ge8192", "drop_ge1024_dw", "drop_ge1024_dx")
RMS_ALL_MUTANTS = RMS_SIZE_MUTANTS + ("piece_swap", "mean_over_dim_minus_1", "no_eps", "rstd_squared", "dres_dropped", "dw_without_rstd", "dot_without_w",
                                      "neighbour_width")


class RmsCase(Case):
    """x fp32 [rows, dim] dense; y bf16 or fp32; rstd fp32 [rows]; dy of y's type; dres fp32 or absent; dx fp32, dxb bf16 (bf16 families); dw [dim].
    Row 0 is of magnitude 1e-4, row 1 all zero, row 2 of magnitude 1e4, and row rows - 2 all zero again (past the caps of the large shapes); a
    single row takes one of the three kinds by its width's index"""

    def __init__(self, family, dim, rows):
        self.kernel, self.dim, self.rows = family, dim, rows
        _, self.bf, eps = RMS_FAMILIES[family]
        self.eps = float(torch.tensor(eps, dtype=torch.float32))
        i = RMS_WIDTHS.index(dim)
        self.has_dres = self.bf and (i + RMS_ROWS.index(rows) if rows in RMS_ROWS else i) % 2 == 0
        g = _gen(20000 + dim + rows)                      # the same data for the three families
        T = rows + TAIL
        x = torch.randn((T, dim), generator=g) * 1.5
        kinds = {0: 1e-4, 1: 0.0, 2: 1e4}
        if rows == 1:
            x[0] *= kinds[i % 3]
        else:
            for r, k in kinds.items():
                if r < rows:
                    x[r] *= k
            if rows >= 5:
                x[rows - 2] = 0.0
        dy = torch.randn((T, dim), generator=g)
        dy[rows - 1] *= 4                                 # the last row: loud enough to show in dw when dropped
        if self.bf:
            dy = dy.to(torch.bfloat16)
        dres = torch.randn((T, dim), generator=g)
        x[rows:], dy[rows:], dres[rows:] = NAN, NAN, NAN
        self.x, self.dy, self.dres = x, dy, dres if self.has_dres else None
        self.w = 0.5 + torch.rand(dim, generator=g)
        xs = x[:rows].double()
        self.rstd_in = torch.full((T,), NAN)
        self.rstd_in[:rows] = (1.0 / torch.sqrt((xs * xs).sum(-1) / dim + self.eps)).float()

    def mutant_names(self):
        J = self.dim // 128
        out = []
        for m in (RMS_SIZE_MUTANTS if self.rows > 4096 else RMS_ALL_MUTANTS):
            if (m == "drop_ge8192" and self.rows <= 8192) or (m.startswith("drop_ge1024") and self.rows <= 1024):
                continue
            if (m == "piece_swap" and J == 1) or (m == "dres_dropped" and not self.has_dres):
                continue
            out.append(m)
        return out

    def evaluate(self, dt=torch.float64, mut="", x=None, w=None, pure=False):
        rows, dim = self.rows, self.dim
        xs = self.x[:rows].to(dt) if x is None else x
        wv = self.w.to(dt) if w is None else w
        if mut == "piece_swap":
            J = dim // 128
            wv = wv.reshape(J, 128)[[1, 0] + list(range(2, J))].reshape(dim)
        nxt = RMS_WIDTHS[(RMS_WIDTHS.index(dim) + 1) % len(RMS_WIDTHS)]
        div = {"mean_over_dim_minus_1": dim - 1, "neighbour_width": nxt}.get(mut, dim)
        rstd = 1.0 / torch.sqrt((xs * xs).sum(-1, keepdim=True) / div + (0.0 if mut == "no_eps" else self.eps))
        y = xs * rstd * wv
        ri = rstd if pure else self.rstd_in[:rows, None].to(dt)
        dy = self.dy[:rows].to(dt)
        g = dy * wv
        dot = (xs * (dy if mut == "dot_without_w" else g)).sum(-1, keepdim=True)
        k = dot * (ri * ri if mut == "rstd_squared" else ri * ri * ri) / (nxt if mut == "neighbour_width" else dim)
        dx = g * ri - xs * k
        S = ri * g.abs() + xs.abs() * ri * ri * ri / dim * (xs * g).abs().sum(-1, keepdim=True)
        if self.has_dres and mut != "dres_dropped":
            dx = dx + self.dres[:rows].to(dt)
        if self.has_dres:
            S = S + self.dres[:rows].to(dt).abs()
        terms = dy * xs * (1.0 if mut == "dw_without_rstd" else ri)
        return dict(y=y, rstd=rstd[:, 0], dx=dx, S=S, terms=terms)

    def _assemble(self, e, mut=""):
        rows, dim, T = self.rows, self.dim, self.rows + TAIL
        y, rstd, dx = _buf(T, dim, P16 if self.bf else P32), torch.full((T,), P32, dtype=torch.float64), _buf(T, dim, P32)
        y[:rows], rstd[:rows], dx[:rows] = e["y"].double(), e["rstd"].double(), e["dx"].double()
        first = {"drop_last": rows - 1, "drop_ge8192": 8192}.get(mut)
        if first is not None:
            y[first:rows], rstd[first:rows] = P16 if self.bf else P32, P32
        first = {"drop_last": rows - 1, "drop_ge1024_dx": 1024}.get(mut)
        if first is not None:
            dx[first:rows] = P32
        keep = torch.ones(rows, dtype=torch.float64)
        first = {"drop_last": rows - 1, "drop_ge1024_dw": 1024}.get(mut)
        if first is not None:
            keep[first:] = 0.0
        res = {"y": y, "rstd": rstd, "dx": dx, "dw": (e["terms"].double() * keep[:, None]).sum(0)}
        if self.bf:
            res["dxb"] = torch.where(dx == P32, torch.full_like(dx, P16), dx)
        return res

    def reference(self):
        e = self.evaluate()
        r = self._assemble(e)
        rows = self.rows

        def region(v):
            t = torch.zeros_like(r["y"])
            t[:rows] = v
            return t

        fin = 2.0 ** -8 * region(e["y"].abs())
        fl = (FLOOR + RSQ_REL) * region(e["y"].abs())
        qs = {"y": Q(r["y"], (fin if self.bf else 0.0) + fl)}
        rb = torch.zeros_like(r["rstd"])
        rb[:rows] = RSQ_REL * e["rstd"]
        qs["rstd"] = Q(r["rstd"], rb)
        fl = DOT * region(e["S"])
        qs["dx"] = Q(r["dx"], fl)
        if self.bf:
            qs["dxb"] = Q(r["dxb"], fl + 2.0 ** -8 * region(e["dx"].abs()))
        self.col_noise = {"dw": _noise(e["terms"], 2.0 ** -22 * float(e["terms"].abs().max()), r["dw"])}
        qs["dw"] = Q(r["dw"], None, col=True)
        self.e = e
        return qs

    def replay(self):
        r = self._assemble(self.evaluate(torch.float32))
        if self.bf:
            r["y"], r["dxb"] = b16(r["y"]), b16(r["dxb"])
        return r

    def mutant(self, m):
        return self._assemble(self.e if m.startswith("drop_") else self.evaluate(mut=m), m)

    def rstd_distance(self):
        """largest relative distance of the replay's rstd from the reference's"""
        a, b = self.evaluate(torch.float32)["rstd"].double(), self.e["rstd"]
        return float(((a - b).abs() / b).max())


# ------------------------------------------------------------------------------------------------------------------ per-head RMSNorm
HEAD_SHAPES = [(1, 1), (7, 3), (67, 8), (2049, 8), (8193, 8)]
HEAD_SIZE_MUTANTS = ("drop_last", "drop_last32", "drop_ge16384", "drop_ge65536")
HEAD_ALL_MUTANTS = HEAD_SIZE_MUTANTS + ("lane_plus_1", "head_plus_1", "no_eps", "mean_over_63", "w_of_other_lane", "stride_of_x_for_dy")
EPS_HEAD = float(torch.tensor(1e-6, dtype=torch.float32))


def _drop_first(mut, nv):
    return {"drop_last": nv - 1, "drop_last32": max(nv - 32, 0), "drop_ge16384": 16384, "drop_ge65536": 65536}.get(mut)


def _size_mutants(names, nv):
    return [m for m in names if not ((m == "drop_ge16384" and nv <= 16384) or (m == "drop_ge65536" and nv <= 65536) or (m == "drop_last32" and nv <= 1))]


def _head_vectors(g, M, H, cols):
    """bf16 [M + TAIL, cols]: head vectors of std 1.5 in columns [0, 64 H), one all-zero vector, one of 1e-3 and one of 1e3 (from 4 vectors
    on); NaN elsewhere"""
    t = torch.full((M + TAIL, cols), NAN, dtype=torch.bfloat16)
    v = _bf((M, H, 64), g, 1.5)
    nv = M * H
    for vec, k in ((nv // 2, 0.0), (nv // 3, 1e-3), (nv - 1, 1e3)) if nv >= 4 else ():
        v[vec // H, vec % H] = (v[vec // H, vec % H].float() * k).to(torch.bfloat16)
    t[:M, :64 * H] = v.reshape(M, 64 * H)
    return t


class HeadCase(Case):
    """x, y, dy, dx bf16 [M, 64 H] with a row stride each (rows + TAIL rows each); w / dw fp32 [64]"""
    kernel = "head_rmsnorm"

    def __init__(self, M, H):
        self.M, self.H, self.eps = M, H, EPS_HEAD
        W = 64 * H
        self.x_rs, self.y_rs, self.dy_rs, self.dx_rs = W + 72, W + 8, W + 16, W + 24
        g = _gen(22000 + M + H)
        self.x = _head_vectors(g, M, H, self.x_rs)
        dy = torch.full((M + TAIL, self.dy_rs), NAN, dtype=torch.bfloat16)
        dy[:M, :W] = _bf((M, W), g)
        dy[M - 1, :W] *= 4
        self.dy = dy
        n = torch.arange(64, dtype=torch.float32)
        self.w = 1 + 0.1 * n - 0.004 * n * n

    def mutant_names(self):
        nv = self.M * self.H
        return _size_mutants(HEAD_SIZE_MUTANTS if nv > 4096 else HEAD_ALL_MUTANTS, nv)

    def evaluate(self, dt=torch.float64, rb=b16, mut="", x=None, w=None):
        M, H, W = self.M, self.H, 64 * self.H
        off = 64 if mut == "head_plus_1" else 0
        xs = (self.x[:M, off:off + W].to(dt) if x is None else x).reshape(M, H, 64)
        if mut == "lane_plus_1":
            xs = xs.roll(-8, -1)
        wv = self.w.to(dt) if w is None else w
        if mut == "w_of_other_lane":
            wv = wv.roll(-8)
        rstd = 1.0 / torch.sqrt((xs * xs).sum(-1, keepdim=True) / (63 if mut == "mean_over_63" else 64) + (0.0 if mut == "no_eps" else self.eps))
        n = rb(xs * rstd)
        dy = (_flat_rows(self.dy, M, W, self.x_rs) if mut == "stride_of_x_for_dy" else self.dy[:M, :W]).to(dt).reshape(M, H, 64)
        g = dy * wv
        k = (xs * g).sum(-1, keepdim=True) * rstd * rstd * rstd / 64
        S = rstd * g.abs() + xs.abs() * rstd * rstd * rstd / 64 * (xs * g).abs().sum(-1, keepdim=True)
        return dict(y=n * wv, n=n, dx=g * rstd - xs * k, S=S, terms=dy * xs * rstd, rstd=rstd)

    def _assemble(self, e, mut=""):
        M, H, W = self.M, self.H, 64 * self.H
        nv = M * H
        y, dx = _buf(M + TAIL, self.y_rs), _buf(M + TAIL, self.dx_rs)
        keep = torch.ones(nv, dtype=torch.float64)
        first = _drop_first(mut, nv)
        if first is not None:
            keep[first:] = 0.0
        gone = (keep == 0).reshape(M, H, 1).expand(M, H, 64).reshape(M, W)
        p = torch.full((M, W), P16, dtype=torch.float64)
        y[:M, :W] = torch.where(gone & (mut != "drop_ge16384"), p, e["y"].reshape(M, W).double())
        dx[:M, :W] = torch.where(gone & (mut != "drop_ge65536"), p, e["dx"].reshape(M, W).double())
        if mut == "drop_ge65536":
            keep[:] = 1.0
        return {"y": y, "dx": dx, "dw": (e["terms"].reshape(nv, 64).double() * keep[:, None]).sum(0)}

    def reference(self):
        e = self.evaluate()
        r = self._assemble(e)
        M, W = self.M, 64 * self.H

        def region(v, like):
            t = torch.zeros_like(like)
            t[:M, :W] = v.reshape(M, W)
            return t

        ay = e["y"].abs()
        tight = region((2.0 ** -8 + FLOOR + RSQ_REL) * ay, r["y"])
        qs = {"y": Q(r["y"], tight + region(2.0 ** -7 * ay, r["y"]), tight)}
        qs["dx"] = Q(r["dx"], region(2.0 ** -8 * e["dx"].abs() + (DOT + 3 * RSQ_REL) * e["S"], r["dx"]))
        t = e["terms"].reshape(-1, 64)
        self.col_noise = {"dw": _noise(t, (2.0 ** -22 + RSQ_REL) * float(t.abs().max()), r["dw"])}
        qs["dw"] = Q(r["dw"], None, col=True)
        self.e = e
        return qs

    def replay(self):
        r = self._assemble(self.evaluate(torch.float32))
        return {k: (v if k == "dw" else b16(v)) for k, v in r.items()}

    def mutant(self, m):
        return self._assemble(self.e if m.startswith("drop_") else self.evaluate(mut=m), m)

    def rstd_distance(self):
        a, b = self.evaluate(torch.float32)["rstd"].double(), self.e["rstd"]
        return float(((a - b).abs() / b).max())


# ---------------------------------------------------------------------------------------------------------------------- qkrms_rope
QKR_SHAPES = [(1, 1, 1), (3, 7, 5), (2, 100, 3), (2, 1025, 8), (5, 1640, 8)]
QKR_COLS = ("dq_w", "dk_w")
QKR_SIZE_MUTANTS = ("pos_row", "pos_next", "v_not_copied", "gate_written", "drop_last", "drop_last32", "drop_ge16384", "drop_ge65536")
QKR_ALL_MUTANTS = QKR_SIZE_MUTANTS + ("swap_qk_params", "lane_plus_1", "head_plus_1", "no_eps", "half_split", "unconj_bwd")


class QkrCase(Case):
    """qkvg bf16 [M, 4D] at row stride in_rs (columns q | k | v | gate, the gate NaN); out bf16 [M, 3D] at row stride out_rs; dqkv bf16 [M, 3D]
    dense; dqkvg bf16 [M, 4D] at row stride dq_rs, of which columns [0, 3D) are written; dq_w, dk_w fp32 [64]"""
    kernel = "qkrms_rope"

    def __init__(self, B, L, H):
        self.B, self.L, self.H, self.eps = B, L, H, EPS_HEAD
        self.M, self.D = B * L, 64 * H
        M, D = self.M, self.D
        self.in_rs, self.out_rs, self.dq_rs = 4 * D + 16, 3 * D + 8, 4 * D + 8
        g = _gen(23000 + 100 * L + 10 * H + B)
        back = torch.full((M + TAIL, self.in_rs), NAN, dtype=torch.bfloat16)
        back[:, :2 * D] = _head_vectors(g, M, 2 * H, 2 * D)
        back[:M, 2 * D:3 * D] = _bf((M, D), g)
        self.backing = back
        up = _bf((M + TAIL, 3 * D), g)
        up[M - 1] *= 4
        up[M:] = NAN
        self.up_backing = up
        n = torch.arange(64, dtype=torch.float32)
        self.params = [1 + 0.1 * n - 0.004 * n * n, 0.5 + 0.05 * (63 - n)]                # q_w, k_w
        self.cos_ext, self.sin_ext = rope_tables(M + 1)                                    # rows [0, L) are the kernel's table

    def mutant_names(self):
        nv = self.M * self.H
        out = []
        for m in _size_mutants(QKR_SIZE_MUTANTS if nv > 4096 else QKR_ALL_MUTANTS, nv):
            if (m == "pos_row" and self.B == 1) or (m == "pos_next" and self.L == 1):
                continue
            out.append(m)
        return out

    def evaluate(self, dt=torch.float64, rb=b16, mut="", x=None, params=None):
        """everything the two kernels compute, as tensors [2 (q|k), M, H, 64] of dtype dt"""
        M, L, H, D = self.M, self.L, self.H, self.D
        row = self.backing[:M].to(dt) if x is None else x
        P = [p.to(dt) for p in self.params] if params is None else list(params)
        if mut == "swap_qk_params":
            P = [P[1], P[0]]
        if mut == "lane_plus_1":
            P = [p.roll(-8) for p in P]
        w = torch.stack(P)[:, None, None, :]
        off = 64 if mut == "head_plus_1" else 0
        xs = torch.stack([row[:, off + i * D: off + (i + 1) * D].reshape(M, H, 64) for i in (0, 1)])
        rstd = 1.0 / torch.sqrt((xs * xs).sum(-1, keepdim=True) / 64 + (0.0 if mut == "no_eps" else self.eps))
        xh = xs * rstd
        t = rb(rb(xh) * w)
        r = torch.arange(M)
        pos = r if mut == "pos_row" else ((r + 1) % L if mut == "pos_next" else r % L)
        cs = self.cos_ext.to(dt)[pos][None, :, None, :]
        sn = self.sin_ext.to(dt)[pos][None, :, None, :]
        half = mut == "half_split"

        def pairs(v):
            return (v[..., :32], v[..., 32:]) if half else (v[..., 0::2], v[..., 1::2])

        def join(v0, v1):
            return torch.cat([v0, v1], -1) if half else torch.stack([v0, v1], -1).reshape(2, M, H, 64)

        a, bb = pairs(t)
        y = join(a * cs - bb * sn, a * sn + bb * cs)
        mag = join(a.abs() + bb.abs(), a.abs() + bb.abs())
        gy = torch.stack([self.up_backing[:M].to(dt)[:, i * D:(i + 1) * D].reshape(M, H, 64) for i in (0, 1)])
        g0, g1 = pairs(gy)
        sg = -1.0 if mut == "unconj_bwd" else 1.0
        gr = join(rb(g0 * cs + sg * g1 * sn), rb(g1 * cs - sg * g0 * sn))
        gw = gr * w
        k = (xs * gw).sum(-1, keepdim=True) * rstd * rstd * rstd / 64
        S = rstd * gw.abs() + xs.abs() * rstd * rstd * rstd / 64 * (xs * gw).abs().sum(-1, keepdim=True)
        return dict(y=y, mag=mag, dx=gw * rstd - xs * k, S=S, terms=gr * xh, rstd=rstd)

    def _assemble(self, e, mut=""):
        M, D, H = self.M, self.D, self.H
        nv = M * H
        out, dq = _buf(M + TAIL, self.out_rs), _buf(M + TAIL, self.dq_rs)
        keep = torch.ones(nv, dtype=torch.float64)
        first = _drop_first(mut, nv)
        if first is not None:
            keep[first:] = 0.0
        gone = (keep == 0).reshape(M, H, 1).expand(M, H, 64).reshape(M, D)
        p = torch.full((M, D), P16, dtype=torch.float64)
        v, dv = self.backing[:M, 2 * D:3 * D].double(), self.up_backing[:M, 2 * D:].double()
        for i in (0, 1):
            out[:M, i * D:(i + 1) * D] = torch.where(gone & (mut != "drop_ge16384"), p, e["y"][i].reshape(M, D).double())
            dq[:M, i * D:(i + 1) * D] = torch.where(gone & (mut != "drop_ge65536"), p, e["dx"][i].reshape(M, D).double())
        if mut != "v_not_copied":
            out[:M, 2 * D:3 * D] = torch.where(gone & (mut != "drop_ge16384"), p, v)
            dq[:M, 2 * D:3 * D] = torch.where(gone & (mut != "drop_ge65536"), p, dv)
        if mut == "gate_written":
            dq[:M, 3 * D:4 * D] = 0.0
        if mut == "drop_ge65536":
            keep[:] = 1.0
        res = {"out": out, "dqkvg": dq}
        for i, nm in enumerate(QKR_COLS):
            res[nm] = (e["terms"][i].reshape(nv, 64).double() * keep[:, None]).sum(0)
        return res

    def reference(self):
        e = self.evaluate()
        r = self._assemble(e)
        M, D = self.M, self.D

        def region(vals, like):
            t = torch.zeros_like(like)
            for i in (0, 1):
                t[:M, i * D:(i + 1) * D] = vals[i].reshape(M, D)
            return t

        tight = region(2.0 ** -8 * e["y"].abs() + (FLOOR + RSQ_REL) * e["mag"], r["out"])
        qs = {"out": Q(r["out"], tight + region(2 * 2.0 ** -7 * e["mag"], r["out"]), tight)}     # two rounded intermediates: bf16(x rstd), then t
        tight = region(2.0 ** -8 * e["dx"].abs() + (DOT + 3 * RSQ_REL) * e["S"], r["dqkvg"])
        qs["dqkvg"] = Q(r["dqkvg"], tight + region(2.0 ** -7 * e["S"], r["dqkvg"]), tight)
        self.col_noise = {}
        nv = M * self.H
        for i, nm in enumerate(QKR_COLS):
            t = e["terms"][i].reshape(nv, 64)
            quiet = t[: nv - self.H] if M > 1 else t       # two flipped roundings of the rotated gradient outside the loud last row
            self.col_noise[nm] = max(_sum_bound(t, (2.0 ** -22 + RSQ_REL) * float(t.abs().max())) + 2.0 ** -6 * float(quiet.abs().max()),
                                     2.0 ** -23 * float(r[nm].abs().max()))
            qs[nm] = Q(r[nm], None, col=True)
        self.e = e
        return qs

    def replay(self):
        r = self._assemble(self.evaluate(torch.float32))
        return {k: (v if k in QKR_COLS else b16(v)) for k, v in r.items()}

    def mutant(self, m):
        e = self.e if m in ("v_not_copied", "gate_written") or m.startswith("drop_") else self.evaluate(mut=m)
        return self._assemble(e, m)

    def rstd_distance(self):
        a, b = self.evaluate(torch.float32)["rstd"].double(), self.e["rstd"]
        return float(((a - b).abs() / b).max())


# --------------------------------------------------------------------------------------------------------------------- rope_rotate
ROPE_KEYS = [(37, 7, 3, 0), (37, 7, 3, 1), (23, 23, 5, 0), (23, 5, 5, 1), (4097, 257, 16, 0), (4097, 257, 16, 1), (19, 4, 17, 0), (19, 4, 17, 1),
             (65537, 4099, 1, 0), (65537, 4099, 1, 1)]
ROPE_MUTANTS = ("pos_row", "pos_next", "unconj", "pair_swap", "v_rotated", "drop_pieces_ge256", "drop_rows_ge_cap")


class RopeCase(Case):
    """qkv bf16 [M + TAIL, ld], rotated in place in rows [0, M), columns [0, 128 H); ld = 192 H + 8 (H = 1 at M = 65537: ld = 128, no v).  The
    rest of the buffer holds real values, which must keep their bits"""
    kernel = "rope_rotate"

    def __init__(self, M, L, H, conj):
        self.M, self.L, self.H, self.conj = M, L, H, conj
        self.ld = 128 if M > 65536 else 192 * H + 8
        self.qkv = _bf((M + TAIL, self.ld), _gen(24000 + M + H + conj), 1.5)
        self.cos_ext, self.sin_ext = rope_tables(M + 1)
        tx = min(16 * H, 256)
        self.cap_rows = 4096 * (256 // tx)

    def mutant_names(self):
        out = []
        for m in ROPE_MUTANTS:
            if (m == "pos_row" and self.M <= self.L) or (m == "v_rotated" and self.ld < 192 * self.H) or (m == "drop_pieces_ge256" and self.H <= 16):
                continue
            if m == "drop_rows_ge_cap" and self.M <= self.cap_rows:
                continue
            out.append(m)
        return out

    def evaluate(self, dt=torch.float64, mut="", x=None, conj=None):
        M, L, H = self.M, self.L, self.H
        nh = (3 if mut == "v_rotated" else 2) * H
        x = (self.qkv[:M, :64 * nh].to(dt) if x is None else x).reshape(M, nh, 32, 2)
        r = torch.arange(M)
        pos = r if mut == "pos_row" else ((r + 1) % L if mut == "pos_next" else r % L)
        cs, sn = self.cos_ext.to(dt)[pos][:, None, :], self.sin_ext.to(dt)[pos][:, None, :]
        if (self.conj if conj is None else conj) != (mut == "unconj"):
            sn = -sn
        a, b = (x[..., 1], x[..., 0]) if mut == "pair_swap" else (x[..., 0], x[..., 1])
        y = torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(M, 64 * nh)
        mag = (a.abs() + b.abs())[..., None].expand(M, nh, 32, 2).reshape(M, 64 * nh)
        return y, mag

    def _assemble(self, y, mut=""):
        M = self.M
        out = self.qkv.double().clone()
        src = out[:M, :y.shape[1]].clone()
        if mut == "drop_pieces_ge256":
            y = torch.cat([y[:, :2048], src[:, 2048:]], 1)
        if mut == "drop_rows_ge_cap":
            y = torch.cat([y[:self.cap_rows], src[self.cap_rows:]])
        out[:M, :y.shape[1]] = y.double()
        return {"qkv": out}

    def reference(self):
        y, mag = self.evaluate()
        r = self._assemble(y)
        bar = torch.zeros_like(r["qkv"])
        bar[:self.M, :128 * self.H] = 2.0 ** -8 * y.abs() + FLOOR * mag
        return {"qkv": Q(r["qkv"], bar)}

    def replay(self):
        r = self._assemble(self.evaluate(torch.float32)[0])
        return {"qkv": b16(r["qkv"])}

    def mutant(self, m):
        return self._assemble(self.evaluate(mut=m)[0], m)


# ------------------------------------------------------------------------------------------------------------------ residual_scale
RES_SHAPES = [(1, 4), (3, 340), (1, 1024), (257, 4), (2049, 128), (8193, 512)]
RES_SCALES = (0.3, -0.0123456, -1.7, 0.0031)              # none is a bf16 value
RES_BWD_CAP, RES_FWD_CAP = 256 * 256 * 4, 4096 * 256 * 4
RES_MUTANTS = ("scale_unrounded", "y_unrounded", "g_unrounded", "sum_before_rounding", "drop_last", "drop_ge65536x4", "drop_ge_fwd_cap", "ds_without_y_rounding")


class ResCase(Case):
    """x, y, out, dout, dy fp32 [rows, dim] dense; scale fp32 [1]; dscale fp32 [1].  y and dout are bf16 values times (1 + 2^-10): fp32 values
    that round back to them, so that a missing rounding is a wrong answer; y has dout's sign, so that the terms of dscale do not cancel"""
    kernel = "residual_scale"

    def __init__(self, rows, dim):
        self.rows, self.dim = rows, dim
        g = _gen(25000 + rows + dim)
        T = rows + TAIL
        self.scale = torch.tensor([RES_SCALES[RES_SHAPES.index((rows, dim)) % 4]], dtype=torch.float32)
        sign = torch.randint(0, 2, (T, dim), generator=g) * 2.0 - 1.0
        self.y = (_bf((T, dim), g).float().abs() * sign) * (1 + 2.0 ** -10)
        self.dout = (_bf((T, dim), g).float().abs() * sign) * (1 + 2.0 ** -10)
        self.x = torch.randn((T, dim), generator=g)
        self.x[rows:], self.y[rows:], self.dout[rows:] = NAN, NAN, NAN

    def mutant_names(self):
        n = self.rows * self.dim
        return [m for m in RES_MUTANTS if not ((m == "drop_ge65536x4" and n <= RES_BWD_CAP) or (m == "drop_ge_fwd_cap" and n <= RES_FWD_CAP))]

    def evaluate(self, dt=torch.float64, rb=b16, mut="", y=None, scale=None):
        rows = self.rows
        s = self.scale.to(dt) if scale is None else scale
        sb = s if mut == "scale_unrounded" else rb(s)
        yv = self.y[:rows].to(dt) if y is None else y
        yb = yv if mut == "y_unrounded" else rb(yv)
        prod = sb * yb
        out = self.x[:rows].to(dt) + (prod if mut == "sum_before_rounding" else rb(prod))
        gv = self.dout[:rows].to(dt)
        gb = gv if mut == "g_unrounded" else rb(gv)
        terms = gb * (yv if mut == "ds_without_y_rounding" else rb(yv))
        return dict(out=out if rb is ident else out.float().to(dt), dy=rb(sb * gb), terms=terms.reshape(-1, 1))

    def _assemble(self, e, mut=""):
        rows, dim, T = self.rows, self.dim, self.rows + TAIL
        n = rows * dim
        out, dy = _buf(T, dim, P32), _buf(T, dim, P32)
        out[:rows], dy[:rows] = e["out"].double(), e["dy"].double()
        keep = torch.ones(n, dtype=torch.float64)
        if mut in ("drop_last", "drop_ge_fwd_cap"):
            out[:rows].reshape(-1)[n - 4 if mut == "drop_last" else RES_FWD_CAP:] = P32
        if mut in ("drop_last", "drop_ge65536x4"):
            first = n - 4 if mut == "drop_last" else RES_BWD_CAP
            dy[:rows].reshape(-1)[first:] = P32
            keep[first:] = 0.0
        return {"out": out, "dy": dy, "dscale": (e["terms"].double() * keep[:, None]).sum(0)}

    def reference(self):
        e = self.evaluate()
        r = self._assemble(e)
        # every term is the exact product of two bf16 values: only the sum's order is left to the kernel
        self.col_noise = {"dscale": _noise(e["terms"], 0.0, r["dscale"])}
        self.e = e
        return {"out": Q(r["out"], 0.0), "dy": Q(r["dy"], 0.0), "dscale": Q(r["dscale"], None, col=True)}

    def replay(self):
        return self._assemble(self.evaluate(torch.float32))

    def mutant(self, m):
        return self._assemble(self.e if m.startswith("drop_") else self.evaluate(mut=m), m)


# -------------------------------------------------------------------------------------------------------------------------- swiglu
SWIGLU_SHAPES = [(1, 8), (3, 24), (130, 2048), (4100, 2048)]
SWIGLU_CAP = 4096 * 256
SWIGLU_SIZE_MUTANTS = ("drop_last", "drop_ge1048576")
SWIGLU_MUTANTS = ("halves_swapped", "silu_on_x", "grad_without_x_term", "dx_dg_swapped", "col_plus_8", "drop_last", "drop_ge1048576")


def silu_unit(g, s):
    """one unit of an fp32 sigma(g) = 1 / (1 + E), E = exp(-g), relative to sigma: d sigma / sigma = (1 - sigma) dE / E, dE / E = |g| 2^-24 from
    the argument's rounding (+ 4 for exp itself, the sum and the division), + 2 for the roundings of sigma and of the product -- after `_sigma_reach`
    of tests/gated_cases.py"""
    return ((1.0 - s) * (g.abs().clamp(max=128.0) + 4.0) + 2.0) * 2.0 ** -24


def silu_reach(g, s, units=SILU_UNITS):
    return units * silu_unit(g, s) * (g * s).abs() + 2.0 ** -148


def silu_grad(g):
    s = torch.sigmoid(g)
    return s * (1.0 + g * (1.0 - s))


def silu_grad_reach(g, s, units=SILU_UNITS):
    """s (1 + g (1 - s)) in fp32: s and s (1 - s) to `units` each, and 1 - s an fp32 difference (2^-24 absolute, times g s)"""
    ag = g.abs().clamp(max=128.0)
    flushed = torch.where(s < 2.0 ** -126, silu_grad(g).abs(), torch.zeros_like(s))      # an fp32 sigma under 2^-126 may be 0 (E is inf from g = -89 on)
    return units * (silu_unit(g, s) * (s + ag * s * (1.0 - s)) + ag * s * 2.0 ** -24) + flushed + 2.0 ** -148


class SwigluCase(Case):
    """h bf16 [M, 2I] = [x | g]; a, da bf16 [M, I]; dh bf16 [M, 2I] = [dx | dg].  A third of g is spread over +-90 (silu saturates, exp(-g)
    leaves the fp32 range), a third lies near 0"""
    kernel = "swiglu"

    def __init__(self, M, I):
        self.M, self.I = M, I
        g = _gen(26000 + M + I)
        h = _bf((M + TAIL, 2 * I), g, 1.5)
        kind = torch.randint(0, 3, (M + TAIL, I), generator=g)
        wide = ((torch.rand((M + TAIL, I), generator=g) * 2 - 1) * 90).to(torch.bfloat16)
        gt = torch.where(kind == 0, wide, torch.where(kind == 1, (h[:, I:].float() * 2.0 ** -9).to(torch.bfloat16), h[:, I:]))
        if M * I >= 24:
            gt[0, :8] = torch.tensor([-90.0, -89.0, -88.5, -88.0, 88.0, 90.0, 0.0, -0.0], dtype=torch.bfloat16)
        h[:, I:] = gt
        da = _bf((M + TAIL, I), g)
        h[M:], da[M:] = NAN, NAN
        self.h, self.da = h, da

    def mutant_names(self):
        large = self.M * self.I // 8 > SWIGLU_CAP
        return [m for m in (SWIGLU_SIZE_MUTANTS if large else SWIGLU_MUTANTS)
                if not ((m == "drop_ge1048576" and not large) or (m == "col_plus_8" and self.I == 8))]

    def evaluate(self, dt=torch.float64, rb=b16, mut="", h=None):
        M, I = self.M, self.I
        hh = self.h[:M].to(dt) if h is None else h
        x, gt = hh[:, :I], hh[:, I:]
        if mut == "halves_swapped":
            x, gt = gt, x
        if mut == "col_plus_8":
            gt = gt.roll(-8, 1)
        dy = self.da[:M].to(dt)
        s = torch.sigmoid(gt)
        sv = gt * s
        if dt == torch.float64 and rb is b16:
            reach = torch.where(torch.isfinite(gt), silu_reach(gt, s), torch.zeros_like(gt))
            lo, hi = _either(sv, reach)
            # exp(-g) past the fp32 range: the quotient is -0; a silu under 2^-126 may be flushed
            cands = (lo, hi, torch.where((gt <= SILU_OVERFLOW) | (sv.abs() < 2.0 ** -126), torch.zeros_like(sv), lo))
        else:
            cands = (rb(sv),) * 3
        gp = s if mut == "grad_without_x_term" else s * (1.0 + gt * (1.0 - s))
        res = []
        for sr in cands:
            a = rb(torch.sigmoid(x) * x) * gt if mut == "silu_on_x" else sr * x
            res.append(dict(a=a, dx=dy * sr, dg=rb(dy * x) * gp, sr=sr))
        return res, x, gt, dy, s

    def _assemble(self, r, mut=""):
        M, I = self.M, self.I
        a, dh = _buf(M + TAIL, I), _buf(M + TAIL, 2 * I)
        a[:M] = r["a"].double()
        lo, hi = (r["dg"], r["dx"]) if mut == "dx_dg_swapped" else (r["dx"], r["dg"])
        dh[:M, :I], dh[:M, I:] = lo.double(), hi.double()
        first = {"drop_last": M * I - 8, "drop_ge1048576": SWIGLU_CAP * 8}.get(mut)
        if first is not None:
            gone = torch.arange(M * I).reshape(M, I) >= first
            p = torch.full((M, I), P16, dtype=torch.float64)
            a[:M] = torch.where(gone, p, a[:M])
            dh[:M, :I], dh[:M, I:] = torch.where(gone, p, dh[:M, :I]), torch.where(gone, p, dh[:M, I:])
        return {"a": a, "dh": dh}

    def reference(self):
        (rA, rB, rC), x, gt, dy, s = self.evaluate()
        A, B, C = self._assemble(rA), self._assemble(rB), self._assemble(rC)
        M, I = self.M, self.I
        self.ambiguous = (rA["sr"] != rB["sr"]) | (rA["sr"] != rC["sr"])
        self.rA = rA
        step = 2.0 ** -7 * rA["sr"].abs()                      # one bf16 step of the rounded silu, through the factor it multiplies
        fin = lambda t: (2.0 ** -8 + FLOOR) * t.abs() + 2.0 ** -133
        bar_a, bar_dh = torch.zeros_like(A["a"]), torch.zeros_like(A["dh"])
        bar_a[:M] = fin(torch.maximum(rA["a"].abs(), rB["a"].abs()))
        bar_dh[:M, :I] = fin(torch.maximum(rA["dx"].abs(), rB["dx"].abs()))
        bar_dh[:M, I:] = fin(rA["dg"]) + b16(dy * x).abs() * silu_grad_reach(gt, s)
        t_a, t_dh = bar_a.clone(), bar_dh.clone()
        bar_a[:M] += x.abs() * step
        bar_dh[:M, :I] += dy.abs() * step
        return {"a": Q([A["a"], B["a"], C["a"]], bar_a, t_a), "dh": Q([A["dh"], B["dh"], C["dh"]], bar_dh, t_dh)}

    def replay(self):
        (rA, _, _), _, _, _, _ = self.evaluate(torch.float32)
        return {k: b16(v) for k, v in self._assemble(rA).items()}

    def mutant(self, m):
        if m.startswith("drop_"):
            return self._assemble(self.rA, m)
        (rA, _, _), _, _, _, _ = self.evaluate(mut=m)
        return self._assemble(rA, m)

    def silu_distance(self):
        """largest distance of the replay's fp32 silu and silu' from the float64 ones, in units"""
        g64 = self.h[:self.M, self.I:].double()
        g32 = g64.float()
        ok = g64 > SILU_OVERFLOW
        s64, s32 = torch.sigmoid(g64), 1.0 / (1.0 + torch.exp(-g32))
        d = ((g32 * s32).double() - g64 * s64).abs() / silu_reach(g64, s64, 1.0)
        d2 = ((s32 * (1.0 + g32 * (1.0 - s32))).double() - silu_grad(g64)).abs() / silu_grad_reach(g64, s64, 1.0)
        return float(d[ok].max()), float(d2[ok].max())


# ------------------------------------------------------------------------------------------------------------------- the cases
SPECS = {}


def _add(cls, *a):
    kernel = a[0] if cls is RmsCase else cls.kernel
    SPECS["-".join([kernel] + [str(v) for v in (a[1:] if cls is RmsCase else a)])] = (cls, a)


for _f, (_widths, _, _) in RMS_FAMILIES.items():
    for _d in _widths:
        for _r in RMS_ROWS + ((RMS_LARGE,) if _d in RMS_LARGE_WIDTHS else ()):
            _add(RmsCase, _f, _d, _r)
for _s in HEAD_SHAPES:
    _add(HeadCase, *_s)
for _s in QKR_SHAPES:
    _add(QkrCase, *_s)
for _s in ROPE_KEYS:
    _add(RopeCase, *_s)
for _s in RES_SHAPES:
    _add(ResCase, *_s)
for _s in SWIGLU_SHAPES:
    _add(SwigluCase, *_s)
NAMES = list(SPECS)
KERNELS = list(RMS_FAMILIES) + ["head_rmsnorm", "qkrms_rope", "rope_rotate", "residual_scale", "swiglu"]
ALL_MUTANTS = {"head_rmsnorm": HEAD_ALL_MUTANTS, "qkrms_rope": QKR_ALL_MUTANTS, "rope_rotate": ROPE_MUTANTS, "residual_scale": RES_MUTANTS, "swiglu": SWIGLU_MUTANTS}
ALL_MUTANTS.update({f: tuple(m for m in RMS_ALL_MUTANTS if m != "dres_dropped" or RMS_FAMILIES[f][1]) for f in RMS_FAMILIES})


def case(name):
    cls, a = SPECS[name]
    c = cls(*a)
    c.name = name
    return c


def names(kernel):
    return [n for n in NAMES if n.startswith(kernel + "-")]


def bars(name):
    """not cached: the large cases hold hundreds of megabytes (the CPU proofs keep `proof(name)`, a summary)"""
    return Bars(case(name))


@functools.lru_cache(maxsize=None)
def proof(name):
    """what tests/test_rms_cases_cpu.py asserts about one case, without the tensors"""
    b = bars(name)
    c = b.case
    got = c.replay()
    cols = {}
    for nm, q in b.q.items():
        if q.col:
            cols[nm] = dict(bar=q.bar, noise=b.noise[nm], devs=[float((r[nm] - q.want).abs().max()) for r in b.mut.values()])
    return dict(kernel=c.kernel, mutants=list(b.mut), undetected={m: b.ratios(b.mut[m]) for m in b.undetected()}, cols=cols,
                replay=b.ratios(got), shares={nm: q.share(got[nm]) for nm, q in b.q.items()},
                rstd=c.rstd_distance() if hasattr(c, "rstd_distance") else 0.0, silu=c.silu_distance() if hasattr(c, "silu_distance") else (0.0, 0.0),
                ambiguous=(int(c.ambiguous.sum()), c.ambiguous.numel()) if hasattr(c, "ambiguous") else (0, 1))


# (case, quantity): column sums no mutant of the case moves by DETECT x noise, or whose bar would be under 8 x noise
NOT_ASSERTED = {}
# (case, mutant): not caught by any asserted quantity of that case; every one is caught by another case of its kernel
_ZERO = "the case's only row is all zero: y = 0, the dot product is 0 and dw is 0 whatever multiplies them"
_LOUD = "the case's only row is of magnitude 1e4: eps against a mean square of 1e8 moves nothing"
_ONE = "one row and one head at position 0: no row stride is used, the rotation is the identity, and eps = 1e-6 against a mean square of order 1 moves nothing"
EXEMPT_MUTANTS = {("rmsnorm-1280-1", "mean_over_dim_minus_1"): "the only row is of magnitude 1e-4: its mean square 2e-8 is nothing against this family's eps = 1e-5"}
for _f, (_widths, _, _) in RMS_FAMILIES.items():
    for _d in _widths:
        if RMS_WIDTHS.index(_d) % 3 == 1:
            EXEMPT_MUTANTS.update({(f"{_f}-{_d}-1", m): _ZERO
                                   for m in ("mean_over_dim_minus_1", "rstd_squared", "dw_without_rstd", "dot_without_w", "neighbour_width")})
        if RMS_WIDTHS.index(_d) % 3 == 2:
            EXEMPT_MUTANTS[(f"{_f}-{_d}-1", "no_eps")] = _LOUD
EXEMPT_MUTANTS.update({("head_rmsnorm-1-1", m): _ONE for m in ("no_eps", "stride_of_x_for_dy")})
EXEMPT_MUTANTS.update({("qkrms_rope-1-1-1", m): _ONE for m in ("no_eps", "half_split", "unconj_bwd")})
