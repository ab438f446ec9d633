"""Edge cases, float64 references, fp32 replays and reference mutants of vt_groupnorm_fwd / vt_groupnorm_bwd (csrc/vt_groupnorm.hip):
GroupNorm(G, C, eps) over (C/G channels x P positions) of each clip of a bf16 channels-last [B, P, C] tensor, with an optional fused swish.
Plain torch on the CPU: no GPU and no built library.  The pattern, the class Q and the constants FLOOR, RSQ_REL, DETECT and `silu_reach` /
`silu_grad_reach` are those of tests/rms_cases.py and tests/gated_cases.py: read their docstrings first.

REFERENCE: the formulas of the kernel's header in float64 on the exact bf16 inputs and fp32 parameters; the final rounding of an output is
part of the bar.  REPLAY: the same function in float32 (what an honest fp32 kernel may give; it must pass every bar).  MUTANT: the reference
with one thing miscounted -- group_of_neighbour, stats_over_batch, biased_by_one_position, swish_skipped (both directions where they apply),
dx_without_mean_terms (backward), and two for the parameter sums alone: dparams_of_first_clip, dparams_drop_last_position.  A mutant is
CAUGHT by a quantity when its ratio is >= 4.

Bars, from the reference's own operands (no constant comes from a kernel's output):
    mean   FLOOR max|x|                     an fp32 sum of bf16 values in any fixed order, times a rounded 1/n
    rstd   (RSQ_REL + 2 FLOOR) rstd         the mean of squared deviations in fp32, one reciprocal square root
    y      2^-8 |want| (the output's rounding) + |gamma| rstd FLOOR max|x| (the mean's error; this is what a constant input or a mean far
           above the deviation leaves) + (RSQ_REL + 4 FLOOR) (|xhat gamma| + |beta|); with swish the error of y passes through silu'
           (|silu'| <= 1.1) and `silu_reach` is added
    dx     2^-8 |want| + rstd (|dz gamma| (silu_grad_reach + |dy| / 2: |silu''| <= 1/2) + 4 FLOOR (|g gamma| + mean|g gamma| +
           |xhat| mean|g gamma xhat|)); the backward is given the reference's own mean and rstd, rounded to fp32, so that it is judged apart
           from the forward
    dgamma / dbeta: the column-sum rule of tests/gated_cases.py -- noise = `_sum_bound` of the float64 terms (with the terms' own elementwise
           error), floored at 2^-23 of the largest sum; a mutant is detectable at dev >= DETECT noise; bar = 1/4 of the smallest detectable
           deviation; not asserted (NOT_ASSERTED) where no mutant is detectable.
Cases: C/G in {1, 2, 4, 8} at 105 = 3 x 5 x 7 positions, B = 2 with different statistics per clip, a clip of mean 16 and deviation 1/4, a
constant clip (rstd = eps^-1/2), with and without swish, and two cases above CHUNK_ELEMS = 32768 elements per clip, the size from which the
kernels cut a clip into more than one workgroup per (clip, group) (2100 positions at 16 channels, 300 at 128).
POISON: operands are heads of NaN-tailed allocations, outputs are prefilled with the sentinels of tests/gemm_cases.py."""
import collections
import functools

import torch

from tests.conv3d_cases import TAIL, NAN, out_alloc, poisoned  # noqa: F401  (the GPU test's too)
from tests.gated_cases import DETECT, Q
from tests.gemm_cases import assert_bits, sentinel
from tests.rms_cases import FLOOR, RSQ_REL, silu_grad, silu_grad_reach, silu_reach
from tests.test_rows_edges_gpu import _sum_bound

EPS = float(torch.tensor(1e-6, dtype=torch.float32))
CHUNK_ELEMS = 32768            # GN_CHUNK_ELEMS of csrc/vt_groupnorm.hip
U8 = 2.0 ** -8

Case = collections.namedtuple("Case", "name B P C G swish kind")
CASES = [Case(f"cg{C // 16}_{'swish' if s else 'plain'}", 2, 105, C, 16, s, "two_clips") for C in (16, 32, 64, 128) for s in (0, 1)] + [
    Case("mean16_std_quarter", 1, 105, 32, 16, 1, "offset"), Case("mean16_std_quarter_plain", 2, 105, 64, 16, 0, "offset"),
    Case("constant", 2, 105, 32, 16, 1, "constant"), Case("constant_plain", 1, 105, 16, 16, 0, "constant"),
    Case("two_chunks_c16", 2, 2100, 16, 16, 1, "two_clips"), Case("two_chunks_c128", 1, 300, 128, 16, 0, "two_clips"),
    Case("groups_of_3", 2, 105, 48, 16, 1, "two_clips")]
BY_NAME = {c.name: c for c in CASES}
FWD_MUTANTS = ("group_of_neighbour", "stats_over_batch", "biased_by_one_position", "swish_skipped")
BWD_MUTANTS = ("group_of_neighbour", "stats_over_batch", "swish_skipped", "dx_without_mean_terms", "dparams_of_first_clip", "dparams_drop_last_position")


def applies(mutant, c):
    if mutant == "swish_skipped":
        return bool(c.swish)
    if mutant in ("stats_over_batch", "dparams_of_first_clip"):
        return c.B > 1
    if mutant in ("group_of_neighbour", "biased_by_one_position"):
        return c.kind != "constant"            # every group of a constant clip has the same mean and no deviation
    return True


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x, dz bf16 [B, P, C]; gamma, beta fp32 [C]"""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 31 * c.C)
    n = lambda *s: torch.randn(*s, generator=g)
    if c.kind == "two_clips":                  # clip 0: N(0, 1) with a per-group offset; clip b: mean 3 b, deviation 1 + b
        x = n(c.B, c.P, c.C) + (torch.arange(c.C) // (c.C // c.G) % 3).float()
        x = x * (1 + torch.arange(c.B)).view(-1, 1, 1) + 3.0 * torch.arange(c.B).view(-1, 1, 1)
    elif c.kind == "offset":
        x = 16.0 + 0.25 * n(c.B, c.P, c.C)
    else:
        x = torch.full((c.B, c.P, c.C), 2.75) * (1 + torch.arange(c.B)).view(-1, 1, 1)
    return dict(x=x.to(torch.bfloat16), dz=n(c.B, c.P, c.C).to(torch.bfloat16), gamma=1.0 + 0.5 * n(c.C), beta=0.5 * n(c.C))


def _stats(c, xg, mutant):
    """mean, rstd [B, 1, G, 1] of xg [B, P, G, cg]"""
    dims = (0, 1, 3) if mutant == "stats_over_batch" else (1, 3)
    mean = xg.mean(dims, keepdim=True)
    var = ((xg - mean) ** 2).mean(dims, keepdim=True)
    if mutant == "biased_by_one_position":
        var = var * c.P / (c.P - 1)
    if mutant == "stats_over_batch":
        mean, var = mean.expand(c.B, 1, c.G, 1), var.expand(c.B, 1, c.G, 1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    if mutant == "group_of_neighbour":
        mean, rstd = mean.roll(-1, 2), rstd.roll(-1, 2)
    return mean, rstd


def forward(c, d, dt=torch.float64, mutant=None):
    x, ga, be = d["x"].to(dt), d["gamma"].to(dt), d["beta"].to(dt)
    xg = x.view(c.B, c.P, c.G, c.C // c.G)
    mean, rstd = _stats(c, xg, mutant)
    y = ((xg - mean) * rstd).reshape(c.B, c.P, c.C) * ga + be
    z = y * torch.sigmoid(y) if c.swish and mutant != "swish_skipped" else y
    return dict(y=z, mean=mean.reshape(c.B, c.G), rstd=rstd.reshape(c.B, c.G))


def saved_stats(c, d):
    """what the backward is given: the reference's mean and rstd as fp32 holds them"""
    f = forward(c, d)
    return f["mean"].float(), f["rstd"].float()


def _bwd_terms(c, d, dt, mutant=None):
    x, dz, ga, be = d["x"].to(dt), d["dz"].to(dt), d["gamma"].to(dt), d["beta"].to(dt)
    mean, rstd = (t.to(dt).view(c.B, 1, c.G, 1) for t in saved_stats(c, d))
    if mutant == "group_of_neighbour":
        mean, rstd = mean.roll(-1, 2), rstd.roll(-1, 2)
    xhat = ((x.view(c.B, c.P, c.G, -1) - mean) * rstd).reshape(c.B, c.P, c.C)
    y = xhat * ga + be
    gy = dz * silu_grad(y) if c.swish and mutant != "swish_skipped" else dz
    return xhat, y, gy, rstd


def backward(c, d, dt=torch.float64, mutant=None):
    xhat, y, gy, rstd = _bwd_terms(c, d, dt, mutant)
    ga = d["gamma"].to(dt)
    gg = (gy * ga).view(c.B, c.P, c.G, -1)
    xh = xhat.view(c.B, c.P, c.G, -1)
    dims = (0, 1, 3) if mutant == "stats_over_batch" else (1, 3)
    m1, m2 = gg.mean(dims, keepdim=True), (gg * xh).mean(dims, keepdim=True)
    if mutant == "dx_without_mean_terms":
        m1, m2 = 0 * m1, 0 * m2
    dx = (rstd * (gg - m1 - xh * m2)).reshape(c.B, c.P, c.C)
    rows = gy[:1] if mutant == "dparams_of_first_clip" else gy[:, :-1] if mutant == "dparams_drop_last_position" else gy
    rows_x = xhat[:rows.shape[0], :rows.shape[1]]
    return dict(dx=dx, dgamma=(rows * rows_x).sum((0, 1)), dbeta=rows.sum((0, 1)))


@functools.lru_cache(maxsize=None)
def bars(name):
    """quantity -> Q, forward and backward"""
    c, d = BY_NAME[name], inputs(name)
    f = forward(c, d)
    x, ga, be = d["x"].double(), d["gamma"].double().abs(), d["beta"].double().abs()
    xmax = float(x.abs().max())
    rs_c = f["rstd"].repeat_interleave(c.C // c.G, 1).unsqueeze(1)                  # [B, 1, C]
    xg = x.view(c.B, c.P, c.G, -1)
    xhat = ((xg - f["mean"].view(c.B, 1, c.G, 1)) * f["rstd"].view(c.B, 1, c.G, 1)).reshape(c.B, c.P, c.C)
    y = xhat * d["gamma"].double() + d["beta"].double()
    ey = ga * rs_c * FLOOR * xmax + (RSQ_REL + 4 * FLOOR) * ((xhat * ga).abs() + be)
    want = f["y"]
    ybar = U8 * want.abs() + (1.1 * ey + silu_reach(y, torch.sigmoid(y)) if c.swish else ey)
    out = dict(y=Q(want, ybar), mean=Q(f["mean"], FLOOR * xmax), rstd=Q(f["rstd"], (RSQ_REL + 2 * FLOOR) * f["rstd"]))
    # backward
    xh, yb, gy, rstd = _bwd_terms(c, d, torch.float64)
    b = backward(c, d)
    dz = d["dz"].double().abs()
    ey_b = 4 * FLOOR * ((xh * ga).abs() + be)
    eg = dz * (silu_grad_reach(yb, torch.sigmoid(yb)) + 0.5 * ey_b) if c.swish else torch.zeros_like(dz)      # elementwise error of g
    gg = (gy * ga).abs().view(c.B, c.P, c.G, -1)
    m1 = gg.mean((1, 3), keepdim=True)
    m2 = (gg * xh.abs().view(c.B, c.P, c.G, -1)).mean((1, 3), keepdim=True)
    fl = (4 * FLOOR * (gg + m1 + xh.abs().view(c.B, c.P, c.G, -1) * m2)).reshape(c.B, c.P, c.C)
    rs_b = rstd.expand(c.B, 1, c.G, c.C // c.G).reshape(c.B, 1, c.C)
    out["dx"] = Q(b["dx"], U8 * b["dx"].abs() + rs_b * (eg * ga + fl))
    for q, terms, tol in (("dgamma", gy * xh, eg * xh.abs() + gy.abs() * 4 * FLOOR * xh.abs()), ("dbeta", gy, eg)):
        t2 = terms.reshape(-1, c.C)
        noise = max(_sum_bound(t2, float(tol.max())), 2.0 ** -23 * float(b[q].abs().max()))
        devs = [float((backward(c, d, mutant=m)[q] - b[q]).abs().max()) for m in BWD_MUTANTS if applies(m, c)]
        seen = [v for v in devs if v >= DETECT * noise]
        out[q] = Q(b[q], min(seen) / 4 if seen else None, col=True)
    return out


# (case, quantity): column sums no mutant of the case moves by DETECT x noise
NOT_ASSERTED = {
}


def check(q, alloc, what):
    """alloc: a whole flat output allocation after the call (CPU): its head against the quantity, its tail against the sentinel"""
    n = q.want.numel()
    r = q.ratio(alloc[:n].reshape(q.want.shape))
    assert r is None or r <= 1.0, f"{what}: ratio {r:.3f}"
    assert_bits(alloc[n:], sentinel((alloc.numel() - n,), alloc.dtype), what + " (behind the addressed part)")
    return r
