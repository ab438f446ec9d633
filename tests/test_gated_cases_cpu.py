"""The power of tests/test_gated_edges_gpu.py, proved on the CPU from the float64 references of tests/gated_cases.py alone (no kernel, no
GPU).  Per case: every reference mutant is caught by an asserted quantity (ratio >= 4 of its bar) or named in EXEMPT_MUTANTS; every column
sum that is left out is named in NOT_ASSERTED; both tables are exact.  Per kernel: every mutant is caught by some case.  Every column bar
is at least 8 x its noise and at most a quarter of the smallest deviation it has to catch.  "At least 8 x noise" is asserted for the
column sums ONLY: the elementwise bars are the analytic rounding bounds of tests/gated_cases.py (tighter than 8 x a replay distance could
be: one final rounding is itself the largest part of the replay's distance), and for them the two checks are "every mutant reaches 4 x the
bar" and "the fp32 replay stays within 1 x the bar".  The fp32 replay of every case passes every bar
and every share condition.  With the rounding points switched off every backward restatement is torch.autograd of its forward."""
import collections

import pytest
import torch

from tests import gated_cases as G

NAMES = list(G.SPECS)
KERNELS = collections.OrderedDict()
for _n in NAMES:
    KERNELS.setdefault(G.SPECS[_n][0].kernel + ("-" + G.SPECS[_n][1][0] if G.SPECS[_n][0] is G.GateCase else ""), []).append(_n)


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_is_caught_by_its_case_or_named(name):
    b = G.bars(name)
    for m in b.undetected():
        assert (name, m) in G.EXEMPT_MUTANTS, (m, b.ratios(b.mut[m]))
    for nm, q in b.q.items():
        if not q.col:
            continue
        if q.bar is None:
            assert (name, nm) in G.NOT_ASSERTED, (nm, b.noise[nm])
            continue
        devs = [float((r[nm] - q.want).abs().max()) for r in b.mut.values()]
        hits = [d for d in devs if d >= G.DETECT * b.noise[nm]]
        assert hits and q.bar <= min(hits) / 4 * (1 + 1e-12) and q.bar >= 8 * b.noise[nm]


def test_the_exemption_tables_are_exact():
    missed, unasserted = set(), set()
    for name in NAMES:
        b = G.bars(name)
        missed |= {(name, m) for m in b.undetected()}
        unasserted |= {(name, nm) for nm, q in b.q.items() if q.col and q.bar is None}
    assert missed == set(G.EXEMPT_MUTANTS), missed ^ set(G.EXEMPT_MUTANTS)
    assert unasserted == set(G.NOT_ASSERTED), unasserted ^ set(G.NOT_ASSERTED)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_every_mutant_is_caught_by_some_case_of_its_kernel(kernel):
    caught = collections.defaultdict(bool)
    for name in KERNELS[kernel]:
        b = G.bars(name)
        u = set(b.undetected())
        for m in b.mut:
            caught[m] |= m not in u
    assert caught and all(caught.values()), [m for m, ok in caught.items() if not ok]
    want = {"qknorm_rope": set(G.QK_ALL_MUTANTS),
            "sigmoid_gate-block": {"sigmoid_unrounded", "dsig_unrounded", "gate_col_minus_D", "gate_stride_D"},
            "sigmoid_gate-cols": {"sigmoid_unrounded", "dsig_unrounded", "gate_col_minus_D", "gate_stride_D", "dgate_at_gate_rs", "cap_dropped"},
            "geglu": {"halves_swapped", "gelu_unrounded", "out_stride_I", "da_stride_I", "cap_dropped"},
            "stat_gate": {"b2_dropped", "logit_unrounded", "p_unrounded", "dp_unrounded", "drop_last_row", "drop_last_group", "drop_last_block", "w2_chunks_permuted",
                          "stride_W", "dz_unmasked", "extra_channel", "z_unmasked", "no_ste_term", "no_dmask", "no_dprobs"}}[kernel]
    assert set(caught) == want, set(caught) ^ want


def test_the_dropped_terms_are_caught_with_ste_on_and_off():
    """no_dprobs with ste = 0 and ste = 1; the STE term and dmask only exist with ste = 1"""
    seen = collections.defaultdict(set)
    for name in KERNELS["stat_gate"]:
        b = G.bars(name)
        for m in ("no_ste_term", "no_dmask", "no_dprobs"):
            if m in b.mut and b.caught(m):
                seen[m].add(b.case.ste)
    assert seen["no_dprobs"] == {0, 1} and seen["no_ste_term"] == {1} and seen["no_dmask"] == {1}


@pytest.mark.parametrize("name", NAMES)
def test_the_fp32_replay_passes_every_bar_and_share(name):
    b = G.bars(name)
    got = b.case.replay()
    for nm, r in b.ratios(got).items():
        assert r is None or r <= 1.0, (nm, r)
    for nm, q in b.q.items():
        assert q.share(got[nm]) <= G.SHARE, (nm, q.share(got[nm]))
    c = b.case
    if getattr(c, "exhaustive", False):                   # at most 1 % of the finite patterns may accept either neighbour
        assert int(c.finite.sum()) == 65280
        assert 0 < int((c.ambiguous & c.finite).sum()) <= 0.01 * 65280
    if isinstance(c, G.StatCase):                        # at most 2 % of the rows may accept a second probs (one row below 50 rows)
        assert c.ambiguity_ok(), int(c.ambiguous_rows.sum())


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("qknorm_rope") and G.SPECS[n][1][1] < 500])
def test_qknorm_backward_is_autograd_of_the_forward(name):
    c = G.case(name)
    M, D = c.M, c.D
    x = torch.nan_to_num(c.qkvg.double()).requires_grad_(True)
    P = [p.double().requires_grad_(True) for p in c.params]
    e = c.evaluate(rb=G.ident, x=x, params=P)
    gy = torch.stack([c.up.double()[:, i * D:(i + 1) * D].reshape(M, c.H, 64) for i in (0, 1)])
    (e["y"] * gy).sum().backward()
    r = c._assemble({k: (v.detach() if torch.is_tensor(v) else v) for k, v in e.items()})
    assert _close(r["dqkvg"][:M, :2 * D], x.grad[:, :2 * D])
    for nm, p in zip(G.QK_COLS, P):
        assert _close(r[nm], p.grad), nm


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("sigmoid_gate", "geglu")) and "4100" not in n and "True" not in n])
def test_gate_and_geglu_backward_is_autograd_of_the_forward(name):
    c = G.case(name)
    if isinstance(c, G.GateCase):
        o = c.o[: c.M].double().requires_grad_(True)
        gate = c.gate_backing[: c.M, c.col:c.col + c.D].double().requires_grad_(True)
        (r, _, _), _, dy, _ = c.evaluate(rb=G.ident, o=o, gate=gate)
        (r["og"] * dy).sum().backward()
        assert _close(r["d_o"].detach(), o.grad) and _close(r["dgate"].detach(), gate.grad)
    else:
        h = c.h[: c.M].double().requires_grad_(True)
        (r, _), _, _, dy = c.evaluate(rb=G.ident, h=h)
        (r["a"] * dy).sum().backward()
        assert _close(torch.cat([r["dx"], r["dg"]], 1).detach(), h.grad)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("stat_gate") and "8193" not in n])
def test_stat_backward_is_autograd_of_the_forward(name):
    c = G.case(name)
    G.bars(name)
    f = c.fsq
    u = c.rows(c.u_backing).double().requires_grad_(True)
    w2, b2 = c.w2.double().requires_grad_(True), c.b2.double().requires_grad_(True)
    z = c.z.double().requires_grad_(True)
    g = G.gelu(u)
    p = torch.sigmoid(g @ w2 + b2)
    mask = c.mask.double()
    m = (mask - p).detach() + p if c.ste else mask
    loss = (c.dprobs.double() * p).sum() if c.has_dprobs else 0.0
    if c.ste and c.has_dmask:
        loss = loss + (c.dmask.double() * m).sum()
    if c.has_z:
        bounded = torch.tanh(z * m[:, None] + f.shift.double()) * f.half_l.double() - f.offset.double()
        q = bounded + (torch.round(bounded) - bounded).detach()
        loss = loss + (c.dcodes.double() * q / f.hw.double()).sum()
    loss.backward()
    bw = c.backward(p.detach(), mask, g=g.detach(), pure=True)
    assert _close(bw["dU"], u.grad) and _close(bw["dw2"], w2.grad) and _close(bw["db2"], b2.grad)
    if c.has_z:
        assert _close(bw["dz"], z.grad)
