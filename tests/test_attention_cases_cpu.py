"""The power of tests/test_attention_edges_gpu.py, proved on the CPU from the float64 references alone (no kernel, no GPU).  Per case: every
reference mutant of tests/attention_cases.py -- the same formula with one key or query miscounted -- moves an asserted quantity by 32 x
its rounding noise, or is named in the module's exemption tables; every asserted tolerance is at most a quarter of the deviations it has
to catch, at most 0.5 row-relative and at least 8 x noise; every quantity a case leaves out is named.  The tables are exact.  Per shape:
every mutant is caught by some family.  And the constructed families are what they claim to be."""
import collections
import math

import pytest
import torch

from tests import attention_cases as A

KEYS = A.case_keys()
SHAPES = collections.OrderedDict()
for _k in KEYS:
    SHAPES.setdefault((_k[0], _k[3], _k[2], _k[4]), []).append(_k)          # (kind, hd, L, q_begin) -> the families built at that shape


@pytest.mark.parametrize("key", KEYS, ids=A.key_id)
def test_every_mutant_is_caught_by_its_case_or_named(key):
    """A mutant is caught by a case when it moves an ASSERTED quantity by at least 32 x that quantity's noise.  Everything a case cannot
    catch, and every quantity it does not assert, is named in the module's two tables."""
    b = A.bars(*key)
    fam = key[1]
    for m in b.undetected():
        assert (fam, A.mutant_class(m)) in A.EXEMPT_MUTANTS, (m, b.dev[m], b.noise)
    for n in A.FWD_Q + A.BWD_Q:
        if b.tol[n] is None:
            assert (fam, n) in A.NOT_ASSERTED, (n, b.noise[n])
            continue
        hits = [d[n] for d in b.dev.values() if n in d and d[n] >= A.DETECT * b.noise[n]]
        assert hits and b.tol[n] <= min(hits) / 4 * (1 + 1e-12) and b.tol[n] >= 8 * b.noise[n]
        assert n == "lse2" or b.tol[n] <= A.REL_CAP
    assert b.tol["lse2"] is not None and b.tol["dv"] is not None          # asserted in every case of every family
    assert b.tol["o"] is not None or fam in ("flat", "planted")


def test_the_exemption_tables_are_exact():
    """no stale entry: every named (family, mutant) is really missed by some case, every named (family, quantity) really unasserted"""
    missed, unasserted = set(), set()
    for key in KEYS:
        b = A.bars(*key)
        missed |= {(key[1], A.mutant_class(m)) for m in b.undetected()}
        unasserted |= {(key[1], n) for n, t in b.tol.items() if t is None}
    assert missed == set(A.EXEMPT_MUTANTS), missed ^ set(A.EXEMPT_MUTANTS)
    assert unasserted == set(A.NOT_ASSERTED), unasserted ^ set(A.NOT_ASSERTED)


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}-hd{s[1]}-L{s[2]}-q{s[3]}")
def test_every_mutant_is_caught_at_every_shape(shape):
    """what one family cannot see by construction another does: at every shape every mutant, the exempt ones included, is caught by at
    least one family's case"""
    caught = collections.defaultdict(bool)
    for key in SHAPES[shape]:
        b = A.bars(*key)
        u = set(b.undetected())
        for m in b.dev:
            caught[m] |= m not in u
    missed = [m for m, ok in caught.items() if not ok]
    assert not missed, missed
    assert "bwd_zero_key" not in caught                                      # exempt by name: a no-op for a backward that recomputes P from lse2


@pytest.mark.parametrize("key", KEYS, ids=A.key_id)
def test_exempt_mutants_are_no_ops(key):
    b = A.bars(*key)
    base = b.ref.base
    for name in A.EXEMPT:
        r = b.ref.mutant(name)
        for n in r:
            assert torch.equal(r[n], base[n]), (name, n)


@pytest.mark.parametrize("key", [k for k in KEYS if k[1] == "planted"], ids=A.key_id)
def test_planted_reference_equals_the_planted_integers(key):
    b = A.bars(*key)
    c, ref = b.case, b.ref
    want = torch.gather(ref.v, 2, c.planted[:, :, c.q_begin:, None].expand(-1, -1, -1, c.hd))
    assert float((ref.base["o"] - want).abs().max()) < 1e-9
    assert float(want.abs().max()) <= 8 and float(want.abs().min()) >= 1      # no poison (v = 1000) among the targets, no zeros


@pytest.mark.parametrize("key", [k for k in KEYS if k[1] == "flat"], ids=A.key_id)
def test_flat_reference_is_the_count_of_visible_keys(key):
    b = A.bars(*key)
    c = b.case
    i = torch.arange(c.q_begin, c.L, dtype=torch.float64)
    want = torch.log2(i + 1) if c.causal else torch.full_like(i, math.log2(c.L))
    assert float((b.ref.base["lse2"] - want).abs().max()) < 1e-12


@pytest.mark.parametrize("key", [k for k in KEYS if k[1] in ("ramp_rise", "ramp_wave") and k[2] > 64], ids=A.key_id)
def test_ramp_fires_the_lazy_rescale_in_every_tile(key):
    """fwd_tile moves its reference point when a row maximum of the tile exceeds it by more than 8 (log2 units).  Replayed on the
    float64 scores: for the ramp queries that happens in every 64-key tile after the first, the ragged last one included (causal: every
    tile the query sees), so O and l are rescaled from a non-empty accumulator in both unrolled bodies, the tail and the masked tile."""
    b = A.bars(*key)
    c, ref = b.case, b.ref
    s2 = ref.s2 + torch.where(ref.vis > 0, 0.0, -math.inf)
    nt = (c.L + 63) // 64
    fired = torch.zeros(c.B, c.H, c.L - c.q_begin, nt, dtype=torch.bool)
    m = torch.full(s2.shape[:-1], -math.inf, dtype=torch.float64)
    for t in range(nt):
        want = s2[..., t * 64:(t + 1) * 64].amax(-1)
        fire = want > m + 8
        fired[..., t] = fire
        m = torch.where(fire, torch.maximum(m, want), m)
    ramp_rows = torch.ones(c.L - c.q_begin, dtype=torch.bool)
    ramp_rows[[i for i in range(c.L - c.q_begin) if (i + c.q_begin) % 8 == 3]] = False        # the probe queries have no ramp
    for t in range(1, nt):
        rows = ramp_rows & (ref.qi >= t * 64 if c.causal else torch.ones_like(ramp_rows))        # causal: rows that see a key of tile t
        if rows.any():
            assert bool(fired[:, :, rows, t].all()), t


GROUPS = collections.OrderedDict()
for _f, _n in A.decode_keys():
    GROUPS.setdefault(_n, []).append(_f)


@pytest.mark.parametrize("n_keys", list(GROUPS))
def test_every_decode_mutant_is_caught(n_keys):
    """per case: caught, or (family, mutant) named; per n_keys: caught by some family, but for the one mutant decode_exempt() explains"""
    caught = collections.defaultdict(list)
    for fam in GROUPS[n_keys]:
        c = A.decode_case(fam, n_keys)
        d = c.bars()
        if d["tol"] is None:
            assert (fam, n_keys) in A.DECODE_NOT_ASSERTED
        else:
            assert 8 * d["noise"] <= d["tol"] <= A.REL_CAP
            assert d["tol"] <= min(v for v in d["dev"].values() if v >= A.DETECT * d["noise"]) / 4 * (1 + 1e-12)
        for m, v in d["dev"].items():
            caught[m].append(d["tol"] is not None and m not in d["undetected"])
            assert caught[m][-1] or (fam, A.mutant_class(m)) in A.DECODE_EXEMPT_MUTANTS, (fam, m)
        if fam == "planted":
            want = torch.gather(c.vc[: c.B].double(), 2, c.planted[:, :, None, None].expand(-1, -1, 1, 64)).squeeze(2)
            assert float((c.reference() - want).abs().max()) < 1e-9 and float(want.abs().max()) <= 8
    missed = [m for m, hits in caught.items() if not any(hits) and not A.decode_exempt(m, n_keys)]
    assert not missed, missed


def test_the_decode_exemption_tables_are_exact():
    missed, unasserted = set(), set()
    for fam, n in A.decode_keys():
        d = A.decode_case(fam, n).bars()
        missed |= {(fam, A.mutant_class(m)) for m in d["undetected"]}
        if d["tol"] is None:
            unasserted.add((fam, n))
            missed |= {(fam, A.mutant_class(m)) for m in d["dev"]}
    assert missed == set(A.DECODE_EXEMPT_MUTANTS), missed ^ set(A.DECODE_EXEMPT_MUTANTS)
    assert unasserted == set(A.DECODE_NOT_ASSERTED)
