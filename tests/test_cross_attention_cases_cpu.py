"""The power of the bar cases in tests/test_cross_attention_gpu.py, proved on the CPU from the float64 references of
tests/cross_attention_cases.py alone (no kernel, no GPU): the NOT_ASSERTED table is exact, every asserted tolerance follows the rule of
tests/attention_cases.py (a quarter of the smallest detectable deviation, at most REL_CAP row-relative, at least 8 x noise), and at
every shape every mutant -- a key or a query dropped at an edge index, a zero key counted, the last key or query counted twice -- is
seen by at least one family in an asserted quantity."""
import collections
import math

import pytest
import torch

from tests import attention_cases as A
from tests import cross_attention_cases as X

KEYS = X.case_keys()


@pytest.mark.parametrize("key", KEYS, ids=X.key_id)
def test_bars_follow_the_rule_and_unasserted_quantities_are_named(key):
    b = X.bars(*key)
    fam, Lq, Lk = key
    for n in X.FWD_Q + X.BWD_Q:
        if b.tol[n] is None:
            assert (fam, n) in X.NOT_ASSERTED, (n, b.noise[n])
            continue
        hits = [d[n] for d in b.dev.values() if n in d and d[n] >= A.DETECT * b.noise[n]]
        assert hits and b.tol[n] <= min(hits) / 4 * (1 + 1e-12) and b.tol[n] >= 8 * b.noise[n]
        assert n == "lse2" or b.tol[n] <= A.REL_CAP
    assert b.tol["lse2"] is not None and b.tol["dv"] is not None          # asserted in every case of every family
    if fam == "random1" and Lk > 1:                                        # the family that carries dQ and dK at every shape with more than one key
        assert all(b.tol[n] is not None for n in X.BWD_Q)
    if Lk == 1:                                                            # one key: the softmax is constant, dS = 0
        assert b.tol["dq"] is None and b.tol["dk"] is None


def test_the_not_asserted_table_is_exact():
    unasserted = set()
    for key in KEYS:
        unasserted |= {(key[0], n) for n, t in X.bars(*key).tol.items() if t is None}
    assert unasserted == set(X.NOT_ASSERTED), unasserted ^ set(X.NOT_ASSERTED)


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: f"q{s[0]}-k{s[1]}")
def test_every_mutant_is_caught_at_every_shape(shape):
    caught = collections.defaultdict(bool)
    for fam in X.FAMILIES:
        b = X.bars(fam, *shape)
        u = set(b.undetected())
        for m in b.dev:
            caught[m] |= m not in u
    missed = [m for m, ok in caught.items() if not ok]
    assert not missed, missed
    Lq, Lk = shape
    want = {"fwd_zero_key", "fwd_dup_last_key", "bwd_dup_last_query"} | {f"bwd_drop_query_{i}" for i in A.edges(Lq)}
    if Lk > 1:
        want |= {"bwd_dup_last_key"} | {f"{p}_drop_key_{j}" for p in ("fwd", "bwd") for j in A.edges(Lk)}
    assert set(caught) == want                                             # the mutant list itself: every edge index of both lengths


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: f"q{s[0]}-k{s[1]}")
def test_constructed_families_are_what_they_claim(shape):
    Lq, Lk = shape
    b = X.bars("flat", Lq, Lk)
    assert float((b.ref.base["lse2"] - math.log2(Lk)).abs().max()) < 1e-12
    b = X.bars("planted", Lq, Lk)
    c, ref = b.case, b.ref
    want = torch.gather(ref.v, 2, c.planted[..., None].expand(-1, -1, -1, 64))
    assert float((ref.base["o"] - want).abs().max()) < 1e-9
    assert float(want.abs().max()) <= 8 and float(want.abs().min()) >= 1      # no poison (v = 1000) among the targets, no zeros
