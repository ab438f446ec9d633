"""The power of the bar cases in tests/test_varlen_attention_gpu.py, proved on the CPU from the float64 references of
tests/varlen_attention_cases.py alone (no kernel, no GPU): the NOT_ASSERTED table is exact, every asserted tolerance follows the rule of
tests/attention_cases.py (a quarter of the smallest detectable deviation, at most REL_CAP row-relative, at least 8 x noise), and at every
packing and head pair every mutant -- a key leaked across a boundary in either direction, a key or a query dropped at an edge index of a
sequence, the last key or query counted twice, the wrong KV head, a query head missing from a group's dK / dV sum -- is seen by at least one
family in an asserted quantity."""
import collections
import math

import pytest
import torch

from tests import attention_cases as A
from tests import varlen_attention_cases as V

KEYS = V.case_keys()
SHAPES = [(lengths, heads) for lengths in V.PACKINGS for heads in V.HEADS]
shape_id = lambda s: f"n{len(s[0])}first{s[0][0]}-h{s[1][0]}_{s[1][1]}"


@pytest.mark.parametrize("key", KEYS, ids=V.key_id)
def test_bars_follow_the_rule_and_unasserted_quantities_are_named(key):
    b = V.bars(*key)
    fam = key[0]
    for n in V.FWD_Q + V.BWD_Q:
        if b.tol[n] is None:
            assert (fam, n) in V.NOT_ASSERTED, (n, b.noise[n])
            continue
        hits = [d[n] for d in b.dev.values() if n in d and d[n] >= A.DETECT * b.noise[n]]
        assert hits and b.tol[n] <= min(hits) / 4 * (1 + 1e-12) and b.tol[n] >= 8 * b.noise[n]
        assert n == "lse2" or b.tol[n] <= A.REL_CAP
    assert all(b.tol[n] is not None for n in ("lse2", "o", "dv"))         # asserted in every case of every family
    if fam == "random1":                                                   # the family that carries dQ and dK at every packing and head pair
        assert all(b.tol[n] is not None for n in V.BWD_Q) and not b.undetected()
    if fam == "flat":
        assert not b.undetected()


def test_the_not_asserted_table_is_exact():
    unasserted = set()
    for key in KEYS:
        unasserted |= {(key[0], n) for n, t in V.bars(*key).tol.items() if t is None}
    assert unasserted == set(V.NOT_ASSERTED), unasserted ^ set(V.NOT_ASSERTED)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_mutant_is_caught_at_every_packing_and_head_pair(shape):
    lengths, (Hq, Hkv) = shape
    caught = collections.defaultdict(bool)
    for fam in V.FAMILIES:
        b = V.bars(fam, lengths, (Hq, Hkv))
        u = set(b.undetected())
        for m in b.dev:
            caught[m] |= m not in u
    missed = [m for m, ok in caught.items() if not ok]
    assert not missed, missed
    want = {"group_head_missing"} | ({"wrong_kv_head"} if Hq != Hkv else set())        # the mutant list itself: every boundary, every edge index
    for b, L in enumerate(lengths):
        want |= {f"fwd_dup_last_key_b{b}", f"bwd_dup_last_query_b{b}"} | {f"bwd_drop_query_b{b}_{i}" for i in A.edges(L)}
        if L > 1:
            want |= {f"bwd_dup_last_key_b{b}"} | {f"{p}_drop_key_b{b}_{j}" for p in ("fwd", "bwd") for j in A.edges(L)}
        if b > 0:
            want |= {f"fwd_leak_prev_b{b}", f"bwd_leak_prev_b{b}"}
        if b < len(lengths) - 1:
            want |= {f"fwd_leak_next_b{b}", f"bwd_leak_next_b{b}"}
    assert set(caught) == want


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_constructed_families_are_what_they_claim(shape):
    lengths, heads = shape
    b = V.bars("flat", lengths, heads)
    want = torch.cat([torch.full((L,), math.log2(L), dtype=torch.float64) for L in lengths])
    assert float((b.ref.base["lse2"] - want).abs().max()) < 1e-12
    b = V.bars("planted", lengths, heads)
    o = b.ref.base["o"]
    assert float((o - o.round()).abs().max()) < 1e-9 and float(o.abs().max()) < 8 + 1e-9   # o_i = v[target(i)], an integer, and no poison (1000)
    muts = b.ref.mutants()
    for s, L in enumerate(lengths):                          # a row leaked from a neighbour of 16 rows and more takes the softmax: o lands on 1000
        for name, nb in ((f"fwd_leak_next_b{s}", s + 1), (f"fwd_leak_prev_b{s}", s - 1)):
            if name in muts and lengths[nb] >= 2 * A.POISON_ROWS:
                leaked = dict((n, t) for n, _, t in muts[name])["o"]
                assert float((leaked - A.POISON_V).abs().max()) < 1e-6, name


def test_the_group_sum_and_the_head_map_are_flash_attention_s():
    """the reference against torch's attention per sequence on K / V repeat_interleave'd over the group (flash-attn's published contract)"""
    c = V.bars("random1", V.PACKINGS[0], (6, 2)).case
    ref = V.bars("random1", V.PACKINGS[0], (6, 2)).ref
    M, g = c.M, 3
    q = c.q_backing[:M].double().reshape(M, 6, 64).requires_grad_(True)
    k = c.k_backing[:M].double().reshape(M, 2, 64).requires_grad_(True)
    v = c.v_backing[:M].double().reshape(M, 2, 64).requires_grad_(True)
    out = []
    for a, e in zip(c.cu[:-1], c.cu[1:]):
        qs = q[a:e].transpose(0, 1)
        ks, vs = (t[a:e].repeat_interleave(g, dim=1).transpose(0, 1) for t in (k, v))
        out.append((torch.softmax(qs @ ks.transpose(-1, -2) * 0.125, -1) @ vs).transpose(0, 1))
    o = torch.cat(out, 0)
    (o * c.dO_backing[:M].double().reshape(M, 6, 64)).sum().backward()
    for n, t in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert float((ref.base[n] - t.permute(1, 0, 2)).abs().max()) < 1e-9 * max(1.0, float(t.abs().max())), n
