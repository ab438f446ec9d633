"""The case table of tests/vq_cases.py proves its own power without a kernel: every case still reaches the planner path it claims, its
token subset obeys the coverage rule, its specials behave as designed in the oracle, every mutant is caught by some case (and by the
cases built for it), and the fp32 replay of the token backward stays inside the analytic bar."""
import numpy as np
import pytest
import torch

from oracle import vq_c
from tests import vq_cases as V


@pytest.mark.parametrize("name", V.names())
def test_case_reaches_what_it_claims(name):
    c = V.CASES[name]
    p = V.split_plan(c.N, c.K)
    for k, v in c.claims.items():
        assert p[k] == v, (name, k, p[k], v)
    for kind, i, j, t in c.ties:
        assert i < j < c.K and t < c.N
        assert V.tie_kind(i, j, c.N, c.K) == kind, (name, i, j, V.tie_kind(i, j, c.N, c.K))
    codes = [k for _, i, j, _ in c.ties for k in (i, j)] + [k for k, _ in c.hits] + list(c.zero_codes)
    toks = [t for *_, t in c.ties] + [t for _, t in c.hits] + list(c.zero_tokens)
    assert len(set(codes)) == len(codes) and len(set(toks)) == len(toks) and all(k < c.K for k in codes) and all(t < c.N for t in toks)
    assert c.mode == "L" or c.l2n
    assert V.workspace_floats(c.N, c.K, c.d)[0] >= V.workspace_floats(c.N, c.K, c.d)[1]


def test_table_covers_the_paths_of_the_issue():
    cs = V.CASES.values()
    for mode in "LD":                                                           # every d instantiation, both modes, ragged everything
        assert {c.d for c in cs if c.mode == mode and c.K % 128 and c.K % 32 and c.N % 256 and c.N % 32} == {8, 16, 24, 32}
    assert {V.split_plan(c.N, c.K)["cps"] for c in cs} >= {1, 3, 4}
    assert {(c.N, c.K) for c in cs} >= {(1, 1), (1, 5), (31, 127), (257, 129), (64, 5), (3073, 15437), (12288, 6145)}
    assert {c.d for c in cs if not c.l2n} == {8, 24}
    kinds = {k for c in cs for k, *_ in c.ties}
    assert kinds == {"half", "tile", "chunk", "split"}
    assert any(c.zero_tokens for c in cs if c.mode == "L") and any(c.zero_tokens for c in cs if c.mode == "D")
    assert any(c.zero_codes for c in cs)
    assert all(c.ldz == c.d + 8 and c.ldp == 64 for c in cs if c.N == 289)
    # the codebook-gradient plan: the cap binds first at N = 16385 (three empty slabs), N = 3585 has one token in its last slab
    assert V.cb_plan(16384)["empty"] == 0 and V.cb_plan(16385) == {"ns": 32, "slab_len": 576, "empty": 3, "last_len": 257, "partial_chunk": 1}
    p = V.cb_plan(3585)
    assert (p["ns"], p["slab_len"], p["last_len"], p["empty"]) == (8, 512, 1, 0)
    shapes = V.cbgrad_cases()
    assert {(N, K, d) for N, K, d, _, _ in shapes} >= {(N, K, d) for d in (8, 32) for K in (5, 77, 300) for N in (1, 63, 513, 3585)} | {(16385, 77, 8)}
    assert {l2n for *_, l2n, _ in shapes} == {0, 1} and any(col for *_, col in shapes)
    bw = V.bwd_cases()
    for l2n in (0, 1):
        for d in V.BWD_D:
            assert {v for N, dd, ll, v in bw if dd == d and ll == l2n} == set(V.BWD_VARIANTS)
            assert {N for N, dd, ll, v in bw if dd == d and ll == l2n} == set(V.BWD_N)


@pytest.mark.parametrize("name", V.names())
def test_token_subset_obeys_the_coverage_rule(name):
    c = V.CASES[name]
    sel = set(V.token_subset(c).tolist())
    assert sel <= set(range(c.N)) and set(c.special_tokens) <= sel
    if not c.subset:
        assert len(sel) == c.N
        return
    for w in range((c.N + 255) // 256):
        first, last = 256 * w, min(c.N, 256 * w + 256) - 1
        if last - first + 1 < 256:
            assert set(range(first, last + 1)) <= sel, w                      # every token of the partial workgroup
            continue
        for tile in (first // 32, last // 32):                                  # the tiles at the workgroup's two ends
            assert 32 * tile in sel and 32 * tile + 31 in sel, (w, tile)
    assert len(sel) < c.N // 4                                                  # and it is a subset: the oracle stays near a second


@pytest.mark.parametrize("name", V.names())
def test_specials_behave_as_designed(name):
    c, r = V.CASES[name], V.reference(name)
    at = {int(t): int(i) for t, i in zip(r.sel, r.idx)}
    W, _ = V.inputs(name)
    for kind, i, j, t in c.ties:
        assert np.array_equal(W[i], W[j]) and np.array_equal(r.E[i], r.E[j])
        assert at[t] == i, (name, kind, i, j, at[t])                            # the lowest index wins, in both modes
    for k, t in c.hits:
        assert at[t] == k
    for k in c.zero_codes:
        assert not r.E[k].any() and r.wnorm[k] == np.float32(1e-12 if c.l2n else 1.0)
    for t in c.zero_tokens:
        assert not r.zn[t].any() and r.znorm[t] == np.float32(1e-12)
        if c.mode == "D":
            assert at[t] == 0                                                   # every score ties at 0
        else:
            ee = (r.E.astype(np.float64) ** 2).sum(1)
            sc = vq_c.search(r.zn[t:t + 1], r.E, "L")[1][0]
            tied = int((np.abs(ee - sc) < 1e-7).sum())
            assert tied >= 2 and at[t] > 0, (tied, at[t])                       # a natural many-way tie, not won by code 0
    assert r.idx.min() >= 0 and r.idx.max() < c.K


def test_every_mutant_is_caught():
    table = {m: [n for n in V.names() if V.caught(n, m)] for m in V.MUTANTS}
    print("\nmutant -> cases that catch it")
    for m, ns in table.items():
        print(f"VQ_MUTANT {m:24s} {len(ns):2d}  {' '.join(ns)}")
    for m, ns in table.items():
        assert ns, f"no case catches mutant {m}"
    for n, c in V.CASES.items():
        for m in c.must_catch:
            assert n in table[m], f"{n} no longer catches {m}"
    # a mutant never moves a token the reference does not own: the vectors have the reference's length
    for n in V.names():
        for m in V.MUTANTS:
            got = V.mutant_idx(n, m)
            assert got is None or got[1].shape == got[0].shape


def test_pad5_cases_hold_the_tokens_they_were_built_for():
    rL, rD = V.reference("pad5_d24_L"), V.reference("pad5_d24_D")
    cos = rL.zn.astype(np.float64) @ rL.E.astype(np.float64).T
    assert (cos.max(1) < 0.5).sum() > 32                                        # mode L: a zero code at distance |z|^2 = 1 would win
    assert ((rD.zn.astype(np.float64) @ rD.E.astype(np.float64).T).max(1) < 0).sum() >= 1   # mode D: a zero code's logit 0 would win


def test_score_gap_bound_accepts_the_oracle_and_rejects_a_wrong_code():
    for name in ("ragged_d8_L", "ragged_d32_D", "raw_d24_L"):
        c, r = V.CASES[name], V.reference(name)
        zn, E, idx = (torch.from_numpy(np.array(a)) for a in (r.zn, r.E, r.idx))
        gap, bound = V.score_gap_and_bound(zn, E, idx, c.mode)
        assert bool((gap <= bound).all()) and bool((gap >= 0).all())
        wrong = (idx + 1) % c.K                                                  # some other code: far outside the bound on most tokens
        gap, bound = V.score_gap_and_bound(zn, E, wrong, c.mode)
        assert float((gap > bound).double().mean()) > 0.9


@pytest.mark.parametrize("N,d,l2n,variant", V.bwd_cases())
def test_backward_replay_is_inside_the_bar(N, d, l2n, variant):
    W, z, gb = V.bwd_inputs(N, V.BWD_K, d, l2n)
    g = None if variant == "no_g_rz" else gb[:, :d]
    if l2n:
        zn, znorm = vq_c.normalize_rows(z)
        E, _ = vq_c.normalize_rows(W)
    else:
        zn, znorm, E = z, np.ones(N, np.float32), W
    idx, _ = vq_c.search(zn, E, "L")
    want, dW, bar = V.bwd_reference(z, W, idx, g, V.GSCAL, l2n)
    got = torch.from_numpy(V.bwd_replay(zn, znorm, E, idx, g, V.GSCAL, l2n)).double()
    assert bool((bar > 0).all()) and bool(torch.isfinite(want).all())
    r = float(((got - want).abs() / bar).max())
    assert r <= 1.0, r
    r16 = float(((got.float().to(torch.bfloat16).double() - want).abs() / V.bwd_bar_bf16(want, bar)).max())
    assert r16 <= 1.0, r16
    # the bar is worth something: dropping the commit term, or taking the default beta, is outside it by the factor 4 that
    # tests/gated_cases.py asks of a caught mutant (at N = 700 the loss terms are 1 / (N d) of the gradient that flows through rz)
    for gs, beta in (((V.GSCAL[0], 0.0, V.GSCAL[2]), V.BETA), (V.GSCAL, 0.25)):
        other = V.bwd_reference(z, W, idx, g, gs, l2n, beta=beta)[0]
        assert float(((other - want).abs() / bar).max()) >= 4.0
    # and the float64 codebook gradient agrees with the oracle's fixed-order one (loosely: that one is bit-compared on the GPU)
    wnorm = vq_c.normalize_rows(W)[1] if l2n else np.ones(V.BWD_K, np.float32)
    ref = vq_c.codebook_grad(zn, E, wnorm, idx, V.s_b_fp32(V.GSCAL, N, d), normalize=bool(l2n))
    assert np.allclose(ref, dW.numpy(), rtol=1e-4, atol=1e-6 * float(dW.abs().max()))
