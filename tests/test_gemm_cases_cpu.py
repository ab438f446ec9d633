"""The GEMM cases of tests/gemm_cases.py can tell a wrong kernel from a right one: rounding shares, the measured GELU floor, every
applicable reference mutant caught by every case (exemption table exact and capped), poison where it is claimed.  CPU only."""
import pytest
import torch

from tests import gemm_cases as G

ALL_NT = G.NT_CASES + G.GELU_CASES


def test_case_axes_cover_what_the_module_claims():
    cs = G.NT_CASES
    assert {c.M for c in cs} >= {1, 17, 64, 65, 127, 129, 191, 193, 200} and {c.N for c in cs} >= {4, 6, 18, 130, 192, 196, 198, 380}
    assert {c.K // 64 for c in cs} == {1, 2, 3, 4, 5, 7}
    for epi in (G.EPI_BF16, G.EPI_F32, G.EPI_MULAUX):
        sub = [c for c in cs if c.epi == epi]
        assert {c.N % 4 for c in sub} == {0, 2} and {c.ldo_pad for c in sub} == {0, 4, 8}
        assert {c.K // 64 for c in sub if c.K // 64 in (3, 5, 7) and not c.colsum} == {3, 5, 7}         # split-K under every exact epilogue
        assert any(c.M <= 64 for c in sub) and any(c.M > 192 for c in sub)
    f32 = [c for c in cs if c.epi == G.EPI_F32]
    assert {c.ldo2_pad for c in f32 if c.out2} == {0, 4, 8}
    assert any(c.omap and c.omap[0] < 128 and c.rowmod == 40 and c.M in (120, 200) for c in f32)      # group boundary inside a tile, period 40
    assert any(c.omap and c.omap[0] >= 192 and c.M > c.omap[0] for c in f32)                          # the 192 kernel's one-wrap row map
    assert any(c.omap and c.N % 4 for c in f32) and any(c.out_scale and c.N % 4 for c in f32)
    assert any(c.colsum and c.M == 200 for c in cs) and any(c.colsum for c in G.GELU_CASES)
    mul = [c for c in cs if c.epi == G.EPI_MULAUX and c.N % 4 == 0 and not c.colsum]              # MULAUX at an aligned N off the 192 kernel
    assert any(c.M <= 64 and c.K // 64 in (3, 5, 7) for c in mul) and any(c.M > 128 for c in mul)
    assert {(t, s) for t, s, f in G.RANDOM_PATHS if f == "tiles"} == {(t, 1) for t in (1, 16, 2, 6, 0)} | {(t, s) for t in (1, 16) for s in (2, 3, 8)}
    assert {(t, s) for t, s, f in G.RANDOM_PATHS if f == "skinny"} == {(7, 1), (0, 1)} and all(len(v) == 3 for v in G.RANDOM_SHAPES.values())
    assert {K // 64 for _, _, K in G.RANDOM_SHAPES["tiles"]} == {3, 5, 7}
    assert {c.epi for c in G.GELU_CASES} == set(G.GELU_EPIS)
    for c in ALL_NT:
        assert not c.rowmod or c.N % 4 == 0
        assert not c.colsum or (c.N % 4 == 0 and c.epi in (G.EPI_DGELU, G.EPI_MULAUX))
        tiles = {t for t, s in G.nt_paths(c) if s == 1}
        assert tiles == ({2, 6, 0, 1} if c.colsum else {1, 16, 2, 6, 0, 7} if c.M <= 64 else {1, 16, 2, 6, 0})
        if c.K // 64 in (3, 5, 7) and not c.colsum:
            assert {(t, min(s, c.K // 64)) for t, s in G.nt_paths(c) if s > 1} == {(t, s) for t in (1, 16) for s in {2, 3, c.K // 64}}
    assert len({c.name for c in ALL_NT}) == len(ALL_NT)


@pytest.mark.parametrize("c", G.NT_CASES, ids=lambda c: c.name)
def test_exact_cases_round_and_do_not_round(c):
    """at least a quarter of every bf16-rounded quantity needs rounding, at least a quarter is representable; ties to even occur"""
    ref = G.nt_reference(c)                      # (asserts fp32 exactness of every expected value itself)
    for need, ok in G.shares(ref):
        assert need >= 0.25 and ok >= 0.25, (c.name, need, ok)
    if c.epi != G.EPI_F32 or c.round_bf16 or c.out2:
        assert ref["pre_round"]


def test_some_exact_case_holds_a_tie_to_even():
    ties = 0
    for c in G.NT_CASES:
        for q in G.nt_reference(c)["pre_round"]:
            r = G.rbf(q)
            half_ulp = (q.frexp()[1].double() - 9).exp2()          # |q| = m 2^e, m in [0.5, 1): a bf16 ulp at q is 2^(e - 8)
            ties += int(((q != r) & ((q - r).abs() == half_ulp)).sum())
    assert ties > 100


def test_gelu_floor_is_the_measured_one():
    fl = G.gelu_floor()
    for k in ("gelu", "grad"):
        assert abs(fl[k] - G.GELU_FLOOR_DOC[k]) <= 0.1 * G.GELU_FLOOR_DOC[k], (k, fl[k])
        assert 1e-7 < fl[k] < 2.0 ** -17          # far below a bf16 ulp of the outputs: the bar stays a bf16 rounding plus noise
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    xg = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xg).sum().backward()
    assert float((G.gelu64(x) - torch.nn.functional.gelu(x)).abs().max()) < 1e-14 and float((G.gelu_grad64(x) - xg.grad).abs().max()) < 1e-14


@pytest.mark.parametrize("c", G.GELU_CASES, ids=lambda c: c.name)
def test_gelu_cases_have_an_exact_pre_activation_that_covers_the_range(c):
    ref = G.nt_reference(c)                      # asserts that acc + bias is bf16-representable
    h = ref["h"]
    hist = torch.histc(h.float(), bins=24 if c.M * c.N >= 4000 else 12, min=-6, max=6)      # half-unit bins; unit bins for the two small cases
    assert float(h.std()) > 1.5 and bool((hist > 0).all()), hist
    if c.epi == G.EPI_DGELU:
        aux = G.nt_inputs(c.name)["aux"]
        assert bool(G.is_bf16(aux).all()) and float(aux.abs().max()) <= 8.0
    # the fp32 restatement of the kernel's arithmetic sits inside the bar (so a correct kernel passes)
    h32 = h.float()
    if c.epi == G.EPI_GELU:
        got = {"out2": G.gelu32(h32)}
    elif c.epi == G.EPI_GELU_GRAD:
        got = {"out": G.gelu_grad32(h32), "out2": G.gelu32(h32)}
    else:
        got = {"out": h32 * G.gelu_grad32(G.nt_inputs(c.name)["aux"].float())}
    for k, v in got.items():
        err = (v.to(torch.bfloat16).double() - ref[k]["exp"]).abs()
        assert bool((err <= ref[k]["bar"]).all()), (c.name, k, float((err / ref[k]["bar"]).max()))


def test_every_mutant_is_caught_by_every_case_it_applies_to():
    pairs, missed = 0, set()
    kinds = set()
    for c in ALL_NT:
        ref = G.nt_reference(c)
        for m in G.nt_mutants(c):
            pairs += 1
            kinds.add(m[0])
            if not G.caught(ref, G.nt_reference(c, mut=m)):
                missed.add((c.name, G.mutant_id(m)))
    assert kinds == {"ktile_drop", "row_clamp", "col_clamp", "last4_drop", "last4_prev", "bias_shift4", "residual_no_omap", "rowmod_period",
                     "round_after_residual", "scale_skipped", "out2_before_scale", "corner_transposed", "splitk_drop"}
    assert missed == set(G.EXEMPT), (missed - set(G.EXEMPT), set(G.EXEMPT) - missed)     # the table is exact: nothing else exempt, every entry in use
    assert len(G.EXEMPT) <= 0.05 * pairs
    assert all(isinstance(r, str) and r for r in G.EXEMPT.values())


@pytest.mark.parametrize("c", ALL_NT, ids=lambda c: c.name)
def test_the_gpu_assertion_passes_the_reference_and_fails_every_mutant_and_every_stray_store(c):
    """check_nt, which the GPU test applies to the kernel's output allocations, on simulated allocations"""
    ref = G.nt_reference(c)
    G.check_nt(c, ref, G.simulate_nt(c, ref), c.name)
    for m in G.nt_mutants(c):
        if (c.name, G.mutant_id(m)) not in G.EXEMPT:
            with pytest.raises(AssertionError):
                G.check_nt(c, ref, G.simulate_nt(c, G.nt_reference(c, mut=m)), c.name)
    for name in [k for k in ("out", "out2", "colsum") if k in ref or (k == "colsum" and c.colsum)]:
        got = G.simulate_nt(c, ref)
        alloc = got[name]
        width = c.N
        for i in ((alloc.shape[0] - 1, 0),) + (((0, width),) if alloc.shape[1] > width else ()):     # the row behind the view, the column behind N
            hit = {k: v.clone() for k, v in got.items()}
            hit[name][i] = 1.0
            with pytest.raises(AssertionError, match="outside the addressed part"):
                G.check_nt(c, ref, hit, c.name)
    if c.omap:                                                   # a row between two groups of the row map
        rows = set(G.out_rows_of(c)[0].tolist())
        gap = next(r for r in range(max(rows)) if r not in rows)
        hit = G.simulate_nt(c, ref)
        hit["out"][gap, 0] = 1.0
        with pytest.raises(AssertionError, match="outside the addressed part"):
            G.check_nt(c, ref, hit, c.name)


def test_reference_is_caught_by_nothing_and_poison_is_where_claimed():
    for c in ALL_NT:
        ref = G.nt_reference(c)
        assert not G.caught(ref, G.nt_reference(c))
        b = G.nt_buffers(c.name)
        for name in ("A", "B", "aux", "residual", "rowmod"):
            if name in b:
                buf, r, k = b[name]
                assert not buf[:r, :k].isnan().any() and buf[r:].isnan().all() and (buf.shape[1] == k or buf[:, k:].isnan().all())
                assert buf.shape[0] > r
        for name in ("A", "B", "aux", "residual"):
            if name in b:
                assert b[name][0].shape[1] > b[name][2]                  # a padded stride on every operand that has one
        if c.bias:
            buf, _, n = b["bias"]
            assert not buf[:n].isnan().any() and buf[n:].isnan().all() and buf.numel() > n
        for name in ("out", "out2", "colsum"):
            if name in b:
                buf = b[name][0]
                assert torch.equal(G.bits(buf), G.bits(G.sentinel(buf.shape, buf.dtype))) and buf.isnan().all() and buf.shape[0] > b[name][1]
        rows, orows = G.out_rows_of(c)
        assert len(set(rows.tolist())) == c.M and orows > int(rows.max()) and (c.omap is None or orows > c.M)
        # operands are what bf16 holds
        d = G.nt_inputs(c.name)
        assert bool(G.is_bf16(d["A"]).all()) and bool(G.is_bf16(d["B"]).all())


def test_random_bound_holds_for_fp32_accumulation_and_not_for_bf16():
    for M, N, K in G.RANDOM_SHAPES["tiles"][:1] + G.RANDOM_SHAPES["skinny"][:1]:
        for std in G.RANDOM_STDS:
            r = G.random_case(M, N, K, std)
            acc32 = torch.zeros(M, N)
            accb = torch.zeros(M, N, dtype=torch.bfloat16)
            for t in range(K // 32):          # fp32 accumulation in MFMA-sized steps, and the same with a bf16 accumulator
                part = r["A"][:, t * 32:(t + 1) * 32].float() @ r["B"][:, t * 32:(t + 1) * 32].float().t()
                acc32 += part
                accb = (accb.float() + part).to(torch.bfloat16)
            assert bool(((acc32.double() - r["ref"]).abs() <= r["bound32"]).all())
            assert bool(((acc32.to(torch.bfloat16).double() - r["ref"]).abs() <= r["bound16"]).all())
            assert not bool(((accb.double() - r["ref"]).abs() <= r["bound16"]).all())


# ------------------------------------------------------------------------------------------------ TN
def test_tn_axes_and_mutants():
    cs = G.TN_CASES
    assert {c.M for c in cs} == {64, 128, 320} and {(c.P, c.Q) for c in cs} == {(8, 8), (136, 200), (192, 392)}
    assert {c.p_lim for c in cs} == {None, 24, 21, 1} and {c.q_lim for c in cs} == {None, 24, 21, 1}
    assert {c.ldo for c in cs} == {"Q", "lim4", "odd"} and {c.perm for c in cs} == {True, False}
    assert any(G.tn_dims(c)[2] % 4 for c in cs) and any(G.tn_dims(c)[1] % 4 and G.tn_dims(c)[2] % 4 == 0 for c in cs)
    tiles = [((pl + 127) // 128) * ((ql + 127) // 128) for pl, ql, _, _ in map(G.tn_dims, G.TN_GROUP)]
    assert len(set(tiles)) == 4 and tiles == sorted(tiles, reverse=True)
    kinds = set()
    for c in cs:
        ref = G.tn_reference(c)
        pl, ql, ldo, orows = G.tn_dims(c)
        d = G.tn_inputs(c.name)
        rows = d["perm"].long() if c.perm else torch.arange(pl)
        assert len(set(rows.tolist())) == pl and int(rows.max()) < orows
        assert int((G.bits(ref) != G.SENT32).sum()) == pl * ql
        for m in G.tn_mutants(c):
            kinds.add(m[0])
            assert not torch.equal(G.bits(ref), G.bits(G.tn_reference(c, m))), (c.name, m)
        b = G.tn_buffers(c.name)
        for name, cols in (("A", c.P), ("B", c.Q)):
            buf = b[name][0]
            assert buf.shape[1] > cols and buf[:, cols:].isnan().all() and buf[c.M:].isnan().all() and not buf[:c.M, :cols].isnan().any()
    assert kinds == {"mtile_drop", "row_short", "col_short", "row_extra", "col_extra", "perm_ignored"}


# ------------------------------------------------------------------------------------------------ decode
def test_decode_axes():
    cs = G.DECODE_CASES
    assert {c.M for c in cs} == {1, 16, 17, 32, 33, 64} and {c.K for c in cs} == {128, 384, 1024} and {c.N for c in cs} == {16, 48, 512}
    for M in (1, 16, 17, 32, 33, 64):
        assert {(c.mode, c.norm) for c in cs if c.M == M} == {(m, n) for m in (0, 1, 2) for n in (True, False)}
    assert {c.mode for c in cs if c.K == 128} == {0, 1, 2}
    assert {(c.mode, c.norm) for c in cs if c.ldo_pad} == {(m, n) for m in (0, 1, 2) for n in (True, False)}


@pytest.mark.parametrize("c", G.DECODE_CASES, ids=lambda c: c.name)
def test_decode_operand_is_exact_and_mutants_are_caught(c):
    d = G.decode_inputs(c.name)
    if c.norm:
        for ulps in (-4, -1, 0, 1, 4):          # the normalised bf16 operand is +-w whatever the last bits of the hardware rsqrt
            assert torch.equal(G.decode_operand32(d["x"], d["norm_w"], ulps), d["xn"]), ulps
    else:
        assert bool(G.is_bf16(d["x"]).all())
    assert bool(G.is_bf16(d["W"]).all())
    exp, bar = G.decode_reference(c)
    for m in G.decode_mutants(c):
        mexp, _ = G.decode_reference(c, m)
        if bar is None:
            assert not torch.equal(exp, mexp), m
        else:
            assert bool(((exp - mexp).abs() >= 32 * bar).any()), m
    if c.mode == 1:                              # the gate reaches both tails of silu and its middle
        a = (d["xn"] @ d["W"].t()).view(c.M, c.N // 16, 2, 8)[:, :, 1]
        assert float(a.min()) < -1 and float(a.max()) > 1 and bool((a.abs() < 1).any())
        # the kernel's rounding points in fp32 sit inside the bar
        val, gate = (d["xn"] @ d["W"].t()).view(c.M, c.N // 16, 2, 8).unbind(2)
        val, gate = val.reshape(c.M, -1).float(), gate.reshape(c.M, -1).float()
        s = (gate / (1.0 + torch.exp(-gate))).to(torch.bfloat16).float()
        assert bool((((s * val).to(torch.bfloat16).double() - exp).abs() <= bar).all())
