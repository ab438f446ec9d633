"""The power of tests/test_rms_edges_gpu.py, proved on the CPU from the float64 references of tests/rms_cases.py alone (no kernel, no GPU),
as tests/test_gated_cases_cpu.py does for the gated passes.  Per case: every reference mutant is caught by an asserted quantity (ratio >= 4 of
its bar, or the column-sum rule) or named in EXEMPT_MUTANTS; every column sum that is left out is named in NOT_ASSERTED; both tables are
exact.  Per kernel: every mutant is caught by some case.  Every column bar is at least 8 x its noise and at most a quarter of the smallest
deviation it has to catch.  The fp32 replay of every case passes every bar and every share condition, and the two derived floors (rstd,
silu) keep their stated margin over what the replay shows.  With the rounding points switched off every backward reference is
torch.autograd of its forward, at the small shapes.  A case's tensors are dropped once `rms_cases.proof` has its summary."""
import collections

import pytest
import torch

from tests import rms_cases as R

SMALL = [n for n in R.NAMES if not any(n.endswith(e) for e in ("-1029", "-8197", "2049-8", "8193-8", "1025-8", "1640-8", "8193-512", "4100-2048"))
         and not n.startswith(("rope_rotate-4097", "rope_rotate-65537"))]


@pytest.mark.parametrize("name", R.NAMES)
def test_every_mutant_is_caught_by_its_case_or_named(name):
    p = R.proof(name)
    for m, ratios in p["undetected"].items():
        assert (name, m) in R.EXEMPT_MUTANTS, (m, ratios)
    for nm, c in p["cols"].items():
        if c["bar"] is None:
            assert (name, nm) in R.NOT_ASSERTED, (nm, c["noise"])
            continue
        hits = [d for d in c["devs"] if d >= R.DETECT * c["noise"]]
        assert hits and c["bar"] <= min(hits) / 4 * (1 + 1e-12) and c["bar"] >= 8 * c["noise"]


def test_the_exemption_tables_are_exact():
    missed, unasserted = set(), set()
    for name in R.NAMES:
        p = R.proof(name)
        missed |= {(name, m) for m in p["undetected"]}
        unasserted |= {(name, nm) for nm, c in p["cols"].items() if c["bar"] is None}
    assert missed == set(R.EXEMPT_MUTANTS), missed ^ set(R.EXEMPT_MUTANTS)
    assert unasserted == set(R.NOT_ASSERTED), unasserted ^ set(R.NOT_ASSERTED)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_every_mutant_is_caught_by_some_case_of_its_kernel(kernel):
    caught = collections.defaultdict(bool)
    for name in R.names(kernel):
        p = R.proof(name)
        for m in p["mutants"]:
            caught[m] |= m not in p["undetected"]
    assert caught and all(caught.values()), [m for m, ok in caught.items() if not ok]
    assert set(caught) == set(R.ALL_MUTANTS[kernel]), set(caught) ^ set(R.ALL_MUTANTS[kernel])


def test_the_size_mutants_are_caught_at_the_sizes_they_are_for():
    """each cap of the table in the module docstring of tests/test_rms_edges_gpu.py has a case past it that catches the dropped remainder"""
    for name, m in (("rmsnorm-768-8197", "drop_ge8192"), ("rmsnorm_any-128-8197", "drop_ge8192"), ("rmsnorm_any_f32-2560-8197", "drop_ge8192"),
                    ("rmsnorm-2560-1029", "drop_ge1024_dw"), ("rmsnorm_any_f32-128-1029", "drop_ge1024_dx"), ("head_rmsnorm-2049-8", "drop_ge16384"),
                    ("head_rmsnorm-8193-8", "drop_ge65536"), ("qkrms_rope-2-1025-8", "drop_ge16384"), ("qkrms_rope-5-1640-8", "drop_ge65536"),
                    ("rope_rotate-65537-4099-1-0", "drop_rows_ge_cap"), ("rope_rotate-4097-257-16-1", "drop_rows_ge_cap"),
                    ("rope_rotate-19-4-17-0", "drop_pieces_ge256"), ("residual_scale-2049-128", "drop_ge65536x4"),
                    ("residual_scale-8193-512", "drop_ge_fwd_cap"), ("swiglu-4100-2048", "drop_ge1048576")):
        p = R.proof(name)
        assert m in p["mutants"] and m not in p["undetected"], (name, m)


@pytest.mark.parametrize("name", R.NAMES)
def test_the_fp32_replay_passes_every_bar_and_share(name):
    p = R.proof(name)
    for nm, r in p["replay"].items():
        assert r is None or r <= 1.0, (nm, r)
    for nm, s in p["shares"].items():
        assert s <= R.SHARE, (nm, s)
    n, of = p["ambiguous"]                                # elements of a SwiGLU case that accept a second rounding of silu(g): 3 %, or the
    assert n <= max(0.03 * of, 3), (n, of)                # three planted values from -88.5 down, where exp(-g) leaves the fp32 range


def test_the_derived_floors_keep_their_margin():
    """RSQ_REL and SILU_UNITS against what the replay shows, with the margins stated next to the constants"""
    rstd = max(R.proof(n)["rstd"] for n in R.NAMES)
    silu = max(max(R.proof(n)["silu"]) for n in R.NAMES)
    print(f"\nlargest replay distance: rstd {rstd:.3e} relative, silu / silu' {silu:.3f} units")
    assert 0 < R.RSQ_MARGIN * rstd <= R.RSQ_REL <= 2 * R.RSQ_MARGIN * rstd
    assert 0 < R.SILU_MARGIN * silu <= R.SILU_UNITS <= 2 * R.SILU_MARGIN * silu


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("rmsnorm")])
def test_rmsnorm_backward_is_autograd_of_the_forward(name):
    c = R.case(name)
    x = c.x[:c.rows].double().requires_grad_(True)
    w = c.w.double().requires_grad_(True)
    e = c.evaluate(x=x, w=w, pure=True)
    (e["y"] * c.dy[:c.rows].double()).sum().backward()
    dx = e["dx"].detach() - (c.dres[:c.rows].double() if c.has_dres else 0.0)
    assert _close(dx, x.grad) and _close(e["terms"].detach().sum(0), w.grad)


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("head_rmsnorm")])
def test_head_rmsnorm_backward_is_autograd_of_the_forward(name):
    c = R.case(name)
    M, W = c.M, 64 * c.H
    x = c.x[:M, :W].double().requires_grad_(True)
    w = c.w.double().requires_grad_(True)
    e = c.evaluate(rb=R.ident, x=x, w=w)
    (e["y"] * c.dy[:M, :W].double().reshape(M, c.H, 64)).sum().backward()
    assert _close(e["dx"].detach().reshape(M, W), x.grad) and _close(e["terms"].detach().reshape(-1, 64).sum(0), w.grad)


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("qkrms_rope")])
def test_qkrms_rope_backward_is_autograd_of_the_forward(name):
    c = R.case(name)
    M, D = c.M, c.D
    x = torch.nan_to_num(c.backing[:M].double()).requires_grad_(True)
    P = [p.double().requires_grad_(True) for p in c.params]
    e = c.evaluate(rb=R.ident, x=x, params=P)
    gy = torch.stack([c.up_backing[:M].double()[:, i * D:(i + 1) * D].reshape(M, c.H, 64) for i in (0, 1)])
    (e["y"] * gy).sum().backward()
    for i in (0, 1):
        assert _close(e["dx"][i].detach().reshape(M, D), x.grad[:, i * D:(i + 1) * D])
        assert _close(e["terms"][i].detach().reshape(-1, 64).sum(0), P[i].grad)


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("rope_rotate") and n.endswith("-1")])
def test_the_conjugate_rotation_is_autograd_of_the_forward(name):
    c = R.case(name)
    W = 128 * c.H
    x = torch.randn((c.M, W), dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    y, _ = c.evaluate(x=x, conj=0)
    gy = c.qkv[:c.M, :W].double()
    (y * gy).sum().backward()
    assert _close(c.evaluate()[0], x.grad)


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("residual_scale")])
def test_residual_scale_backward_is_autograd_of_the_forward(name):
    c = R.case(name)
    y = c.y[:c.rows].double().requires_grad_(True)
    s = c.scale.double().requires_grad_(True)
    e = c.evaluate(rb=R.ident, y=y, scale=s)
    (e["out"] * c.dout[:c.rows].double()).sum().backward()
    assert _close(e["dy"].detach(), y.grad) and _close(e["terms"].detach().sum(0), s.grad)


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith("swiglu")])
def test_swiglu_backward_is_autograd_of_the_forward(name):
    c = R.case(name)
    h = c.h[:c.M].double().requires_grad_(True)
    (r, _, _), _, _, dy, _ = c.evaluate(rb=R.ident, h=h)
    (r["a"] * dy).sum().backward()
    assert _close(torch.cat([r["dx"], r["dg"]], 1).detach(), h.grad)
