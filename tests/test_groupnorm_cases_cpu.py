"""The GroupNorm cases of tests/groupnorm_cases.py can tell a wrong kernel from a right one: the reference equals torch's own group_norm and
its autograd in float64, the fp32 replay passes every bar, every applicable mutant is caught, the not-asserted table is exact, and the
library's host-side validation refuses bad arguments.  CPU only."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import groupnorm_cases as N


def test_case_axes_cover_what_the_module_claims():
    cs = N.CASES
    assert {c.C // c.G for c in cs} >= {1, 2, 4, 8} and {c.swish for c in cs} == {0, 1} and {c.B for c in cs} == {1, 2}
    assert all(c.P == 105 for c in cs if not c.name.startswith("two_chunks"))
    assert {c.kind for c in cs} == {"two_clips", "offset", "constant"}
    assert sum(c.P * c.C > N.CHUNK_ELEMS for c in cs) == 2 and all(c.P * c.C <= 2 * N.CHUNK_ELEMS for c in cs)
    off = N.inputs("mean16_std_quarter")["x"].double()
    assert abs(float(off.mean()) - 16) < 0.1 and abs(float(off.std()) - 0.25) < 0.05
    two = N.forward(N.BY_NAME["cg2_plain"], N.inputs("cg2_plain"))
    assert float((two["mean"][0] - two["mean"][1]).abs().min()) > 1 and float((two["rstd"][0] / two["rstd"][1]).min()) > 1.5
    const = N.forward(N.BY_NAME["constant"], N.inputs("constant"))
    assert torch.equal(const["rstd"], torch.full_like(const["rstd"], N.EPS ** -0.5))


@pytest.mark.parametrize("c", N.CASES, ids=lambda c: c.name)
def test_reference_equals_torch_group_norm_and_its_autograd(c):
    d = N.inputs(c.name)
    x = d["x"].double().permute(0, 2, 1).clone().requires_grad_()              # [B, C, P]
    ga, be = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    y = F.group_norm(x, c.G, ga, be, N.EPS)
    z = y * torch.sigmoid(y) if c.swish else y
    f = N.forward(c, d)
    assert torch.allclose(z.detach().permute(0, 2, 1), f["y"], rtol=1e-12, atol=1e-12)
    if c.kind != "constant":                                                   # (the saved statistics are fp32 roundings: compare where that is benign)
        gx, gg, gb = torch.autograd.grad(z, (x, ga, be), d["dz"].double().permute(0, 2, 1))
        b = N.backward(c, d)
        scale = float(gx.abs().max())
        assert float((gx.permute(0, 2, 1) - b["dx"]).abs().max()) < 1e-5 * scale
        assert torch.allclose(gg, b["dgamma"], rtol=1e-4, atol=1e-4 * float(gg.abs().max()))
        assert torch.allclose(gb, b["dbeta"], rtol=1e-4, atol=1e-4 * float(gb.abs().max()))


@pytest.mark.parametrize("c", N.CASES, ids=lambda c: c.name)
def test_the_fp32_replay_passes_every_bar(c):
    d, q = N.inputs(c.name), N.bars(c.name)
    got = {**N.forward(c, d, torch.float32), **N.backward(c, d, torch.float32)}
    for name, quant in q.items():
        g = got[name].to(torch.bfloat16) if name in ("y", "dx") else got[name]
        r = quant.ratio(g)
        assert r is None or r <= 1.0, (name, r)


def _worst(c, mutant, fn, names):
    d, q = N.inputs(c.name), N.bars(c.name)
    got = fn(c, d, mutant=mutant)
    return max((q[n].ratio(got[n]) or 0.0) for n in names)


def test_every_applicable_mutant_is_caught_on_every_case_it_applies_to():
    for c in N.CASES:
        for m in N.FWD_MUTANTS:
            if N.applies(m, c):
                assert _worst(c, m, N.forward, ("y", "mean", "rstd")) >= 4.0, (c.name, m, "forward")
        for m in N.BWD_MUTANTS:
            if N.applies(m, c):
                assert _worst(c, m, N.backward, ("dx", "dgamma", "dbeta")) >= 4.0, (c.name, m, "backward")


def test_the_not_asserted_table_is_exact():
    missing = {(c.name, n) for c in N.CASES for n in ("dgamma", "dbeta") if N.bars(c.name)[n].bar is None}
    assert missing == set(N.NOT_ASSERTED), (missing, set(N.NOT_ASSERTED))
    assert len(missing) <= 0.05 * 2 * len(N.CASES)


def test_host_validation_refuses_bad_arguments_without_a_gpu():
    import video_tokenizer_amd as vt
    lib = vt.hip.lib()
    p, buf = 4096, ctypes.create_string_buffer(512)

    def err():
        lib.vt_last_error(buf, 512)
        return buf.value.decode()

    fwd = lambda B=1, P=8, C=32, G=16, swish=1, eps=1e-6, x=p: lib.vt_groupnorm_fwd(x, p, p, eps, B, P, C, G, swish, p, p, p, p, None)
    for kw, word in ((dict(C=24), "C=24"), (dict(G=5), "G=5"), (dict(P=0), "P=0"), (dict(swish=2), "swish=2"), (dict(eps=0.0), "eps=0"), (dict(x=None), "null"),
                     (dict(x=4100), "aligned"), (dict(C=2048), "C=2048")):
        assert fwd(**kw) == -1 and "vt_groupnorm_fwd" in err() and word in err(), err()
    assert lib.vt_groupnorm_bwd(p, p, p, p, p, p, 1, 8, 32, 3, 0, p, p, p, p, None) == -1 and "vt_groupnorm_bwd" in err() and "G=3" in err()
    assert lib.vt_groupnorm_workspace_bytes(2, 105, 32, 16) == 2 * 2 * 1 * 32 * 4 and lib.vt_groupnorm_workspace_bytes(2, 2100, 16, 16) == 2 * 2 * 2 * 16 * 4
