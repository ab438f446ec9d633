"""The convolution cases of tests/conv3d_cases.py can tell a wrong kernel from a right one: the tap-by-tap references equal torch's own
conv3d and its autograd in float64, the case axes cover what the module claims, every applicable reference mutant is caught (exemption table
exact and capped), the reference alone passes, and the library's host-side validation refuses bad arguments.  CPU only."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import conv3d_cases as K


def test_case_axes_cover_what_the_module_claims():
    cs = K.CASES
    assert {(c.T, c.H, c.W) for c in cs} == {(1, 1, 1), (1, 4, 4), (3, 5, 7), (2, 9, 17), (4, 16, 16), (5, 18, 35)}
    for shape in {(c.T, c.H, c.W) for c in cs}:
        assert {c.stride for c in cs if (c.T, c.H, c.W) == shape} == set(K.STRIDES), shape
    assert {c.B for c in cs} == {1, 2} and {c.res for c in cs} == {False, True}
    assert {(c.cin, c.cout) for c in cs if c.cin_real == c.cin and c.cout_real == c.cout} >= {(16, 16), (16, 32), (32, 32), (64, 128), (128, 64),
                                                                                              (128, 1024), (1024, 128)}
    assert any(c.cin_real == 3 and c.cin == 16 for c in cs) and any(c.cout_real == 3 and c.cout == 16 for c in cs)
    for s in K.STRIDES:
        sub = [c for c in cs if c.stride == s]
        assert {c.H % 2 for c in sub} == {0, 1} and {c.W % 2 for c in sub} == {0, 1} and {c.res for c in sub} == {False, True} and {c.B for c in sub} == {1, 2}
    assert len(K.RANDOM_CASES) == 3 and {c.stride for c in K.RANDOM_CASES} == set(K.STRIDES)


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_references_equal_torch_conv3d_and_its_autograd(c):
    d = K.inputs(c.name)
    x, w = d["x"].clone().requires_grad_(), d["w"].clone().requires_grad_()
    y = F.conv3d(x, w, None, stride=c.stride, padding=1)
    assert torch.equal(y.detach(), K.conv_acc(c, d["x"], d["w"]))
    assert torch.equal(F.conv3d(d["x"].float(), d["w"].float(), None, stride=c.stride, padding=1).double(), y.detach())   # fp32 and float64 agree: exact data
    gx, gw = torch.autograd.grad(y, (x, w), d["dy"])
    assert torch.equal(gx, K.dgrad_acc(c, d["dy"], d["w"]))
    assert torch.equal(gw, K.wgrad_reference(c, d))
    for t in (d["x"], d["w"], d["dy"]) + ((d["res"],) if c.res else ()):
        assert bool(K.rbf(t).eq(t).all())                                      # operands are bf16 values
    assert K.is_f32(d["bias"])


def _caught(kind, c, mutant):
    d = K.inputs(c.name)
    ref = K.REFERENCES[kind]
    return not torch.equal(ref(c, d), ref(c, d, mutant, exact=False))


def test_every_applicable_mutant_is_caught_and_the_exemptions_are_exact():
    pairs, missed = 0, {}
    for kind, mutants in K.MUTANTS.items():
        for m in mutants:
            hit = 0
            for c in K.CASES:
                if not K.applies(m, c):
                    continue
                pairs += 1
                if _caught(kind, c, m):
                    hit += 1
                else:
                    missed[(m, c.name)] = True
            assert hit > 0, f"mutant {m} changes no asserted bit on any case"
    assert set(missed) == set(K.EXEMPT), (sorted(set(missed) - set(K.EXEMPT)), sorted(set(K.EXEMPT) - set(missed)))
    assert len(K.EXEMPT) <= 0.05 * pairs, (len(K.EXEMPT), pairs)


def _simulate(exp, dtype):
    """the allocation a kernel that computes `exp` would leave"""
    a = K.out_alloc(exp.numel(), dtype)
    a[:exp.numel()] = exp.reshape(-1).to(torch.float32).to(dtype)
    return a


def test_the_reference_alone_passes_and_a_mutant_or_a_stray_store_fails():
    c = K.BY_NAME["b2_3x5x7_c16to16_s111"]
    d = K.inputs(c.name)
    exp = K.channels_last(K.fwd_reference(c, d), c.cout).double()
    K.check_alloc(_simulate(exp, torch.bfloat16), exp.numel(), exp, None, c.name)
    bad = K.channels_last(K.fwd_reference(c, d, "tap_drop(13)", exact=False), c.cout).double()
    with pytest.raises(AssertionError):
        K.check_alloc(_simulate(bad, torch.bfloat16), exp.numel(), exp, None, c.name)
    stray = _simulate(exp, torch.bfloat16)
    stray[exp.numel() + 3] = 0.0
    with pytest.raises(AssertionError, match="behind the addressed part"):
        K.check_alloc(stray, exp.numel(), exp, None, c.name)
    dw = K.wgrad_reference(c, d)
    K.check_alloc(_simulate(dw, torch.float32), dw.numel(), dw, None, c.name)
    for r in K.RANDOM_CASES:                       # the float64 value itself, rounded as the kernel rounds, is inside its own bar
        rd = K.random_inputs(r.name)
        for fn, dt in ((K.fwd_bar, torch.bfloat16), (K.dgrad_bar, torch.bfloat16), (K.wgrad_bar, torch.float32)):
            ref, bar = fn(r, rd)
            K.check_alloc(_simulate(ref, dt), ref.numel(), ref, bar, r.name)
            with pytest.raises(AssertionError):
                K.check_alloc(_simulate(ref + 40 * bar + 1e-3, dt), ref.numel(), ref, bar, r.name)


def test_operand_allocations_are_poisoned_behind_the_operand():
    t = torch.ones(2, 3, dtype=torch.bfloat16)
    a = K.poisoned(t)
    assert a.numel() == 6 + K.TAIL and bool(a[6:].isnan().all()) and bool((a[:6] == 1).all())


def _err(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vt_last_error(buf, 512)
    return buf.value.decode()


def test_host_validation_refuses_bad_arguments_without_a_gpu():
    import video_tokenizer_amd as vt
    lib = vt.hip.lib()
    p = 4096                                       # non-null, 16-byte aligned, never dereferenced
    ok = dict(B=1, T=2, H=4, W=4, Cin=16, Cout=32, st=1, sh=2, sw=2)

    def fwd(**over):
        a = dict(ok, **over)
        return lib.vt_conv3d_fwd(over.get("x", p), p, p, None, a["B"], a["T"], a["H"], a["W"], a["Cin"], a["Cout"], a["st"], a["sh"], a["sw"], p, None)

    for over, word in ((dict(Cin=24), "Cin=24"), (dict(Cout=2048), "Cout=2048"), (dict(st=2, sh=1, sw=1), "stride (2,1,1)"), (dict(T=0), "T=0"),
                       (dict(x=None), "null"), (dict(x=4104), "aligned")):
        assert fwd(**over) == -1
        assert "vt_conv3d_fwd" in _err(lib) and word in _err(lib), _err(lib)
    assert lib.vt_conv3d_dgrad(p, p, 1, 2, 4, 4, 16, 20, 1, 1, 1, p, None) == -1 and "vt_conv3d_dgrad" in _err(lib) and "Cout=20" in _err(lib)
    assert lib.vt_conv3d_wgrad(p, p, 1, 2, 4, 4, 16, 32, 1, 1, 1, 33, 16, p, p, None) == -1 and "cout_lim=33" in _err(lib)
    assert lib.vt_conv3d_wgrad(p, p, 1, 2, 4, 4, 16, 32, 1, 1, 1, 32, 16, p, None, None) == -1 and "vt_conv3d_wgrad" in _err(lib)
    assert lib.vt_conv3d_wgrad_workspace_bytes(1, 2, 4, 4, 16, 32, 1, 1, 1, 32, 16) == 2 * 32 * 16 * 27 * 4  # a position tile per frame: two runs
    assert lib.vt_conv3d_pack_weight(p, 3, 3, 16, 8, 0, p, None) == -1 and "cin_abi=8" in _err(lib)
    assert lib.vt_conv3d_packed_elems(16, 16) == 27 * 16 * 32
    assert lib.vt_upsample_nearest_fwd(p, 1, 2, 4, 4, 16, 2, 1, 2, p, None) == -1 and "scale (2,1,2)" in _err(lib)
    assert lib.vt_upsample_nearest_bwd(p, 1, 2, 4, 4, 12, 2, 2, 2, p, None) == -1 and "C=12" in _err(lib)
    assert lib.vt_video_to_channels_last(p, 1, 3, 2, 4, 4, 8, p, None) == -1 and "Cpad=8" in _err(lib)
    assert lib.vt_channels_last_to_video(p, 1, 17, 2, 4, 4, 16, p, None) == -1 and "vt_channels_last_to_video" in _err(lib)
