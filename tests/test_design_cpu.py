"""model_design's CrossAttention layer without a GPU: the torch-CPU restatement of tests/design_reference.py reproduces the fixture the
reference's own code wrote (tests/golden/make_golden_cross.py), the module has the reference's state-dict layout, and CPU tensors
are refused."""
import pytest
import torch

from tests import design_reference as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_reference(golden, case):
    out = R.run_case(case)
    for t in R.TENSORS:
        want = torch.from_numpy(golden[f"{case}/{t}"])
        assert out[t].shape == want.shape
        assert R.rel_l2(out[t], want) <= 1e-5, t


@pytest.mark.parametrize("case", list(R.CASES))
def test_emulated_rounding_lies_where_the_reference_under_autocast_does(golden, case):
    """the restatement with its bf16 rounding points is as far from the fp32 fixture as the reference's own autocast run, within a factor 2"""
    out = R.run_case(case, emulate_bf16=True)
    for t in R.TENSORS:
        d = R.rel_l2(out[t], torch.from_numpy(golden[f"{case}/{t}"]))
        assert d <= 2 * float(golden[f"{case}/{t}_bf16_dist"]), (t, d)


@pytest.mark.parametrize("case", list(R.CASES))
def test_module_has_the_reference_layout(golden, case):
    import video_tokenizer_amd as vt
    c = R.CASES[case]
    m = vt.CrossAttention(c["dim"], c["heads"], c["context_dim"])
    sd = m.state_dict()
    assert tuple(sd) == R.PARAM_NAMES
    for n in R.PARAM_NAMES:
        assert tuple(sd[n].shape) == golden[f"{case}/d_{n}"].shape, n
    assert isinstance(m.norm_q, vt.RMSNorm) and m.norm_q.eps == 1e-6
    assert bool((m.q_norm.weight == 1).all())


def test_constructor_refuses_what_the_kernels_cannot_serve():
    import video_tokenizer_amd as vt
    with pytest.raises(ValueError, match="64 \\* heads"):
        vt.CrossAttention(256, 8)
    with pytest.raises(ValueError, match="RMSNorm widths"):
        vt.CrossAttention(128, 2, context_dim=192)


def test_cpu_tensors_are_refused():
    import video_tokenizer_amd as vt
    m = vt.CrossAttention(128, 2)
    with pytest.raises(vt.hip.HipError, match="GPU tensors only"):
        m(torch.zeros(1, 4, 128), torch.zeros(1, 3, 128))
    with pytest.raises(vt.hip.HipError, match="no stand-alone forward"):
        vt.RMSNorm(128)(torch.zeros(2, 128))
    z = torch.zeros(8, 128, dtype=torch.bfloat16)
    for call in (lambda: vt.hip.attention_cross_fwd(z, z, z, 1, 8, 8, 2), lambda: vt.hip.head_rmsnorm_fwd(z, torch.ones(64), 1e-6, 2),
                 lambda: vt.hip.sigmoid_gate_cols_fwd(z, z), lambda: vt.hip.rmsnorm_any_fwd(z.float(), torch.ones(128), 1e-6)):
        with pytest.raises(vt.hip.HipError, match="GPU tensors only"):
            call()
