"""model_design's transformer stack and modules on the CPU: the torch restatement of tests/design_stack_reference.py against the fixture the
reference's own code wrote (tests/golden/make_golden_design_stack.py), the rotary tables against the reference's get_freqs, and the registry
entry of the whole model.  No GPU.

  * the restatement matches every fp32 tensor of the fixture to relative L2 1e-5 (the bar of tests/test_design_cpu.py): it IS the reference's
    arithmetic, so the GPU tests may lean on it;
  * with emulate_bf16 it lies within 2 x the reference's own autocast-bf16 distance from its fp32 run (`<tensor>_bf16_dist`): the rounding points
    listed there are the ones autocast has.
"""
import math

import numpy as np
import pytest
import torch

from tests import design_stack_reference as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _compare(got, golden, prefix, emu):
    failures = []
    for t, v in got.items():
        want = torch.from_numpy(golden[f"{prefix}{t}"])
        assert tuple(v.shape) == tuple(want.shape), t
        d = R.rel_l2(v, want)
        bar = 2 * float(golden[f"{prefix}{t}_bf16_dist"]) if emu else 1e-5
        print(f"{'RATIO' if emu else 'FP32'} {prefix}{t} {d:.3e} bar {bar:.3e}")
        if not d <= bar:
            failures.append((t, d, bar))
    assert not failures, failures


@pytest.mark.parametrize("emu", [False, True])
@pytest.mark.parametrize("case", list(R.STACK_CASES))
def test_stack_restatement_matches_the_reference(golden, case, emu):
    got = R.run_stack(case, emulate_bf16=emu)
    assert {f"{case}/{t}" for t in got} == {k for k in golden if k.startswith(case + "/") and not k.endswith("_bf16_dist")}
    _compare(got, golden, case + "/", emu)


@pytest.mark.parametrize("emu", [False, True])
def test_module_restatement_matches_the_reference(golden, emu):
    got = R.run_mod((golden["mod/main_q"], golden["mod/first_q"]), emulate_bf16=emu)
    mods = ("encoder/", "first_frame_encoder/", "decoder/")
    assert set(got) == {k for k in golden if k.startswith(mods) and not k.endswith("_bf16_dist")}
    _compare(got, golden, "", emu)


@pytest.mark.parametrize("case", list(R.STACK_CASES))
def test_rope_tables_are_the_references_get_freqs(golden, case):
    """titok.rope_tables (fp32) against the real and imaginary parts of get_freqs (float64): equal after the one rounding to fp32, up to the last
    bit of the float64 cos / sin of angles below 1e5 (|d angle| <= 1e5 * 2^-52 = 2e-11, far below half an fp32 ulp of 6e-8)"""
    c = R.STACK_CASES[case]
    cos, sin = R.tables(c["tokens"], c["grid"])
    L = c["tokens"] + math.prod(c["grid"])
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (L, 32) == tuple(sin.shape)
    for got, want in ((cos, golden[f"rope/{case}_cos"]), (sin, golden[f"rope/{case}_sin"])):
        assert want.dtype == np.float64 and np.abs(got.numpy().astype(np.float64) - want).max() <= 2.0 ** -24 + 1e-9


def test_autoencoder_design_is_registered_with_the_references_state_dict(golden):
    import video_tokenizer_amd as vt
    assert "autoencoder_design" in vt.models
    m = vt.make({"name": "autoencoder_design", "args": {"bottleneck": {"name": "fsq", "args": {}}, "prior_model": None, "num_latent_tokens": 1024,
                                                          "input_size": 128, "frame_num": 16, "encoder_depth": 6}})
    sd = m.state_dict()
    names = [str(n) for n in golden["state_dict/names"]]
    shapes = [tuple(int(d) for d in str(s).split(",") if d) for s in golden["state_dict/shapes"]]
    assert list(sd.keys()) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    for mod in (m.encoder, m.first_frame_encoder, m.decoder):
        for i, layer in enumerate(mod.transformer.layers):
            scales = [layer.res_scale_sa, layer.res_scale_ffn] + ([layer.res_scale_ca] if layer.has_cross_attn else [])
            for s in scales:
                assert s.dim() == 0 and s.requires_grad and float(s.detach()) == pytest.approx(1.0 / math.sqrt(2 * i + 1), rel=1e-6)
    assert len(m.first_frame_encoder.transformer.layers) == max(len(m.encoder.transformer.layers) // 2, 2)
    assert vt.design.RMSNorm(8).weight.shape == (8,)


def test_layers_refuse_cpu_tensors_and_bad_widths():
    import video_tokenizer_amd as vt
    st = vt.TransformerStack(128, heads=2, mlp_ratio=1, num_layers=1)
    cos, sin = R.tables(4, (1, 2, 2))
    with pytest.raises(vt.hip.HipError, match="GPU tensors only"):
        st(torch.zeros(1, 8, 128), (cos, sin))
    with pytest.raises(ValueError, match="64 \\* heads"):
        vt.SelfAttention(100, 2)
    with pytest.raises(vt.hip.HipError, match="no stand-alone forward"):
        st.layers[0].ffn[2](torch.zeros(2))
