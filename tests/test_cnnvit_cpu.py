"""video_tokenizer_amd.cnnvit without a GPU: state-dict keys and shapes of Encoder_cnn / Decoder_cnn at the constructor defaults equal the
reference's (stored in the fixture), the constructor keywords and defaults are the reference's, dropout > 0 raises, CPU tensors are refused,
and the fixture is complete and within the size limit."""
import glob
import inspect
import os

import pytest
import torch

import video_tokenizer_amd as vt
from tests import cnnvit_reference as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("stage,cls", [("enc", "Encoder_cnn"), ("dec", "Decoder_cnn")])
def test_state_dict_keys_and_shapes_equal_the_reference(golden, stage, cls):
    with torch.device("meta"):
        sd = getattr(vt.cnnvit, cls)().state_dict()
    assert list(sd) == str(golden[f"default/{stage}/state_dict_keys"]).split("\n")
    assert [",".join(map(str, v.shape)) for v in sd.values()] == str(golden[f"default/{stage}/state_dict_shapes"]).split("\n")


def test_constructor_keywords_and_defaults():
    sig = lambda c: [(p.name, p.default) for p in list(inspect.signature(c.__init__).parameters.values())[1:]]
    assert sig(vt.Encoder_cnn) == [("in_channels", 3), ("ch", 16), ("ch_mult", (1, 2, 4, 4)), ("num_res_blocks", 2), ("norm_type", "group"), ("dropout", 0.0),
                                   ("z_channels", 256), ("use_attn", True)]
    assert sig(vt.Decoder_cnn) == [("z_channels", 256), ("ch", 16), ("ch_mult", (1, 2, 4, 4)), ("num_res_blocks", 2), ("norm_type", "group"), ("dropout", 0.0),
                                   ("out_channels", 3), ("use_attn", True)]
    assert sig(vt.ResnetBlock3D) == [("in_channels", inspect.Parameter.empty), ("out_channels", None), ("conv_shortcut", False), ("dropout", 0.0),
                                     ("norm_type", "group")]
    assert sig(vt.Downsample3D)[2][0] == "stride" and sig(vt.Upsample3D)[1][0] == "scale_factor" and sig(vt.AttnBlock3D)[0][0] == "in_channels"
    blk = vt.ResnetBlock3D(16, 32, conv_shortcut=True)
    assert list(blk.state_dict())[-2:] == ["conv_shortcut.weight", "conv_shortcut.bias"] and tuple(blk.conv_shortcut.kernel_size) == (3, 3, 3)
    assert "nin_shortcut.weight" in vt.ResnetBlock3D(16, 32).state_dict() and "nin_shortcut.weight" not in vt.ResnetBlock3D(16).state_dict()


def test_dropout_raises_and_cpu_tensors_are_refused():
    for make in (lambda: vt.ResnetBlock3D(16, dropout=0.1), lambda: vt.Encoder_cnn(dropout=0.1), lambda: vt.Decoder_cnn(dropout=0.5)):
        with pytest.raises(NotImplementedError, match="dropout"):
            make()
    with pytest.raises(vt.hip.HipError, match="GPU tensors only"):
        vt.ResnetBlock3D(16)(torch.zeros(1, 16, 1, 2, 2))


def test_fixture_is_complete_and_small(golden):
    files = glob.glob(os.path.join(R.GOLDEN, R.PATTERN))
    assert files and all(os.path.getsize(f) < 900_000 for f in files)
    for case, c in R.CASES.items():
        for stage, cls in zip(R.STAGES, (vt.Encoder_cnn, vt.Decoder_cnn)):
            with torch.device("meta"):
                keys = [k for k, _ in cls(**R.ctor(case, stage)).named_parameters()]
            want = {"out", "din"} | {"g:" + k for k in keys if R.stored_grad(case, stage, k)}
            have = {k.split("/", 2)[2] for k in golden if k.startswith(f"{case}/{stage}/") and not k.endswith("_bf16_dist")}
            assert have == want
            assert all(f"{case}/{stage}/{k}_bf16_dist" in golden for k in want)
            if c["grads"] == "all":
                assert len(want) == len(keys) + 2
            else:
                assert all(any(s in k for k in want) for s in ("norm", "conv_in", "conv_out", "res.0.conv1", "sample", "attn.0.q", "mid.1.q", "nin_shortcut"))
    assert tuple(golden["A/enc/out"].shape) == R.latent_shape("A") == (2, 64, 2, 4, 6) and R.latent_shape("B")[2] == 1
