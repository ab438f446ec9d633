"""`autoencoder_stat` host surface (models/model_stat/autoencoder.py:8-152): registry name and yaml args, stage logic, the
reference's state-dict layout and parameter count (tests/golden/stat_layout.npz), and the host-side argument checks of the two gate
entry points (include/vt_hip.h, csrc/vt_stat.hip).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import video_tokenizer_amd as vt
from tests import stat_reference as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def model():
    return vt.make({"name": "autoencoder_stat", "args": dict(S.YAML_ARGS)})


def test_yaml_args_build_and_stage(model):
    assert "autoencoder_stat" in vt.models
    assert model.prior_model is None and model.output_format == "bcthw"
    assert model.quantize.levels == (8, 8, 8, 5, 5, 5) and model.quantize.codebook_size == 64000
    assert model.encoder.out_tokens == 1280 and model.decoder.in_tokens == 1280 and model.encoder.width == 768
    assert len(model.encoder.model_layers.attn_layer) == 12 and model.encoder.grid == [4, 16, 16]
    assert model.get_stage(-1) == "vanilla" and model.get_stage(0) == "adaptive" and model.get_stage(7) == "adaptive"
    import inspect
    assert "current_epoch" in inspect.signature(model.forward).parameters and "current_epoch" in inspect.signature(model.encode).parameters
    with pytest.raises(vt.hip.HipError):                                       # CPU tensors: no CPU path
        model(torch.zeros(2, 3, 16, 128, 128), current_epoch=0)


def test_state_dict_layout_and_parameter_count_equal_the_reference(model):
    ref = np.load(os.path.join(GOLDEN, "stat_layout.npz"))
    layout = json.loads(str(ref["layout"]))
    sd = model.state_dict()
    assert list(sd) == list(layout)
    assert {k: list(v.shape) for k, v in sd.items()} == layout
    assert sum(p.numel() for p in model.parameters()) == int(ref["n_params"])
    # init_weights as the reference applies it (utils.py:44-51): zero Linear biases, unit LayerNorms
    assert float(model.encoder.prob_head.net[2].bias.detach().abs().sum()) == 0 and float(model.decoder.proj_out.bias.detach().abs().sum()) == 0
    assert float(model.encoder.model_layers.ffd_layer[0][0].weight.detach().mean()) == 1.0


def test_small_geometry_override():
    m = vt.make({"name": "autoencoder_stat", "args": {"bottleneck": None, "prior_model": None,
                                                       "_geometry": dict(in_grid=[8, 32, 32], tokens=32, model_size="tiny")}})
    assert m.encoder.width == 256 and m.encoder.out_tokens == 32 and tuple(m.encoder.proj_in.weight.shape) == (256, 768)
    assert tuple(m.decoder.proj_out.weight.shape) == (768, 256) and tuple(m.encoder.prob_head.net[2].weight.shape) == (1, 256)
    cfg = S.make_cfg("tiny")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in S.init_state_dict(cfg).items()}


def _err(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vt_last_error(buf, 512)
    return buf.value


def test_gate_entry_points_reject_bad_arguments_on_the_host():
    """null pointers, d above FSQ's maximum (16) and bad levels give -1 and the entry point's name, before any launch"""
    lib = vt.hip.lib()
    P = ctypes.c_void_p
    fake = P(4096)                     # never dereferenced: every call below fails its host-side checks
    lv = vt.hip._levels([8, 8, 8, 5, 5, 5])

    def fwd(g=fake, w2=fake, b2=fake, z=fake, M=64, W=768, d=6, levels=lv, mode=vt.hip.STAT_THRESHOLD, probs=fake, mask=fake, codes=fake):
        return lib.vt_stat_gate_forward(g, W, w2, b2, z, M, W, d, levels, mode, 1, None, probs, mask, codes, None, None)

    def bwd(dcodes=fake, z=fake, u=fake, g=fake, M=64, W=768, d=6, levels=lv, dU=fake, dz=fake, ws=fake):
        return lib.vt_stat_gate_backward(dcodes, None, None, z, fake, fake, u, g, W, fake, M, W, d, levels, 1, dU, dz, fake, fake, ws, None)

    bad17 = vt.hip._levels([2] * 17)
    for name, call in (("vt_stat_gate_forward", fwd), ("vt_stat_gate_backward", bwd)):
        cases = [dict(g=None), dict(z=fake, d=17, levels=bad17), dict(levels=vt.hip._levels([8, 1, 8, 5, 5, 5])), dict(W=700), dict(M=0)]
        cases += [dict(probs=None), dict(codes=None), dict(mode=7)] if call is fwd else [dict(u=None), dict(dU=None), dict(ws=None), dict(dcodes=None)]
        for kw in cases:
            assert call(**kw) == -1, (name, kw)
            assert name.encode() in _err(lib), (name, kw, _err(lib))
    assert lib.vt_stat_gate_workspace_bytes(768) >= 769 * 4
