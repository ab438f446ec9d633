"""Host-side surface of `autoencoder_dualpatch` (no GPU): the registry entry and the reference's state-dict keys and shapes, from the fixture
the reference's own code wrote (tests/golden/make_golden_dualpatch.py); the refusals of vt_patchify_dual / vt_unpatchify_dual, which validate
every argument on the host before any launch.

Every library call below is INVALID in exactly one way and must come back with VT_ERR_INVALID and a message that names the entry point:
the pointers are made-up addresses, so a call that got past the validation would launch on them."""
import ctypes

import pytest
import torch

import video_tokenizer_amd as vt
from tests import dualpatch_reference as R

VT_ERR_INVALID = -1
P = 0x7F0000001000            # a 16-byte aligned made-up address; never dereferenced
GOOD = dict(B=2, C=3, T=7, H=16, W=24, T0=1, pt0=1, pt1=3, ph=8, pw=8)


def last_error():
    buf = ctypes.create_string_buffer(512)
    vt.hip.lib().vt_last_error(buf, 512)
    return buf.value.decode()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _keys_and_shapes(sd):
    return list(sd), [",".join(str(d) for d in v.shape) for v in sd.values()]


def call(unpatchify=False, video=P, rows0=P + (1 << 40), rows1=P + (2 << 40), **change):
    g = dict(GOOD, **change)
    sizes = [g[k] for k in ("B", "C", "T", "H", "W", "T0", "pt0", "pt1", "ph", "pw")]
    lib = vt.hip.lib()
    return lib.vt_unpatchify_dual(rows0, rows1, *sizes, video, None) if unpatchify else lib.vt_patchify_dual(video, *sizes, rows0, rows1, None)


REFUSED = {
    "a null video": (dict(video=None), "null"),
    "null rows0": (dict(rows0=None), "null"),
    "null rows1": (dict(rows1=None), "null"),
    "a misaligned video": (dict(video=P + 4), "video"),
    "misaligned rows0": (dict(rows0=P + 8), "rows0"),
    "misaligned rows1": (dict(rows1=P + 2), "rows1"),
    "B = 0": (dict(B=0), "B=0"),
    "C = 0": (dict(C=0), "C=0"),
    "T < 0": (dict(T=-7), "T=-7"),
    "H = 0": (dict(H=0), "H=0"),
    "W = 0": (dict(W=0), "W=0"),
    "pt0 = 0": (dict(pt0=0), "pt0=0"),
    "pt1 = 0": (dict(pt1=0), "pt1=0"),
    "ph = 0": (dict(ph=0), "ph=0"),
    "pw = 0": (dict(pw=0), "pw=0"),
    "T0 = 0": (dict(T0=0), "T0=0"),
    "T0 = T": (dict(T0=7), "T0=7"),
    "T0 > T": (dict(T0=9), "T0=9"),
    "T0 % pt0 != 0": (dict(T=9, T0=3, pt0=2), "T0=3"),
    "(T - T0) % pt1 != 0": (dict(T=8), "T-T0=7"),
    "H % ph != 0": (dict(H=20), "H=20"),
    "W % pw != 0": (dict(W=28), "W=28"),
    "pw % 8 != 0": (dict(pw=4), "pw=4"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_both_entry_points_refuse_and_name_the_value(what):
    change, value = REFUSED[what]
    assert call(**change) == VT_ERR_INVALID, what
    assert "vt_patchify_dual" in last_error() and value in last_error(), last_error()
    assert call(unpatchify=True, **change) == VT_ERR_INVALID, what
    assert "vt_unpatchify_dual" in last_error() and value in last_error(), last_error()


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(vt.hip.HipError):
        vt.hip.patchify_dual(torch.zeros(1, 1, 2, 8, 8), 1, 1, 1, 8, 8, rows0=torch.zeros(1, 64, dtype=torch.bfloat16), rows1=torch.zeros(1, 64, dtype=torch.bfloat16))
    with pytest.raises(vt.hip.HipError):
        vt.hip.unpatchify_dual(torch.zeros(1, 64), torch.zeros(1, 64), 1, 1, 2, 8, 8, 1, 1, 1, 8, 8, video=torch.zeros(1, 1, 2, 8, 8))
    assert vt.hip.dual_grids(16, 128, 128, 1, 1, 3, 8, 8) == (256, 1280)


def test_dualpatch_is_registered_with_the_reference_state_dict(golden):
    assert vt.models["autoencoder_dualpatch"] is vt.AutoEncoderDualPatch is vt.dualpatch.AutoEncoderDualPatch
    with torch.device("meta"):                                              # every keyword of the reference is accepted and ignored
        m = vt.make({"name": "autoencoder_dualpatch", "args": dict(bottleneck=None, prior_model=None, num_latent_tokens=7, input_size=64, frame_num=4,
                                                                    encoder_hidden_size=3, decoder_depth=1, learned_decoder_latent_pe=True, junk="x")})
    keys, shapes = _keys_and_shapes(m.state_dict())
    assert keys == str(golden["model/state_dict_keys"]).split("\n") and shapes == str(golden["model/state_dict_shapes"]).split("\n")
    e, d = m.encoder, m.decoder
    assert (e.width, e.num_layers, e.heads, d.width, d.num_layers, d.heads) == (768, 5, 12, 768, 5, 12)
    assert e.model_layers.ffd_layer[0][3].in_features == 1024
    assert (e.out_tokens, e.first_num_tokens, e.rest_num_tokens, d.in_tokens, d.total_patch_tokens) == (1024, 256, 1280, 1024, 1536)
    assert e.first_patch_embed.weight[0].numel() == 192 and e.rest_patch_embed.weight[0].numel() == 576
    assert m.prior_model is None and m.output_format == "bcthw" and m.quantize.levels == (8, 8, 8, 5, 5, 5)


@pytest.mark.parametrize("case", list(R.CASES))
def test_encoder_and_decoder_have_the_reference_state_dict(golden, case):
    c = R.CASES[case]
    enc = vt.DualPatchEncoder(out_channels=R.TOKEN_SIZE, out_tokens=c["tokens"], _dims=c["dims"], **R.geometry(case))
    dec = vt.DualPatchDecoder(in_channels=R.TOKEN_SIZE, in_tokens=c["tokens"], _dims=c["dims"], **R.geometry(case))
    for stage, m in (("enc", enc), ("dec", dec)):
        keys, shapes = _keys_and_shapes(m.state_dict())
        assert keys == str(golden[f"{case}/{stage}/state_dict_keys"]).split("\n") == list(R.param_shapes(case, stage)), stage
        assert shapes == str(golden[f"{case}/{stage}/state_dict_shapes"]).split("\n"), stage
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage).items()}, strict=True)
    assert (c["tokens"], enc.first_num_tokens, enc.rest_num_tokens) == R.token_counts(case) == {"A": (32, 32, 64), "B": (16, 16, 32)}[case]
    assert enc.first_temporal_grid == 1 == dec.first_temporal_grid        # also where first_frame_temporal_patch is 2 (case B)


def test_init_is_the_reference_s():
    """init_weights + the width**-0.5 normals; the ConvTranspose3d pair keeps torch's default init (it is no nn.Conv3d): its bias is not zeroed"""
    torch.manual_seed(0)
    c = R.CASES["A"]
    enc = vt.DualPatchEncoder(out_tokens=c["tokens"], _dims=c["dims"], **R.geometry("A"))
    dec = vt.DualPatchDecoder(in_tokens=c["tokens"], _dims=c["dims"], **R.geometry("A"))
    assert not enc.first_patch_embed.bias.any() and not enc.rest_patch_embed.bias.any() and not enc.proj_out.bias.any() and not dec.proj_in.bias.any()
    assert dec.first_unpatch.bias.any() and dec.rest_unpatch.bias.any()
    assert 0.015 < float(enc.model_layers.attn_layer[0].to_qkv.weight.detach().std()) < 0.025      # trunc_normal_(std=0.02)
    assert 0.5 < float(enc.rest_pos_embed.detach().std()) * c["dims"][0] ** 0.5 < 1.5


def test_the_first_token_variants_are_not_registered():
    """their constructors in the reference pass patch_size= / in_grid= to this Encoder, which takes neither: a TypeError there"""
    for name in ("autoencoder_first_token", "autoencoder_first_token_res"):
        assert name not in vt.models
        with pytest.raises(KeyError):
            vt.make({"name": name, "args": {}})
