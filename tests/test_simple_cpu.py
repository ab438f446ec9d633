"""`autoencoder_convpatchify_simplytransformer` without a GPU: the CPU restatement (tests/simple_reference.py) against outputs of the
reference's own ResidualAttentionBlock1 / Encoder3 / Decoder3 (tests/golden/simple_pieces.npz, made by tests/golden/make_golden_simple.py),
the registry name with the reference's state-dict layout, the host-side argument checks of vt_rope_rotate, and the guard on FSQ code
flips that the GPU test's agreement cap relies on."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import video_tokenizer_amd as vt
from oracle import titok_oracle as T
from tests import simple_reference as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The restatement and the reference evaluate the same formulas in fp32 (the rotary product in float64 here, complex64 there) in a different
# operation order.  A length-K fp32 dot product carries a random-walk error of about sqrt(K) * 2^-24 relative; the longest contraction here is
# K = 1024 (fc2 of the `tiny` pieces) and the path through a 4-block encoder / decoder crosses 4 x 4 + 2 = 18 GEMMs, whose errors add in
# quadrature: sqrt(1024) * 2^-24 * sqrt(18) = 8.1e-6, rounded to 1e-5.  That is still three orders below what a wrong formula or a bf16
# rounding would give (>= 4e-3).  Measured: <= 4.6e-7 on the 2-block stack piece, <= 1.3e-6 on the 4-block encoder / decoder pieces.
FP32_BAR = 1e-5

MODEL_SEED, VIDEO_SEED = S.MODEL_SEED, S.VIDEO_SEED


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "simple_pieces.npz"))


def test_stack_restatement_matches_the_reference_module(ref):
    """ResidualAttentionBlock1 (2 blocks, width 128, 2 heads, B 2, L 64): output, input gradient and every parameter gradient"""
    g = S.STACK_PIECE
    p = {k: v.clone().requires_grad_(True) for k, v in S.init_stack_state_dict(g["width"], g["layers"], g["seed"]).items()}
    I = {k: torch.from_numpy(v) for k, v in S.stack_piece_inputs().items()}
    x = I["x"].clone().requires_grad_(True)
    ang = T.rope_angles(g["tokens"], g["grid"], g["width"] // g["heads"])
    y = S.stack(x, p, "", g["layers"], g["heads"], ang)
    (y * I["cot"]).sum().backward()
    errs = {"out": rel(y, ref["stack_out"]), "dx": rel(x.grad, ref["stack_dx"])}
    for k, q in p.items():
        errs[k] = rel(S.subsample(k, q.grad), ref["stack_d." + k])
    print("stack piece, relative L2 vs the reference:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert len([k for k in ref.files if k.startswith("stack_d.")]) == len(p)
    worst = max((v, k) for k, v in errs.items())
    assert worst[0] < FP32_BAR, worst


def test_encoder3_decoder3_restatement_matches_the_reference_modules(ref):
    """Encoder3 / Decoder3 (`tiny`, 8x32x32 clips, 32 latent tokens): output, input gradient, the gradients of the small parameters
    (LayerNorms, biases; the scalar mask token against the entries its gradient sums)"""
    cfg = S.make_cfg(**S.PIECE_CFG)
    p = {k: v.clone().requires_grad_(True) for k, v in S.init_state_dict(cfg, S.PIECE_SEED).items()}
    I = {k: torch.from_numpy(v) for k, v in S.model_piece_inputs().items()}
    errs, taps = {}, {}
    for tag, fn, xin, cot in (("enc", S.encoder3, I["video"], I["enc_cot"]), ("dec", S.decoder3, I["codes"], I["dec_cot"])):
        x = xin.clone().requires_grad_(True)
        y = fn(p, tag + "oder.", x, cfg, taps=taps)
        (y * cot).sum().backward()
        errs[tag + "_out"], errs[tag + "_dx"] = rel(y, ref[tag + "_out"]), rel(x.grad, ref[tag + "_dx"])
        names = [k for k in ref.files if k.startswith(tag + "_d.")]
        assert len(names) >= 30
        for k in names:
            name = tag + "oder." + k[len(tag) + 3:]
            if name in taps:      # scalar mask token: exact gradient 0 (see S.encoder3), both sides hold the rounding residue of the same sum
                assert abs(float(p[name].grad) - float(ref[k].reshape(()))) < FP32_BAR * float(taps[name].grad.abs().sum()), (name, float(p[name].grad), float(ref[k].reshape(())))
            else:
                errs[k] = rel(p[name].grad, ref[k])
    worst = max((v, k) for k, v in errs.items())
    print("encoder / decoder pieces, relative L2 vs the reference:", {k: f"{errs[k]:.1e}" for k in ("enc_out", "enc_dx", "dec_out", "dec_dx")},
          "worst", worst)
    assert worst[0] < FP32_BAR, worst


def test_registry_name_builds_with_the_reference_layout(ref):
    """vt.make resolves the name on the CPU with the yaml-style arguments (all ignored, as in the reference); state-dict keys, order,
    shapes and the parameter count equal the reference's; a dict with those keys loads strictly"""
    assert S.NAME in vt.models
    m = vt.make({"name": S.NAME, "args": dict(S.YAML_ARGS)})
    layout = json.loads(str(ref["layout"]))
    sd = m.state_dict()
    assert list(sd) == list(layout)
    assert {k: list(v.shape) for k, v in sd.items()} == layout
    assert sum(q.numel() for q in m.parameters()) == int(ref["n_params"])
    assert not any("freqs" in k for k in sd) and tuple(sd["encoder.mask_token"].shape) == (1, 1, 1)
    m.load_state_dict({k: torch.zeros(s) for k, s in layout.items()}, strict=True)
    assert m.prior_model is None and m.output_format == "bcthw" and m.quantize.levels == (8, 8, 8, 5, 5, 5)
    assert len(m.encoder.model_layers.blocks) == 12 == len(m.decoder.model_layers.blocks) and m.encoder.width == 768 and m.encoder.heads == 12
    assert m.encoder.out_tokens == 1024 == m.decoder.in_tokens and m.encoder.grid == [4, 16, 16] and m.decoder.grid_size == 1024
    assert tuple(m.decoder.proj_out.weight.shape) == (768, 3, 4, 8, 8) and isinstance(m.decoder.proj_out, torch.nn.ConvTranspose3d)
    for fn in ("encode", "decode", "decode_indices", "forward"):
        assert callable(getattr(m, fn))
    with pytest.raises(vt.hip.HipError):                                       # CPU tensors: no CPU path
        m(torch.zeros(1, 3, 16, 128, 128))


def test_init_weights_and_small_geometry():
    """init_weights as the family (utils.py:44-51): zero Linear biases, unit LayerNorms; `_geometry` shrinks the clip for parity tests and
    the small model's state dict has the restatement's keys and shapes"""
    cfg = S.make_cfg("tiny")
    m = vt.make({"name": S.NAME, "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        in_grid=[cfg["frames"], cfg["side"], cfg["side"]], patch_size=cfg["patch"], tokens=cfg["tokens"], model_size="tiny")}})
    want = S.init_state_dict(cfg)
    assert list(m.state_dict()) == list(want)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}
    b = m.encoder.model_layers.blocks[0]
    assert float(b.attn.proj.bias.detach().abs().sum()) == 0 and float(b.mlp.fc1.bias.detach().abs().sum()) == 0 and b.attn.qkv.bias is None
    assert float(b.norm1.weight.detach().mean()) == 1.0 and float(m.decoder.model_layers.norm.weight.detach().mean()) == 1.0
    assert 0.015 < float(b.mlp.fc2.weight.detach().std()) < 0.025


def _err(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vt_last_error(buf, 512)
    return buf.value


def test_rope_rotate_and_rotary_stack_reject_bad_arguments_on_the_host():
    """null pointers, a row stride that does not cover q and k or is not a multiple of 8, misaligned buffers, a bad conjugate flag and
    empty shapes give -1 and the entry point's name before any launch; the rotary stack calls refuse half a table pair"""
    lib = vt.hip.lib()
    P = ctypes.c_void_p
    fake = P(4096)                     # never dereferenced: every call below fails its host-side checks

    def rot(qkv=fake, ld=3 * 768, M=128, L=64, H=12, cos=fake, sin=fake, conj=0):
        return lib.vt_rope_rotate(qkv, ld, M, L, H, cos, sin, conj, None)

    for kw in (dict(qkv=None), dict(cos=None), dict(sin=None), dict(ld=2 * 768 - 8), dict(ld=3 * 768 + 4), dict(M=0), dict(L=0), dict(H=0),
               dict(conj=2), dict(qkv=P(4104)), dict(cos=P(4100))):
        assert rot(**kw) == -1, kw
        assert b"vt_rope_rotate" in _err(lib), (kw, _err(lib))
    cfg = vt.hip.StackConfig(1, 64, 128, 2, 1)
    h = P()
    assert lib.vt_stack_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        blocks = (vt.hip.BlockTensors * 1)()
        assert lib.vt_stack_forward_rotary(h, blocks, fake, None, fake, fake, fake, None) == -1
        assert b"vt_stack_forward_rotary" in _err(lib)
        assert lib.vt_stack_backward_rotary(h, blocks, None, fake, fake, fake, blocks, fake, 1, None) == -1
        assert b"vt_stack_backward_rotary" in _err(lib)
    finally:
        lib.vt_stack_destroy(h)
    cfg32 = vt.hip.StackConfig(1, 64, 384, 12, 1)                              # head_dim 32: fine for the plain stack, refused with tables
    assert lib.vt_stack_create(ctypes.byref(cfg32), ctypes.byref(h)) == 0
    try:
        assert lib.vt_stack_forward_rotary(h, (vt.hip.BlockTensors * 1)(), fake, fake, fake, fake, fake, None) == -1
        assert b"head_dim 64" in _err(lib)
    finally:
        lib.vt_stack_destroy(h)


def test_fsq_flip_guard_of_the_gpu_model_test():
    """The GPU test lets the device's free-running FSQ indices differ from the bf16-emulating restatement's on up to 0.2 of the entries
    (the family's cap: near-tie roundings flip under any bf16-level perturbation).  The restatement's OWN emu-vs-fp32 flips on that test's
    seeds (weights MODEL_SEED = 1301, video VIDEO_SEED = 1624; base stacks, 12 + 12 blocks, 8x32x32 clips, 32 latent tokens) stay within
    half of that, so the reference side alone does not use up the cap.  The video seed was picked for this: over 1620 .. 1631 the share of
    differing index entries is 0.016 .. 0.109 (one seed above 0.10), at 1624 it is 1 of 64 entries."""
    cfg = S.make_cfg("base")
    sd = S.init_state_dict(cfg, MODEL_SEED)
    from oracle import inputs as gen
    video = torch.from_numpy(gen.video_clips(2, cfg["frames"], cfg["side"], VIDEO_SEED))
    with torch.no_grad():
        a = T.fsq(S.encoder3(sd, "encoder.", video, cfg, emu=True), cfg["levels"])
        b = T.fsq(S.encoder3(sd, "encoder.", video, cfg, emu=False), cfg["levels"])
    share_idx = float((a[1] != b[1]).float().mean())
    share_codes = float((a[0] != b[0]).float().mean())
    print(f"emu vs fp32: {share_idx:.3f} of the {a[1].numel()} index entries, {share_codes:.3f} of the {a[0].numel()} code channels differ")
    assert share_idx <= 0.10 and share_codes <= 0.10
