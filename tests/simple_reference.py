"""CPU restatement of `autoencoder_convpatchify_simplytransformer` (models/model_new/autoencoder.py:418-497) for the tests: the block
and stack of base/simpletransformer.py (`Attn` with rotary q / k :26-72, `Block` :74-87, `ResidualAttentionBlock1` with its final
LayerNorm :89-121), `Encoder3` / `Decoder3` (base/blocks.py:162-288) and the model.  Built on oracle/titok_oracle.py (rotary angles,
apply_rotary, FSQ, the conv-transpose rows) and oracle/larp_oracle.py (`linear`, `patchify`, `_rb`, `gelu_erf`) -- imported, not edited.
Also the deterministic inputs of the reference-piece fixtures (tests/golden/make_golden_simple.py writes their outputs).
TEST INFRASTRUCTURE ONLY.

`emu=True` rounds to bf16 where the HIP path materialises bf16 tensors: the qkv and fc1 Linear outputs, the rotated q / k
(`apply_rotary_emb(...).type_as(x)` on the bf16 qkv), the attention output, gelu(u), and the operands of every Linear.  As in
oracle/larp_oracle.py::block the proj and fc2 outputs are NOT rounded: the engine adds bias and residual in the fp32 epilogue of those
GEMMs (autocast would round the branch to bf16 first; the difference is below the bars and inside the emu-vs-fp32 gap they are derived from).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import inputs as gen
from oracle import titok_oracle as T
from oracle.larp_oracle import _rb, gelu_erf, linear, patchify

LEVELS = (8, 8, 8, 5, 5, 5)
NAME = "autoencoder_convpatchify_simplytransformer"
# seeds of the whole-model GPU test (tests/test_simple_gpu.py::test_model_matches_restatement) and of its FSQ-flip guard
# (tests/test_simple_cpu.py::test_fsq_flip_guard_of_the_gpu_model_test, which says how the video seed was picked)
MODEL_SEED, VIDEO_SEED = 1301, 1624
# yaml-style constructor arguments; like the reference, the model ignores every one of them
YAML_ARGS = {"bottleneck": None, "prior_model": None, "num_latent_tokens": 1024, "input_size": 128, "frame_num": 16, "temporal_patch_size": 4,
             "patch_size": 8, "decoder_temporal_patch_size": 4, "decoder_patch_size": 8, "in_channels": 3,
             "transformer_name": "transformer_encoder_parallel", "encoder_hidden_size": 768, "decoder_hidden_size": 768, "encoder_num_heads": 12,
             "decoder_num_heads": 12, "encoder_depth": 6, "decoder_depth": 6, "latent_pe_scale_factor": 10000, "query_init_std": 0.02,
             "encoder_query_gaussian_init": True, "learned_decoder_latent_pe": False}


# ------------------------------------------------------------------------------------------ simpletransformer.py
def attention(x, p, pre, heads, angles, emu=False):
    """Attn.forward (:39-72): bias-free qkv -> [B, N, 3, H, hd]; rotary on q and k; softmax(q k^T / sqrt(hd)) v; proj"""
    b, n, d = x.shape
    hd = d // heads
    q, k, v = linear(x, p[pre + "qkv.weight"], None, emu).reshape(b, n, 3, heads, hd).unbind(2)
    q, k = _rb(T.apply_rotary(q, angles), emu), _rb(T.apply_rotary(k, angles), emu)
    att = torch.softmax(torch.einsum("blhd,bmhd->bhlm", q, k) * (hd ** -0.5), dim=-1)
    o = _rb(torch.einsum("bhlm,bmhd->blhd", att, v), emu).reshape(b, n, d)
    return linear(o, p[pre + "proj.weight"], p[pre + "proj.bias"], emu, round_out=False)


def block(x, p, pre, heads, angles, emu=False):
    """Block.forward (:84-87), LayerNorm eps 1e-5, erf GELU, dropouts at p = 0"""
    d = x.shape[-1]
    h = F.layer_norm(x, (d,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], 1e-5)
    x = x + attention(h, p, pre + "attn.", heads, angles, emu)
    h = F.layer_norm(x, (d,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], 1e-5)
    g = _rb(gelu_erf(linear(h, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], emu)), emu)
    return x + linear(g, p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"], emu, round_out=False)


def blocks_only(x, p, pre, layers, heads, angles, emu=False):
    for i in range(layers):
        x = block(x, p, f"{pre}blocks.{i}.", heads, angles, emu)
    return x


def stack(x, p, pre, layers, heads, angles, emu=False, keep=None):
    """ResidualAttentionBlock1.forward (:116-121); `keep`: the rows of every sequence the caller goes on with (LayerNorm is row-wise)"""
    x = blocks_only(x, p, pre, layers, heads, angles, emu)
    if keep is not None:
        x = x[:, keep]
    d = x.shape[-1]
    return F.layer_norm(x, (d,), p[pre + "norm.weight"], p[pre + "norm.bias"], 1e-5)


# ------------------------------------------------------------------------------------------ blocks.py / autoencoder.py
def _tap(taps, name, t):
    if taps is not None and t.requires_grad:
        t.retain_grad()
        taps[name] = t
    return t


def encoder3(p, pre, video, cfg, emu=False, taps=None):
    """Encoder3.forward (blocks.py:204-223).  `taps` (a dict) receives the expanded [B, rows, W] mask-token tensor under the parameter's
    name, gradient retained.  The scalar mask token shifts whole rows by a constant and the stream is only ever read through LayerNorms,
    which ignore such a shift: its exact gradient is 0 and what is computed is the rounding residue of a sum over B * rows * W entries --
    to be judged against the size of the summed entries, not against itself."""
    b = video.shape[0]
    width, heads, layers, n_lat = cfg["width"], cfg["heads"], cfg["layers"], cfg["tokens"]
    ang = T.rope_angles(n_lat, cfg["grid"], width // heads)
    w = p[pre + "proj_in.weight"]
    tok = linear(patchify(video, cfg["patch"][0], cfg["patch"][1]), w.reshape(width, -1), p[pre + "proj_in.bias"], emu)
    x = torch.cat([_tap(taps, pre + "mask_token", p[pre + "mask_token"].expand(b, n_lat, width)), tok], dim=1)
    x = stack(x, p, pre + "model_layers.", layers, heads, ang, emu, keep=slice(0, n_lat))
    return linear(x, p[pre + "proj_out.weight"], p[pre + "proj_out.bias"], emu)


def decoder3(p, pre, codes, cfg, emu=False, taps=None):
    """Decoder3.forward (blocks.py:268-288); `taps` as encoder3"""
    b = codes.shape[0]
    width, heads, layers, n_lat = cfg["width"], cfg["heads"], cfg["layers"], cfg["tokens"]
    ang = T.rope_angles(n_lat, cfg["grid"], width // heads)
    y = linear(codes, p[pre + "proj_in.weight"], p[pre + "proj_in.bias"], emu)
    y = torch.cat([y, _tap(taps, pre + "mask_token", p[pre + "mask_token"].expand(b, math.prod(cfg["grid"]), width))], dim=1)
    y = stack(y, p, pre + "model_layers.", layers, heads, ang, emu, keep=slice(n_lat, None))
    return T.conv_transpose_patch(y, p[pre + "proj_out.weight"], p[pre + "proj_out.bias"], cfg["patch"], cfg["grid"], emu)


def model_forward(p, cfg, video, emu=False, force_codes=None, taps=None):
    """AutoEncoder.forward (autoencoder.py:479-497); `force_codes` as titok_oracle.autoencoder_forward: the device's codes go through
    the decoder, the gradient still flows into the encoder through the straight-through form"""
    z = encoder3(p, "encoder.", video, cfg, emu, taps)
    codes, idx, bounded = T.fsq(z, cfg["levels"])
    if force_codes is not None:
        codes = codes + (force_codes - codes).detach()
    return {"pred_frames": decoder3(p, "decoder.", codes, cfg, emu, taps), "z": z, "codes": codes, "indices": idx, "bounded": bounded}


# ------------------------------------------------------------------------------------------ deterministic weights
def make_cfg(size="base", frames=8, side=32, patch=(4, 8, 8), tokens=32):
    return T.make_cfg(size, frames=frames, side=side, patch=patch, tokens=tokens, levels=LEVELS)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def init_stack_state_dict(width, layers, seed, pre=""):
    """weights of one ResidualAttentionBlock1 in the reference's key order; distributions follow init_weights (trunc-normal 0.02 Linear
    weights) except that biases and LayerNorm affine parameters are perturbed so that their gradients and code paths are exercised"""
    s = [seed]

    def nxt():
        s[0] += 1
        return s[0]

    sd = {}
    for i in range(layers):
        b = f"{pre}blocks.{i}."
        sd[b + "norm1.weight"] = _T(1.0 + gen.normal((width,), nxt(), 0.05))
        sd[b + "norm1.bias"] = _T(gen.normal((width,), nxt(), 0.05))
        sd[b + "attn.qkv.weight"] = _T(gen.normal((3 * width, width), nxt(), 0.02))
        sd[b + "attn.proj.weight"] = _T(gen.normal((width, width), nxt(), 0.02))
        sd[b + "attn.proj.bias"] = _T(gen.uniform((width,), nxt(), -0.02, 0.02))
        sd[b + "norm2.weight"] = _T(1.0 + gen.normal((width,), nxt(), 0.05))
        sd[b + "norm2.bias"] = _T(gen.normal((width,), nxt(), 0.05))
        sd[b + "mlp.fc1.weight"] = _T(gen.normal((4 * width, width), nxt(), 0.02))
        sd[b + "mlp.fc1.bias"] = _T(gen.uniform((4 * width,), nxt(), -0.02, 0.02))
        sd[b + "mlp.fc2.weight"] = _T(gen.normal((width, 4 * width), nxt(), 0.02))
        sd[b + "mlp.fc2.bias"] = _T(gen.uniform((width,), nxt(), -0.02, 0.02))
    sd[pre + "norm.weight"] = _T(1.0 + gen.normal((width,), nxt(), 0.05))
    sd[pre + "norm.bias"] = _T(gen.normal((width,), nxt(), 0.05))
    return sd


def init_state_dict(cfg, seed=1301):
    """the model's weights in the reference's state-dict key order (a module's own parameters before its children's)"""
    width, layers = cfg["width"], cfg["layers"]
    pt, ps = cfg["patch"][0], cfg["patch"][1]
    d = len(cfg["levels"])
    sd = {}
    sd["encoder.mask_token"] = _T(gen.normal((1, 1, 1), seed + 1, width ** -0.5))
    sd["encoder.proj_in.weight"] = _T(gen.xavier_uniform((width, 3, pt, ps, ps), seed + 2))
    sd["encoder.proj_in.bias"] = _T(gen.uniform((width,), seed + 3, -0.02, 0.02))
    sd.update(init_stack_state_dict(width, layers, seed + 1000, "encoder.model_layers."))
    sd["encoder.proj_out.weight"] = _T(gen.normal((d, width), seed + 4, 0.05))
    sd["encoder.proj_out.bias"] = _T(gen.uniform((d,), seed + 5, -0.02, 0.02))
    sd["decoder.mask_token"] = _T(gen.normal((1, 1, 1), seed + 6, width ** -0.5))
    sd["decoder.proj_in.weight"] = _T(gen.normal((width, d), seed + 7, 0.05))
    sd["decoder.proj_in.bias"] = _T(gen.uniform((width,), seed + 8, -0.02, 0.02))
    sd.update(init_stack_state_dict(width, layers, seed + 2000, "decoder.model_layers."))
    sd["decoder.proj_out.weight"] = _T(gen.xavier_uniform((width, 3, pt, ps, ps), seed + 9))
    sd["decoder.proj_out.bias"] = _T(gen.uniform((3,), seed + 10, -0.02, 0.02))
    return sd


# ------------------------------------------------------------------------------------------ reference-piece fixtures
# ResidualAttentionBlock1 on its own: B 2, L 64 = 32 latent rows + a [2, 4, 4] grid, width 128, 2 heads, 2 layers
STACK_PIECE = dict(batch=2, tokens=32, grid=[2, 4, 4], width=128, heads=2, layers=2, seed=1400)
SUB = 4     # the four weight-matrix gradients of a block are stored sub-sampled [::SUB, ::SUB] (file size); everything else in full
# Encoder3 / Decoder3: `tiny` (width 256, 4 heads, 4 layers) on 8x32x32 clips, 32 latent tokens
PIECE_CFG = dict(size="tiny", frames=8, side=32, tokens=32)
PIECE_SEED = 1500


def stack_piece_inputs():
    g = STACK_PIECE
    L = g["tokens"] + math.prod(g["grid"])
    return {"x": gen.normal((g["batch"], L, g["width"]), g["seed"] + 500, 1.0), "cot": gen.normal((g["batch"], L, g["width"]), g["seed"] + 501, 1.0)}


def model_piece_inputs():
    cfg = make_cfg(**PIECE_CFG)
    b, d = 2, len(LEVELS)
    grid_n = math.prod(cfg["grid"])
    return {"video": gen.video_clips(b, cfg["frames"], cfg["side"], PIECE_SEED + 1),
            "enc_cot": gen.normal((b, cfg["tokens"], d), PIECE_SEED + 2, 1.0),
            "codes": gen.uniform((b, cfg["tokens"], d), PIECE_SEED + 3, -1.0, 1.0),
            "dec_cot": gen.normal((b, 3, cfg["frames"], cfg["side"], cfg["side"]), PIECE_SEED + 4, 1.0)}


def subsample(name, t):
    """what the fixture stores of gradient `name`: weight matrices of the blocks [::SUB, ::SUB], everything else whole"""
    return t[::SUB, ::SUB] if (t.dim() == 2 and ".blocks." in "." + name) else t
