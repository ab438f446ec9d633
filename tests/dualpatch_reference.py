"""Inputs, weights and cases of the `autoencoder_dualpatch` fixture tests/golden/dualpatch_model_*.npz, which the reference's own Encoder and
Decoder (models/model_dualpatch/base/blocks.py:12-258) wrote through tests/golden/make_golden_dualpatch.py.  Plain numpy / torch on the CPU:
importing this module needs no GPU and no built library.

Inputs and weights come from oracle/inputs.py generators, so the fixture holds OUTPUTS only.  Two stages per case, each with its own
cotangent, so that no result depends on which side of a rounding tie a code falls:
  enc: z = encoder(video), loss sum(z * w_z)        -> z, d_video, the parameter gradients
  dec: pred = decoder(codes), loss sum(pred * w_p)  -> pred, d_codes, the parameter gradients
      (codes = the reference's FSQ of the reference's fp32 z, stored in the fixture)."""
import math
import os

import numpy as np
import torch

from oracle import inputs as gen

LEVELS = (8, 8, 8, 5, 5, 5)
TOKEN_SIZE = len(LEVELS)
CHANNELS = 3
CASES = {
    # non-square frames, a one-frame first segment, two layers, inner 352 (padded to 384 in the GEMM operands); every gradient is stored
    "A": dict(dims=(256, 2, 4, 2.0), batch=2, num_frames=7, first_frame_temporal_patch=1, rest_temporal_patch=3, spatial_size=(32, 64),
              spatial_patch_size=(8, 8), tokens=32, seed=7100, small_only=False),
    # square frames, ONE first-segment temporal token built from two frames; the gradients of parameters below SMALL elements only
    "B": dict(dims=(512, 1, 8, 2.0), batch=4, num_frames=8, first_frame_temporal_patch=2, rest_temporal_patch=3, spatial_size=(32, 32),
              spatial_patch_size=(8, 8), tokens=16, seed=7200, small_only=True),
}
STAGES = ("enc", "dec")
SMALL = 20000
SPLIT_BYTES = 300000                                                  # a larger array is stored as row chunks "<key>@<i>of<k>"
GOLDEN_FILES = tuple(f"dualpatch_model_{i:02d}.npz" for i in range(17))   # each below the size limit of a committed file
GEOMETRY_KEYS = ("spatial_patch_size", "first_frame_temporal_patch", "rest_temporal_patch", "num_frames", "spatial_size")


def geometry(case):
    """the constructor keywords of the reference's Encoder / Decoder (and of ours) that set the case's geometry"""
    return {k: CASES[case][k] for k in GEOMETRY_KEYS}


def token_counts(case):
    """(latent tokens, first-segment tokens N0, rest tokens N1)"""
    c = CASES[case]
    grid = (c["spatial_size"][0] // c["spatial_patch_size"][0]) * (c["spatial_size"][1] // c["spatial_patch_size"][1])
    return c["tokens"], grid, (c["num_frames"] - c["first_frame_temporal_patch"]) // c["rest_temporal_patch"] * grid


def inner_dim(dim, mult, mult_of=32):
    inner = int(mult * (2 / 3) * dim)
    return mult_of * ((inner + mult_of - 1) // mult_of)


def video_shape(case):
    c = CASES[case]
    return (c["batch"], CHANNELS, c["num_frames"]) + tuple(c["spatial_size"])


def param_shapes(case, stage):
    """state-dict name -> shape of the reference's Encoder ('enc') / Decoder ('dec') at the case's geometry, in state-dict order"""
    c = CASES[case]
    D, layers, _, ratio = c["dims"]
    inner = inner_dim(D, ratio)
    n, n0, n1 = token_counts(case)
    k0 = (c["first_frame_temporal_patch"],) + tuple(c["spatial_patch_size"])
    k1 = (c["rest_temporal_patch"],) + tuple(c["spatial_patch_size"])
    if stage == "enc":
        out = {"first_pos_embed": (1, n0, D), "rest_pos_embed": (1, n1, D), "latent_queries": (1, n, D),
               "first_patch_embed.weight": (D, CHANNELS) + k0, "first_patch_embed.bias": (D,),
               "rest_patch_embed.weight": (D, CHANNELS) + k1, "rest_patch_embed.bias": (D,)}
    else:
        out = {"latent_pos_embed": (1, n, D), "first_patch_queries": (1, n0, D), "rest_patch_queries": (1, n1, D),
               "proj_in.weight": (D, TOKEN_SIZE), "proj_in.bias": (D,)}
    attn = {"to_qkv.weight": (4 * D, D), "q_norm.weight": (64,), "q_norm.bias": (64,), "k_norm.weight": (64,), "k_norm.bias": (64,),
            "out_proj.weight": (D, D)}
    ffd = {"0.weight": (D,), "0.bias": (D,), "1.weight": (2 * inner, D), "3.weight": (D, inner)}
    for i in range(layers):
        out.update({f"model_layers.attn_layer.{i}.{k}": s for k, s in attn.items()})
    for i in range(layers):
        out.update({f"model_layers.ffd_layer.{i}.{k}": s for k, s in ffd.items()})
    if stage == "enc":
        out.update({"proj_out.weight": (TOKEN_SIZE, D), "proj_out.bias": (TOKEN_SIZE,)})
    else:
        out.update({"first_unpatch.weight": (D, CHANNELS) + k0, "first_unpatch.bias": (CHANNELS,),
                    "rest_unpatch.weight": (D, CHANNELS) + k1, "rest_unpatch.bias": (CHANNELS,)})
    return out


def _is_norm_weight(name):
    return name.endswith(("q_norm.weight", "k_norm.weight", ".0.weight"))


def params(case, stage):
    """the parameters as numpy float32: matrices and conv kernels N(0, 1 / fan_in) (a ConvTranspose3d kernel [width, C, ...] contracts over
    the width), the position tables and queries N(0, 1 / width); biases and LayerNorm affines perturbed away from 0 / 1 (N(0, 0.1^2) around
    them), so that their gradients are exercised"""
    s = CASES[case]["seed"] + (1000 if stage == "dec" else 0)
    out = {}
    for i, (name, shape) in enumerate(param_shapes(case, stage).items()):
        seed = s + 10 + i
        if _is_norm_weight(name):
            out[name] = (1 + gen.normal(shape, seed, 0.1)).astype(np.float32)
        elif len(shape) == 1:
            out[name] = gen.normal(shape, seed, 0.1).astype(np.float32)
        elif "unpatch" in name:
            out[name] = gen.normal(shape, seed, shape[0] ** -0.5).astype(np.float32)
        elif len(shape) == 3:
            out[name] = gen.normal(shape, seed, shape[-1] ** -0.5).astype(np.float32)
        else:
            out[name] = gen.normal(shape, seed, math.prod(shape[1:]) ** -0.5).astype(np.float32)
    return out


def stored_params(case, stage):
    """the parameters whose gradients the fixture holds"""
    return [n for n, s in param_shapes(case, stage).items() if not CASES[case]["small_only"] or math.prod(s) < SMALL]


def tensors(case, stage):
    """the tensor names the fixture holds for (case, stage), each as "<case>/<stage>/<tensor>" (+ "_bf16_dist")"""
    return (("z", "d_video") if stage == "enc" else ("pred", "d_codes")) + tuple("d_" + n for n in stored_params(case, stage))


def video(case):
    return gen.uniform(video_shape(case), CASES[case]["seed"] + 1).astype(np.float32)


def cotangents(case):
    """w_z [B, tokens, 6] and w_p [B, 3, T, H, W]"""
    c = CASES[case]
    return (gen.normal((c["batch"], c["tokens"], TOKEN_SIZE), c["seed"] + 7).astype(np.float32),
            gen.normal(video_shape(case), c["seed"] + 8).astype(np.float32))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def load_golden():
    """the fixture, merged over its files and with the row chunks of large arrays joined again: "<case>/<stage>/<tensor>", "..._bf16_dist",
    "<case>/codes", "<case>/<stage>/state_dict_keys", "<case>/<stage>/state_dict_shapes", "model/state_dict_keys", "model/state_dict_shapes"
    -> numpy"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    raw = {}
    for fn in GOLDEN_FILES:
        with np.load(os.path.join(here, fn)) as z:
            raw.update({k: z[k] for k in z.files})
    out, chunks = {}, {}
    for k, a in raw.items():
        if "@" in k:
            key, part = k.split("@")
            i, n = (int(v) for v in part.split("of"))
            chunks.setdefault(key, [None] * n)[i] = a
        else:
            out[k] = a
    out.update({k: np.concatenate(parts, axis=0) for k, parts in chunks.items()})
    return out
