"""Cases, inputs and the fixture loader of the `autoencoder_cnnvit` ends (video_tokenizer_amd.cnnvit: Encoder_cnn, Decoder_cnn).

The fixture tests/golden/cnnvit_ends_*.npz is written by tests/golden/make_golden_cnnvit.py from the reference's own base/cnnvit.py; inputs and
weights come from oracle/inputs.py generators by the functions below, so only OUTPUTS are committed.  Keys:
  <case>/<stage>/<tensor>            the reference's fp32 run: `out`, `din` (the gradient of the stage's input) and `g:<parameter>` for the stored
                                     parameter gradients (case A: all; case B: conv_in, conv_out, one block of each kind, every GroupNorm)
  <case>/<stage>/<tensor>_bf16_dist  relative L2 distance between the reference's torch.autocast('cpu', bfloat16) run and its fp32 run
  default/<stage>/state_dict_keys, state_dict_shapes   of the reference's class at its constructor defaults, built on the meta device
Arrays above SPLIT_BYTES are cut into chunks "<key>@<i>of<k>" along the flattened array; the loader joins them.

Case A: ch=16, ch_mult=(1,1,2,2), z_channels=64, 2 clips of 8x32x48: one channel per group, shortcuts that change the width in both pyramids, H != W.
Case B: ch=32, ch_mult=(1,1,1,2), z_channels=32, 1 clip of 4x16x16: T collapses to 1 at the coarsest level.
(Only len(ch_mult) == 4 is self-consistent in the reference: with fewer levels its decoder upsamples T where its encoder did not.)"""
import glob
import math
import os

import numpy as np

from oracle import inputs as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATTERN = "cnnvit_ends_*.npz"
SPLIT_BYTES, FILE_BYTES = 200_000, 900_000
STAGES = ("enc", "dec")
CASES = {
    "A": dict(ch=16, ch_mult=(1, 1, 2, 2), z_channels=64, B=2, T=8, H=32, W=48, grads="all"),
    "B": dict(ch=32, ch_mult=(1, 1, 1, 2), z_channels=32, B=1, T=4, H=16, W=16, grads="some"),
}
_SEED = {"A": 4100, "B": 4200}


def ctor(case, stage):
    c = CASES[case]
    kw = dict(ch=c["ch"], ch_mult=c["ch_mult"], z_channels=c["z_channels"])
    return kw


def latent_shape(case):
    c = CASES[case]
    return (c["B"], c["z_channels"], (c["T"] + 3) // 4, c["H"] // 8, c["W"] // 8)       # strides (1,2,2), (2,2,2), (2,2,2)


def video_shape(case):
    c = CASES[case]
    return (c["B"], 3, c["T"], c["H"], c["W"])


def stage_input(case, stage):
    return gen.uniform(video_shape(case), _SEED[case] + 1, -1.0, 1.0) if stage == "enc" else gen.normal(latent_shape(case), _SEED[case] + 2)


def cotangent(case, stage):
    return gen.normal(latent_shape(case), _SEED[case] + 3) if stage == "enc" else gen.normal(video_shape(case), _SEED[case] + 4)


def params(case, stage, shapes):
    """values for a state dict of the given {key: shape}: convolution weights N(0, 1 / fan_in), their biases N(0, 0.02^2), GroupNorm weights
    1 + N(0, 0.1^2) and biases N(0, 0.05^2); one seed per key"""
    out = {}
    for i, (k, shp) in enumerate(shapes.items()):
        seed = _SEED[case] + 1000 * (1 + STAGES.index(stage)) + i
        if len(shp) == 5:
            out[k] = gen.normal(shp, seed, 1.0 / math.sqrt(shp[1] * shp[2] * shp[3] * shp[4]))
        elif "norm" in k:
            out[k] = (1.0 + gen.normal(shp, seed, 0.1)) if k.endswith("weight") else gen.normal(shp, seed, 0.05)
        else:
            out[k] = gen.normal(shp, seed, 0.02)
        out[k] = np.ascontiguousarray(out[k], dtype=np.float32)
    return out


def stored_grad(case, stage, key):
    """whether the gradient of parameter `key` is in the fixture"""
    if CASES[case]["grads"] == "all":
        return True
    if "norm" in key or key.startswith(("conv_in.", "conv_out.")):
        return True
    kinds = ("conv_blocks.0.res.0.", "conv_blocks.0.downsample.", "conv_blocks.0.upsample.", "conv_blocks.3.res.0." if stage == "enc" else "conv_blocks.1.res.0.",
             "mid.1.", "conv_blocks.3.attn.0." if stage == "enc" else "conv_blocks.0.attn.0.")
    return key.startswith(kinds)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def write_golden(arrays):
    """deal `arrays` (key -> ndarray) to cnnvit_ends_<i>.npz files below FILE_BYTES each, big ones in chunks"""
    for f in glob.glob(os.path.join(GOLDEN, PATTERN)):
        os.remove(f)
    pieces = []
    for k, v in arrays.items():
        v = np.asarray(v)
        if v.nbytes <= SPLIT_BYTES or v.dtype.kind not in "fi":
            pieces.append((k, v))
            continue
        flat, n = v.reshape(-1), -(-v.nbytes // SPLIT_BYTES)
        pieces.append((k + "@shape", np.asarray(v.shape, dtype=np.int64)))
        for i, part in enumerate(np.array_split(flat, n)):
            pieces.append((f"{k}@{i}of{n}", part))
    files, cur, size = [], {}, 0
    for k, v in pieces:
        cost = v.nbytes + 2 * len(k) + 400
        if cur and size + cost > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += cost
    files.append(cur)
    for i, d in enumerate(files):
        np.savez(os.path.join(GOLDEN, PATTERN.replace("*", f"{i:02d}")), **d)
    return len(files)


def load_golden():
    raw = {}
    for f in sorted(glob.glob(os.path.join(GOLDEN, PATTERN))):
        with np.load(f) as z:
            raw.update({k: z[k] for k in z.files})
    out = {k: v for k, v in raw.items() if "@" not in k}
    for k in [k[:-6] for k in raw if k.endswith("@shape")]:
        n = next(int(x.split("of")[1]) for x in raw if x.startswith(k + "@0of"))
        out[k] = np.concatenate([raw[f"{k}@{i}of{n}"] for i in range(n)]).reshape(tuple(raw[k + "@shape"]))
    return out
