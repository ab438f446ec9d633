"""CPU restatement of `autoencoder_stat` (models/model_stat/autoencoder.py:8-152, base/blocks.py:11-154) for the tests, built on
oracle/titok_oracle.py (the gated RoPE stack, FSQ, rotary angles -- imported, not edited) plus the stat pieces: the Linear patchify
over `b c (t pt) (h ph) (w pw) -> b (t h w) (pt ph pw c)`, ProbPredictor behind `x.detach() + 0.1 * (x - x.detach())`, the mask
with its straight-through form, and the Linear unpatchify.  Also the deterministic inputs of the reference-piece fixtures
(tests/golden/make_golden_stat.py writes their outputs, tests/test_stat_gpu.py replays them).  TEST INFRASTRUCTURE ONLY.

`emu=True` rounds where autocast(bf16) materialises bf16 tensors -- the rounding points of the HIP path (video-tokenizer_amd/stat.py):
every Linear output, gelu(u), the sigmoid of the bf16 logit.
"""
import math

import numpy as np
import torch

from oracle import inputs as gen
from oracle import titok_oracle as T
from oracle.larp_oracle import _rb, linear

LEVELS = (8, 8, 8, 5, 5, 5)
# the yaml's model.args (cfgs/larp_tokenizer_stat.yaml:51-109 with frame_num / input_size filled in)
YAML_ARGS = {
    "bottleneck": {"name": "bottleneck", "args": {"bottleneck_dim": 16, "norm": "none",
                                                  "regularizer": {"name": "vq", "args": {"codebook_size": 8192, "commitment_loss_weight": 0.25,
                                                                                          "codebook_loss_weight": 1.0, "entropy_loss_weight": 0.0,
                                                                                          "entropy_loss_temperature": 0.01, "l2_normalized": True,
                                                                                          "stochastic": True, "stochastic_temperature": 0.03}}}},
    "prior_model": {"name": "none", "use_mix_ss": True, "mix_ss_max_ratio": 0.5, "mix_ss_peak_steps_ratio": 0.3, "n_rounds": 2,
                    "avg_loss_over_rounds": True, "no_grad_before_last_round": False, "no_dropout": False, "latent_ce_temperature": 1.0,
                    "args": {"l2_normalized": True}},
    "bottleneck_token_num": 1024, "input_size": 128, "frame_num": 16, "temporal_patch_size": 4, "patch_size": 8,
    "decoder_temporal_patch_size": 4, "decoder_patch_size": 8, "in_channels": 3, "transformer_name": "transformer_encoder_parallel",
    "encoder_name": "none", "decoder_name": "none", "encoder_hidden_size": 768, "decoder_hidden_size": 768, "encoder_num_heads": 12,
    "decoder_num_heads": 12, "encoder_depth": 6, "decoder_depth": 6, "learned_encoder_patch_pe": False, "learned_encoder_latent_query_embed": True,
    "learned_decoder_latent_pe": False, "learned_decoder_patch_query_embed": False, "use_encoder_patch_token_type_embed": False,
    "use_encoder_latent_query_token_type_embed": False, "use_decoder_latent_token_type_embed": False, "use_decoder_patch_query_token_type_embed": True,
    "encoder_query_gaussian_init": True, "latent_pe_scale_factor": 10000, "query_init_std": 0.02,
}


def to_patch_rows(video, patch):
    """rearrange 'b c (t pt) (h ph) (w pw) -> b (t h w) (pt ph pw c)' (blocks.py:72-75)"""
    b, c, tt, hh, ww = video.shape
    pt, ph, pw = patch
    x = video.reshape(b, c, tt // pt, pt, hh // ph, ph, ww // pw, pw).permute(0, 2, 4, 6, 3, 5, 7, 1)
    return x.reshape(b, (tt // pt) * (hh // ph) * (ww // pw), pt * ph * pw * c)


def from_patch_rows(rows, grid, patch, c=3):
    """rearrange 'b (t h w) (pt ph pw c) -> b c (t pt) (h ph) (w pw)' (blocks.py:145-150)"""
    b = rows.shape[0]
    t, h, w = grid
    pt, ph, pw = patch
    y = rows.reshape(b, t, h, w, pt, ph, pw, c).permute(0, 7, 1, 4, 2, 5, 3, 6)
    return y.reshape(b, c, t * pt, h * ph, w * pw)


def prob_head(x, w1, b1, w2, b2, emu=False):
    """ProbPredictor (blocks.py:11-24) on x_for_prob = x.detach() + 0.1 * (x - x.detach()) (:89): probs [..., n]"""
    xp = x.detach() + 0.1 * (x - x.detach())
    g = _rb(T.gelu_erf(linear(xp, w1, b1, emu)), emu)
    return _rb(torch.sigmoid(linear(g, w2, b2, emu)), emu).squeeze(-1)


# ------------------------------------------------------------------------------------------ small model
def make_cfg(size="tiny", frames=8, side=32, patch=(4, 8, 8), tokens=32):
    return T.make_cfg(size, frames=frames, side=side, patch=patch, tokens=tokens, levels=LEVELS)


def init_state_dict(cfg, seed=901):
    """the FSQ family's deterministic weights (titok_oracle.init_state_dict) re-laid out for the stat model: Linear patchify /
    unpatchify, plus the probability head.  The head's fc2 is drawn wide enough that the probabilities spread over (0, 1)."""
    sd = T.init_state_dict(cfg, seed)
    width = cfg["width"]
    pt, ps = cfg["patch"][0], cfg["patch"][1]
    k = 3 * pt * ps * ps
    s = [seed + 500]

    def nxt():
        s[0] += 1
        return s[0]

    def Tn(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    sd["encoder.proj_in.weight"] = Tn(gen.normal((width, k), nxt(), 0.03))
    sd["decoder.proj_out.weight"] = Tn(gen.normal((k, width), nxt(), 0.03))
    sd["decoder.proj_out.bias"] = Tn(gen.uniform((k,), nxt(), -0.02, 0.02))
    sd["encoder.prob_head.net.0.weight"] = Tn(gen.normal((width, width), nxt(), 0.05))
    sd["encoder.prob_head.net.0.bias"] = Tn(gen.uniform((width,), nxt(), -0.05, 0.05))
    sd["encoder.prob_head.net.2.weight"] = Tn(gen.normal((1, width), nxt(), 0.15))
    sd["encoder.prob_head.net.2.bias"] = Tn(gen.uniform((1,), nxt(), -0.05, 0.05))
    return sd


def stat_forward(p, cfg, video, mask, ste, emu=False, force_codes=None, taps=None):
    """autoencoder.py:98-152 with the device's 0/1 `mask` [B, n] taken as the draw (sampled / thresholded / all ones); `ste`: the mask
    is `(mask - probs).detach() + probs` (training, 'adaptive'), else a constant.  Returns pred_frames, probs, mask, codes.
    `taps` (a dict): receives the expanded [B, rows, W] mask-token tensors, with their gradients retained, under the parameter names."""
    b = video.shape[0]
    width, heads, layers = cfg["width"], cfg["heads"], cfg["layers"]
    patch, grid, n_lat = cfg["patch"], cfg["grid"], cfg["tokens"]
    n_grid = math.prod(grid)
    ang = T.rope_angles(n_lat, grid, width // heads)
    tok = linear(to_patch_rows(video, patch), p["encoder.proj_in.weight"], p["encoder.proj_in.bias"], emu)
    enc_mt = p["encoder.mask_token"].expand(b, n_lat, width)
    x = torch.cat([enc_mt, tok], dim=1)
    x = T.residual_attention_block(x, p, "encoder.model_layers.", layers, heads, ang, emu)[:, :n_lat]
    probs = prob_head(x, p["encoder.prob_head.net.0.weight"], p["encoder.prob_head.net.0.bias"], p["encoder.prob_head.net.2.weight"],
                      p["encoder.prob_head.net.2.bias"], emu)
    z = linear(x, p["encoder.proj_out.weight"], p["encoder.proj_out.bias"], emu)
    m = (mask - probs).detach() + probs if ste else mask
    codes, _, _ = T.fsq(z * m.unsqueeze(-1), LEVELS)
    if force_codes is not None:
        codes = codes + (force_codes - codes).detach()
    y = linear(codes, p["decoder.proj_in.weight"], p["decoder.proj_in.bias"], emu)
    dec_mt = p["decoder.mask_token"].expand(b, n_grid, width)
    y = torch.cat([y, dec_mt], dim=1)
    y = T.residual_attention_block(y, p, "decoder.model_layers.", layers, heads, ang, emu)[:, n_lat:]
    rows = linear(y, p["decoder.proj_out.weight"], p["decoder.proj_out.bias"], emu)
    if taps is not None and enc_mt.requires_grad:
        for name, t in (("encoder.mask_token", enc_mt), ("decoder.mask_token", dec_mt)):
            t.retain_grad()
            taps[name] = t
    return {"pred_frames": from_patch_rows(rows, grid, patch), "probs": probs, "mask": m, "codes": codes}


# ------------------------------------------------------------------------------------------ reference-piece fixtures
PIECE = dict(width=256, frames=8, side=32, patch=(4, 8, 8), batch=2, lat_tokens=32, mask_tokens=64)
PIECE_LOGITS = (-3.0, -1.0, -0.25, 0.0, 0.25, 1.0, 3.0)     # bf16-exact; sigmoid of each is far from a bf16 rounding boundary


def piece_inputs():
    """deterministic inputs of the fixtures (float32 numpy): only the reference's OUTPUTS are committed"""
    W, P = PIECE["width"], PIECE["patch"]
    k = 3 * P[0] * P[1] * P[2]
    b, n = PIECE["batch"], PIECE["lat_tokens"]
    grid_n = (PIECE["frames"] // P[0]) * (PIECE["side"] // P[1]) ** 2
    nm = PIECE["mask_tokens"]
    pick = (gen.hash_u64(b * nm, 9609) % np.uint64(len(PIECE_LOGITS))).astype(np.int64)
    return {
        "video": gen.video_clips(b, PIECE["frames"], PIECE["side"], 9601),
        "proj_in_w": gen.normal((W, k), 9602, 0.03), "proj_in_b": gen.uniform((W,), 9603, -0.05, 0.05),
        "lat": gen.normal((b, n, W), 9604, 1.0),
        "fc1_w": gen.normal((W, W), 9605, 0.05), "fc1_b": gen.uniform((W,), 9606, -0.05, 0.05),
        "fc2_w": gen.normal((1, W), 9607, 0.15), "fc2_b": gen.uniform((1,), 9608, -0.05, 0.05),
        "probs_cot": gen.normal((b, n), 9610, 1.0),
        "dec_y": gen.normal((b, grid_n, W), 9611, 1.0),
        "proj_out_w": gen.normal((k, W), 9612, 0.03), "proj_out_b": gen.uniform((k,), 9613, -0.05, 0.05),
        "enc_x": gen.normal((b, nm, len(LEVELS)), 9614, 1.5),
        "enc_logits": np.asarray(PIECE_LOGITS, dtype=np.float32)[pick].reshape(b, nm),
    }


def bf16_sigmoid(logits):
    """probabilities of the eval-masking fixture: the bf16-rounded sigmoid of bf16-exact logits, as the gate computes them"""
    return torch.sigmoid(torch.as_tensor(logits).float()).to(torch.bfloat16).float()
