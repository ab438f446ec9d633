"""Packed variable-length attention layer of the reference's `titok` family (models/model_titok/base/transformer.py:32-62, base/rope.py,
base/blocks.py:32-64): the clips of a batch have different sizes, so they are packed into one [sum L_b, D] tensor and every sequence attends
inside itself; the layers are grouped-query (Hq query heads over Hkv KV heads).  This module is the layer and its rotary tables; the
encoder, the decoder and the `titok` registry entry build on it.
"""
import math

import torch
import torch.nn as nn

from . import functional as F_
from . import hip, packs

LN_WIDTHS = (128, 256, 384, 512, 768, 1024)      # widths of vt_layernorm_fwd
AXES_DIM = (24, 20, 20)                          # RoPE.__init__ for head_dim 64 over (T, H, W): 20 each, the remainder on T
THETA = 10000.0


def get_model_dims(model_size="tiny", head_dim=64, mlp_ratio=4.0):
    """base/blocks.py:32-64 -> (width, layers, [q heads, kv heads], mlp_ratio)"""
    if model_size.endswith("_thin"):
        model_size = model_size[:-5]
        layers = {"tiny": 2, "small": 5, "base": 7, "large": 8}[model_size]
        heads = {"tiny": [8, 2], "small": [12, 4], "base": [16, 4], "large": [32, 8]}[model_size]
        mlp_ratio = mlp_ratio / 2
    else:
        layers = {"tiny": 4, "small": 8, "base": 12, "large": 24}[model_size]
        heads = {"tiny": [4, 2], "small": [8, 2], "base": [12, 4], "large": [16, 4]}[model_size]
    return int(head_dim * heads[0]), layers, heads, mlp_ratio


def _axis_freqs(dim, pos, theta=THETA):
    """get_1d_rotary_pos_embed (rope.py:27-46) in float64: the angles pos * theta^linspace(0, 1, dim / 2) * pi / 2"""
    freqs = theta ** torch.linspace(math.log(1.0, theta), math.log(theta, theta), dim // 2, dtype=torch.float64)
    return (freqs * math.pi / 2.0) * pos.to(torch.float64).unsqueeze(-1)


def position_ids(grid, num_tokens):
    """Lumina2RotaryPosEmbed.forward (rope.py:91-121): the num_tokens latent tokens sit on the diagonal (t, t, t); the grid's (frame, row,
    column) follow, offset by num_tokens -> int64 [num_tokens + prod(grid), 3]"""
    frames, height, width = grid
    ids = torch.zeros(num_tokens + frames * height * width, 3, dtype=torch.int64)
    ids[:num_tokens] = torch.arange(num_tokens).unsqueeze(-1)
    ids[num_tokens:, 0] = torch.arange(frames).view(-1, 1, 1).repeat(1, height, width).flatten()
    ids[num_tokens:, 1] = torch.arange(height).view(1, -1, 1).repeat(frames, 1, width).flatten()
    ids[num_tokens:, 2] = torch.arange(width).view(1, 1, -1).repeat(frames, height, 1).flatten()
    ids[num_tokens:] += num_tokens
    return ids


def rope_freqs(grids, token_counts, device=None):
    """RoPE.forward (rope.py:149-157) for a packed batch: one (grid, token_count) per sequence, sequence b has token_counts[b] +
    prod(grids[b]) rows -> (freqs complex128 [M, 32], cos fp32 [M, 32], sin fp32 [M, 32]).  The complex table is the reference's (its eval
    path, which its precomputed train path equals); cos / sin are its real and imaginary parts rounded to fp32, what the kernels read (the
    reference multiplies in complex128: DESIGN.md records the deviation).  Computed on the host in float64; cos / sin are moved to `device`."""
    angles = []
    for grid, n in zip(grids, token_counts):
        ids = position_ids(tuple(int(g) for g in grid), int(n))
        angles.append(torch.cat([_axis_freqs(d, ids[:, i]) for i, d in enumerate(AXES_DIM)], dim=-1))
    ang = torch.cat(angles, dim=0)
    freqs = torch.polar(torch.ones_like(ang), ang)
    cos, sin = freqs.real.float().contiguous(), freqs.imag.float().contiguous()
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return freqs, cos, sin


class Attn(nn.Module):
    """transformer.py:32-62 with the reference's state-dict keys: pre_ln.weight / bias [D], to_qkv.weight [D + 128 Hkv, D], q_norm.weight /
    bias [64], k_norm.weight / bias [64], out_proj.weight [D, D]; heads = [Hq, Hkv], D = 64 Hq.

    forward(x, freqs, cu_seqlens, max_seqlen): x fp32 [M, D], the packed batch; freqs the rotary table of rope_freqs -- the (cos, sin) pair of
    fp32 [M, 32] device tensors, or the complex [M, 32] table itself, which is then split and moved on every call; cu_seqlens a list, or a
    CPU or device int tensor.  A DEVICE tensor costs one synchronisation per call (the boundaries travel to the kernels in their arguments,
    so the host must know them): build the list on the host, as the reference's encoder does.  max_seqlen is accepted for the reference's
    signature and not used: the grid is sized from the boundaries themselves.  At most hip.VARLEN_MAX_SEQ sequences per call."""

    def __init__(self, dim, heads):
        super().__init__()
        self.dim = dim
        self.q_heads, self.kv_heads = heads
        self.head_dim = dim // self.q_heads
        if dim != 64 * self.q_heads:
            raise ValueError(f"varlen.Attn: dim {dim} must be 64 * q_heads ({self.q_heads}): the attention kernels have head_dim 64")
        if self.q_heads % self.kv_heads:
            raise ValueError(f"varlen.Attn: q_heads {self.q_heads} must be a multiple of kv_heads {self.kv_heads}")
        if dim not in LN_WIDTHS:
            raise ValueError(f"varlen.Attn: dim {dim} must be a LayerNorm width {LN_WIDTHS}")
        self.gqa_dim = self.head_dim * self.kv_heads
        self.pre_ln = nn.LayerNorm(dim)
        self.to_qkv = nn.Linear(dim, self.gqa_dim * 2 + dim, bias=False)
        self.q_norm = nn.LayerNorm(self.head_dim)
        self.k_norm = nn.LayerNorm(self.head_dim)
        self.out_proj = nn.Linear(dim, dim, bias=False)

    def forward(self, x, freqs, cu_seqlens, max_seqlen=None):
        cu = hip.cu_seqlens_list(cu_seqlens)
        hip.require_gpu(x, *self.parameters())
        if isinstance(freqs, (tuple, list)):
            cos, sin = freqs
        else:
            cos, sin = freqs.real.float().contiguous().to(x.device), freqs.imag.float().contiguous().to(x.device)
        return F_.VarlenAttentionLayer.apply(x, cos, sin, cu, self.pre_ln.weight, self.pre_ln.bias, self.to_qkv.weight, self.q_norm.weight,
                                             self.q_norm.bias, self.k_norm.weight, self.k_norm.bias, self.out_proj.weight, self.q_heads,
                                             self.kv_heads, self.pre_ln.eps, packs.get(self, ("to_qkv",)), packs.get(self, ("out_proj",)))
