"""Packed variable-length attention layer of the reference's `titok` family (models/model_titok/base/transformer.py:32-62, base/rope.py,
base/blocks.py:32-64): the clips of a batch have different sizes, so they are packed into one [sum L_b, D] tensor and every sequence attends
inside itself; the layers are grouped-query (Hq query heads over Hkv KV heads).  This module is the layer and its rotary tables, and below
them the feed-forward, the block stack, TiTokEncoder and TiTokDecoder (base/blocks.py:67-222); titok_model.py holds the `titok` registry entry.
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


# ------------------------------------------------------------------------------------------------------------------------
# the model around the layer: feed-forward, block stack, encoder and decoder (transformer.py:14-30, 65-85; blocks.py:67-222)
# ------------------------------------------------------------------------------------------------------------------------
MAX_CLIPS = hip.VARLEN_MAX_SEQ                   # clips per call: one table entry each in the kernels' arguments
_TABLE_CACHE_ENTRIES = 8


class GEGLU(nn.Module):
    """transformer.py:14-17, parameterless: index 2 of ffd.  It never runs on its own here: FeedForward.forward is one Function."""

    def forward(self, x):
        raise RuntimeError("varlen.GEGLU is a placeholder at the reference's index: call the surrounding varlen.ffd(...) module, which runs as one Function")


class FeedForward(nn.Sequential):
    """the nn.Sequential of transformer.py:20-30 (LayerNorm at 0, Linear at 1, GEGLU at 2, Dropout(0.) at 3, Linear at 4; state-dict keys
    0.weight / 0.bias / 1.weight / 4.weight) whose forward is functional.VarlenFeedForwardLayer on x fp32 [M, D]"""

    def forward(self, x, residual=False):
        hip.require_gpu(x, *self.parameters())
        inner = self[4].in_features
        return F_.VarlenFeedForwardLayer.apply(x, self[0].weight, self[0].bias, self[1].weight, self[4].weight, self[0].eps, residual,
                                               packs.get(self, ("1",)), packs.get(self, ("4",), k_pad=(inner + 63) // 64 * 64))


def ffd(dim, mult=4, mult_of=32, dropout=0.):
    if dim not in LN_WIDTHS:
        raise ValueError(f"varlen.ffd: dim {dim} must be a LayerNorm width {LN_WIDTHS}")
    if dropout:
        raise ValueError("varlen.ffd: dropout is not built (the reference runs its layers with 0.)")
    inner_dim = int(mult * (2 / 3) * dim)
    inner_dim = mult_of * ((inner_dim + mult_of - 1) // mult_of)
    return FeedForward(nn.LayerNorm(dim), nn.Linear(dim, inner_dim * 2, bias=False), GEGLU(), nn.Dropout(dropout), nn.Linear(inner_dim, dim, bias=False))


class ResidualAttentionBlock(nn.Module):
    """transformer.py:65-85: num_layer x {x = x + Attn(x); x = x + ffd(x)} on the packed x fp32 [M, D]; keys attn_layer.{i}.*, ffd_layer.{i}.*.
    One Function per half block, the residual additions in the epilogues of the out_proj / second feed-forward GEMMs.  cu_seqlens is turned
    into a host list once and shared by all layers (a device tensor costs one synchronisation)."""

    def __init__(self, embed_dim=512, heads=(8, 2), mlp_ratio=4, num_layer=2):
        super().__init__()
        self.num_layer = num_layer
        self.attn_layer = nn.Sequential()
        self.ffd_layer = nn.Sequential()
        for _ in range(num_layer):
            self.attn_layer.append(Attn(embed_dim, list(heads)))
            self.ffd_layer.append(ffd(embed_dim, mlp_ratio))

    def forward(self, x, freqs, cu_seqlens, max_seqlen=None):
        cu = hip.cu_seqlens_list(cu_seqlens)
        hip.require_gpu(x, *self.parameters())
        if isinstance(freqs, (tuple, list)):
            cos, sin = freqs
        else:
            cos, sin = freqs.real.float().contiguous().to(x.device), freqs.imag.float().contiguous().to(x.device)
        for a, f in zip(self.attn_layer, self.ffd_layer):
            x = F_.VarlenAttentionResidualLayer.apply(x, cos, sin, cu, a.pre_ln.weight, a.pre_ln.bias, a.to_qkv.weight, a.q_norm.weight, a.q_norm.bias,
                                                      a.k_norm.weight, a.k_norm.bias, a.out_proj.weight, a.q_heads, a.kv_heads, a.pre_ln.eps,
                                                      packs.get(a, ("to_qkv",)), packs.get(a, ("out_proj",)))
            x = f(x, residual=True)
        return x


def init_weights(module):
    """blocks.py:67-79"""
    if isinstance(module, nn.Linear):
        module.weight.data = nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)
    elif isinstance(module, nn.LayerNorm):
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)
        if module.weight is not None:
            nn.init.constant_(module.weight, 1.0)
    elif isinstance(module, (nn.Conv3d, nn.Conv2d)):
        nn.init.xavier_uniform_(module.weight)
        nn.init.zeros_(module.bias)


class _PackedSide(nn.Module):
    """What TiTokEncoder and TiTokDecoder share: the geometry of a call -- grids, boundaries and lead counts as host lists, built once per
    forward and never read back from the device -- and a small cache of the rotary tables keyed by (grids, token_counts), so that a steady
    training loop does not rebuild float64 tables every step.  `RoPE` of the reference holds no parameter or persistent buffer: no key."""

    def _setup(self, model_size, patch_size, dims):
        self.patch_size = tuple(int(v) for v in patch_size)
        self.width, self.num_layers, self.heads, mlp_ratio = dims if dims is not None else get_model_dims(model_size)
        if self.width != 64 * self.heads[0]:
            raise ValueError(f"{type(self).__name__}: width {self.width} must be 64 * q heads ({self.heads[0]}): head dimension 64 only")
        if self.width not in LN_WIDTHS:
            raise ValueError(f"{type(self).__name__}: width {self.width} must be a LayerNorm width {LN_WIDTHS}")
        if self.patch_size[1] != self.patch_size[2] or self.patch_size[1] % 8:
            raise ValueError(f"{type(self).__name__}: patch_size {self.patch_size} must be (pt, p, p) with p a multiple of 8")
        self._tables = {}
        return mlp_ratio

    def geometry(self, sizes, token_counts):
        """sizes: (T, H, W) per clip -> (grids, grid_sizes, seq_lens, cu); refuses what the kernels would"""
        who = type(self).__name__
        counts = [int(n) for n in token_counts]
        if not 1 <= len(sizes) <= MAX_CLIPS:
            raise ValueError(f"{who}: {len(sizes)} clips in one call; 1..{MAX_CLIPS} are supported")
        if len(counts) != len(sizes):
            raise ValueError(f"{who}: {len(counts)} token counts for {len(sizes)} clips")
        if any(n < 1 for n in counts):
            raise ValueError(f"{who}: every clip needs at least one latent token, got {counts}")
        for s in sizes:
            if len(s) != 3 or any(int(d) <= 0 or int(d) % q for d, q in zip(s, self.patch_size)):
                raise ValueError(f"{who}: a clip of size {tuple(s)} (T, H, W) is no positive multiple of the patch {self.patch_size}")
        grids = [tuple(int(d) // q for d, q in zip(s, self.patch_size)) for s in sizes]
        grid_sizes = [math.prod(g) for g in grids]
        seq_lens = [g + n for g, n in zip(grid_sizes, counts)]
        cu = [0]
        for n in seq_lens:
            cu.append(cu[-1] + n)
        return grids, grid_sizes, seq_lens, cu

    def rope_tables(self, grids, token_counts, device):
        """(cos, sin) fp32 [M, 32] on `device` from rope_freqs, cached on the module by (grids, token_counts, device)"""
        key = (tuple(tuple(g) for g in grids), tuple(int(n) for n in token_counts), str(device))
        hit = self._tables.get(key)
        if hit is None:
            while len(self._tables) >= _TABLE_CACHE_ENTRIES:
                self._tables.pop(next(iter(self._tables)))
            _, cos, sin = rope_freqs(grids, token_counts, device)
            hit = self._tables[key] = (cos, sin)
        return hit


class TiTokEncoder(_PackedSide):
    """blocks.py:82-147.  forward(x, token_counts): x a list of clips [in_channels, T_b, H_b, W_b] of any sizes that the patch divides,
    token_counts[b] >= 1 latent tokens for clip b -> the packed latents fp32 [sum token_counts, out_channels].  Launches around the layer
    stack: vt_patchify_clips, the proj_in GEMM, vt_packed_scatter ([mask_token x n_b | patch rows]), vt_packed_gather (the latent rows),
    ln_post, the proj_out GEMM.  `_dims` = (width, layers, [Hq, Hkv], mlp_ratio) overrides model_size for small tests."""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=3, out_channels=5, max_grid=(32, 256, 256), max_tokens=2048, _dims=None):
        super().__init__()
        mlp_ratio = self._setup(model_size, patch_size, _dims)
        self.token_size, self.in_channels = out_channels, in_channels
        self.mask_token = nn.Parameter(self.width ** -0.5 * torch.randn(1, self.width))
        self.proj_in = nn.Linear(in_channels * math.prod(self.patch_size), self.width)
        self.model_layers = ResidualAttentionBlock(embed_dim=self.width, heads=self.heads, mlp_ratio=mlp_ratio, num_layer=self.num_layers)
        self.ln_post = nn.LayerNorm(self.width)
        self.proj_out = nn.Linear(self.width, self.token_size, bias=True)

    def forward(self, x, token_counts):
        x = list(x)
        hip.require_gpu(*x, *self.parameters())
        if any(v.dim() != 4 or v.shape[0] != self.in_channels for v in x):
            raise ValueError(f"TiTokEncoder: every clip must be [{self.in_channels}, T, H, W], got {[tuple(v.shape) for v in x]}")
        grids, _, seq_lens, cu = self.geometry([v.shape[1:] for v in x], token_counts)
        counts = [int(n) for n in token_counts]
        rows = F_.PatchRowsClips.apply(self.patch_size[0], self.patch_size[1], *x)
        tok = F_.Linear.apply(rows, self.proj_in.weight, self.proj_in.bias)
        h = F_.PackedScatter.apply(tok, self.mask_token, cu, counts, hip.PACKED_TAIL)
        h = self.model_layers(h, self.rope_tables(grids, counts, h.device), cu, max(seq_lens))
        lat = F_.PackedGather.apply(h, cu, counts, hip.PACKED_LEAD)
        lat = F_.LayerNormRows.apply(lat, self.ln_post.weight, self.ln_post.bias, self.ln_post.eps)
        return F_.Linear.apply(lat, self.proj_out.weight, self.proj_out.bias)


class TiTokDecoder(_PackedSide):
    """blocks.py:150-222.  forward(x, token_counts, grids): x the packed codes [sum token_counts, in_channels], grids[b] = (T_b, H_b, W_b) of
    clip b in PIXELS (the reference's argument) -> a list of clips fp32 [out_channels, T_b, H_b, W_b].  Launches around the layer stack: the
    proj_in GEMM, vt_packed_scatter ([code rows | mask_token x G_b]), ln_pre, vt_packed_gather (the grid rows), the proj_out GEMM,
    vt_unpatchify_clips.  ln_pre's output is rounded to bf16 (the LayerNorm kernel's output format), where autocast keeps fp32."""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=5, out_channels=3, max_grid=(32, 256, 256), max_tokens=2048, _dims=None):
        super().__init__()
        mlp_ratio = self._setup(model_size, patch_size, _dims)
        self.token_size, self.out_channels = in_channels, out_channels
        self.mask_token = nn.Parameter(self.width ** -0.5 * torch.randn(1, self.width))
        self.proj_in = nn.Linear(self.token_size, self.width, bias=True)
        self.ln_pre = nn.LayerNorm(self.width)
        self.model_layers = ResidualAttentionBlock(embed_dim=self.width, heads=self.heads, mlp_ratio=mlp_ratio, num_layer=self.num_layers)
        self.proj_out = nn.Linear(self.width, out_channels * math.prod(self.patch_size))

    def forward(self, x, token_counts, grids):
        hip.require_gpu(x, *self.parameters())
        sizes = [tuple(int(d) for d in g) for g in grids]
        tgrids, _, seq_lens, cu = self.geometry(sizes, token_counts)
        counts = [int(n) for n in token_counts]
        if x.dim() != 2 or tuple(x.shape) != (sum(counts), self.token_size):
            raise ValueError(f"TiTokDecoder: expected packed codes [{sum(counts)}, {self.token_size}], got {tuple(x.shape)}")
        tok = F_.Linear.apply(x, self.proj_in.weight, self.proj_in.bias)
        h = F_.PackedScatter.apply(tok, self.mask_token, cu, counts, hip.PACKED_LEAD)
        h = F_.LayerNormRows.apply(h, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps)
        h = self.model_layers(h, self.rope_tables(tgrids, counts, h.device), cu, max(seq_lens))
        rows = F_.PackedGather.apply(h, cu, counts, hip.PACKED_TAIL)
        rows = F_.Linear.apply(rows, self.proj_out.weight, self.proj_out.bias)
        return list(F_.UnpatchifyClips.apply(rows, sizes, self.out_channels, self.patch_size[0], self.patch_size[1]))
