"""The reference's `autoencoder_design` (models/model_design/autoencoder.py, base/blocks.py, base/transformer.py) on the HIP kernels.

Layers: `RMSNorm`, `CrossAttention` (the layer through which the decoder reads the 256 first-frame tokens), `SelfAttention` (RMSNorm per head on q
and k, rotary, a separate `to_gate`), `TransformerBlock` (every residual is `x + res_scale * f(x)` with a learnable 0-dim scale that stays on the
device) and `TransformerStack` (blocks + an fp32 `final_norm`).  Models: `LearnedQueryTokens`, the Perceiver-style `Encoder` and
`FirstFrameEncoder`, `UnifiedDecoder` and `AutoEncoder`, registered as `autoencoder_design` (the reference registers only the whole model).

Same constructor arguments, module tree and parameter names as the reference, so its state dicts load with strict=True.  Every matrix product,
norm, attention and residual runs in libvt_hip (functional.py composes the launches); torch owns the tensors, the autograd graph, the
concatenation of queries and tokens, the 256-row SiLU / add of the condition adapter and the output rearrange.  No CPU path.
"""
import math

import torch
import torch.nn as nn
from torch.nn import functional as TF

from . import functional as F_
from . import hip, packs
from .fsq import FSQ
from .registry import register
from .titok import get_model_dims, rope_tables

RMS_WIDTHS = (128, 256, 384, 512, 768, 1024, 1280, 1536, 2560)      # vt_rmsnorm_any_* (RMS_WIDTHS of csrc/vt_rmsnorm.hip)


class RMSNorm(nn.Module):
    """transformer.py:18-27.  Holds the weight and eps under the reference's parameter name; the arithmetic runs inside the fused layer
    (CrossAttention: vt_rmsnorm_any_* for norm_q / norm_kv, vt_head_rmsnorm_* per head for q_norm / k_norm; SelfAttention: vt_rmsnorm_any_* and
    vt_qkrms_rope_*; the ffn, the stack's final_norm and the condition adapter through functional.*), so there is no stand-alone forward."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        raise hip.HipError("design.RMSNorm has no stand-alone forward: the layer that owns it (design.CrossAttention) applies it in its fused pass")


class CrossAttention(nn.Module):
    """transformer.py:92-141: out_proj(flash_attn(q_norm(to_q(norm_q(x))), k_norm(k), v) * sigmoid(to_gate(norm_q(x)))) with
    k, v = to_kv(norm_kv(context)).chunk(2); x [B, N, dim], context [B, M, context_dim] -> [B, N, dim].  head_dim must be 64."""

    def __init__(self, dim, heads, context_dim=None):
        super().__init__()
        self.heads = heads
        self.head_dim = dim // heads
        context_dim = context_dim or dim
        if dim != 64 * heads:
            raise ValueError(f"design.CrossAttention: dim {dim} must be 64 * heads ({heads}): the attention kernels have head_dim 64")
        if dim not in RMS_WIDTHS or context_dim not in RMS_WIDTHS:
            raise ValueError(f"design.CrossAttention: dim {dim} and context_dim {context_dim} must be RMSNorm widths {RMS_WIDTHS}")
        self.norm_q = RMSNorm(dim)
        self.norm_kv = RMSNorm(context_dim)
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_kv = nn.Linear(context_dim, dim * 2, bias=False)
        self.to_gate = nn.Linear(dim, dim, bias=False)
        self.q_norm = RMSNorm(self.head_dim)
        self.k_norm = RMSNorm(self.head_dim)
        self.out_proj = nn.Linear(dim, dim, bias=False)

    def forward(self, x, context):
        hip.require_gpu(x, context, *self.parameters())
        return F_.CrossAttentionLayer.apply(x, context, self.norm_q.weight, self.norm_kv.weight, self.to_q.weight, self.to_kv.weight,
                                            self.to_gate.weight, self.q_norm.weight, self.k_norm.weight, self.out_proj.weight, self.heads,
                                            self.norm_q.eps, packs.get(self, ("to_q", "to_gate")), packs.get(self, ("to_kv",)),
                                            packs.get(self, ("out_proj",)))


class SelfAttention(nn.Module):
    """transformer.py:46-85.  forward(x, cos, sin, res_scale) returns the new residual stream x + res_scale * attn(x): the scaled residual is the
    last launch of the fused layer (functional.SelfAttentionLayer).  head_dim must be 64; cos / sin are fp32 [L, 32] device tables."""

    def __init__(self, dim, heads):
        super().__init__()
        self.dim, self.heads, self.head_dim = dim, heads, dim // heads
        if dim != 64 * heads:
            raise ValueError(f"design.SelfAttention: dim {dim} must be 64 * heads ({heads}): the attention kernels have head_dim 64")
        if dim not in RMS_WIDTHS:
            raise ValueError(f"design.SelfAttention: dim {dim} must be an RMSNorm width {RMS_WIDTHS}")
        self.norm = RMSNorm(dim)
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.to_gate = nn.Linear(dim, dim, bias=False)
        self.q_norm = RMSNorm(self.head_dim)
        self.k_norm = RMSNorm(self.head_dim)
        self.out_proj = nn.Linear(dim, dim, bias=False)

    def forward(self, x, cos, sin, res_scale):
        hip.require_gpu(x, cos, sin, res_scale, *self.parameters())
        return F_.SelfAttentionLayer.apply(x, cos, sin, res_scale, self.norm.weight, self.to_qkv.weight, self.to_gate.weight, self.q_norm.weight,
                                           self.k_norm.weight, self.out_proj.weight, self.heads, self.norm.eps, packs.get(self, ("to_qkv", "to_gate")),
                                           packs.get(self, ("out_proj",)))


class GEGLU(nn.Module):
    """transformer.py:11-15; parameterless: it keeps the reference's Sequential indices (ffn.{0,1,3}); the arithmetic is vt_geglu_* inside
    functional.FeedForwardLayer"""

    def forward(self, x):
        raise hip.HipError("design.GEGLU has no stand-alone forward: TransformerBlock applies its ffn as one fused layer")


def ffn_inner_dim(dim, mult=4, mult_of=32):
    """transformer.py:32-33"""
    inner = int(mult * (2 / 3) * dim)
    return mult_of * ((inner + mult_of - 1) // mult_of)


def make_ffn(dim, mult=4, mult_of=32):
    """transformer.py:30-39: holders under the reference's keys ffn.0.weight (RMSNorm), ffn.1.weight, ffn.3.weight"""
    inner = ffn_inner_dim(dim, mult, mult_of)
    return nn.Sequential(RMSNorm(dim), nn.Linear(dim, inner * 2, bias=False), GEGLU(), nn.Linear(inner, dim, bias=False))


class TransformerBlock(nn.Module):
    """transformer.py:148-185: x + s_sa * self_attn(x); [x + s_ca * cross_attn(x, context)]; x + s_ffn * ffn(x), the three scales learnable 0-dim
    parameters initialised to 1 / sqrt(2 * layer_idx + 1)"""

    def __init__(self, dim, heads, mlp_ratio=4, has_cross_attn=False, layer_idx=0, total_layers=1):
        super().__init__()
        self.self_attn = SelfAttention(dim, heads)
        self.ffn = make_ffn(dim, mlp_ratio)
        self.has_cross_attn = has_cross_attn
        if has_cross_attn:
            self.cross_attn = CrossAttention(dim, heads)
        init_scale = 1.0 / math.sqrt(2 * layer_idx + 1)
        self.res_scale_sa = nn.Parameter(torch.tensor(init_scale))
        self.res_scale_ffn = nn.Parameter(torch.tensor(init_scale))
        if has_cross_attn:
            self.res_scale_ca = nn.Parameter(torch.tensor(init_scale))

    def forward(self, x, freqs, context=None):
        cos, sin = freqs
        x = self.self_attn(x, cos, sin, self.res_scale_sa)
        if self.has_cross_attn and context is not None:
            x = F_.ResidualScale.apply(x, self.cross_attn(x, context), self.res_scale_ca)
        ffn = self.ffn
        inner = ffn[3].weight.shape[1]
        return F_.FeedForwardLayer.apply(x, self.res_scale_ffn, ffn[0].weight, ffn[1].weight, ffn[3].weight, ffn[0].eps, packs.get(self, ("ffn.1",)),
                                         packs.get(self, ("ffn.3",), k_pad=F_._pad64(inner)))


class TransformerStack(nn.Module):
    """transformer.py:188-216: the blocks, then final_norm, whose output is fp32 and unrounded.  freqs = (cos, sin) fp32 [L, 32] device tables."""

    def __init__(self, embed_dim=512, heads=8, mlp_ratio=4, num_layers=2, has_cross_attn=False):
        super().__init__()
        self.layers = nn.ModuleList([TransformerBlock(dim=embed_dim, heads=heads, mlp_ratio=mlp_ratio, has_cross_attn=has_cross_attn, layer_idx=i,
                                                      total_layers=num_layers) for i in range(num_layers)])
        self.final_norm = RMSNorm(embed_dim)

    def forward(self, x, freqs, context=None):
        hip.require_gpu(x, context, *freqs)
        x = x.float()
        for layer in self.layers:
            x = layer(x, freqs, context=context)
        return F_.RMSNormF32.apply(x, self.final_norm.weight, self.final_norm.eps)


def init_weights(module):
    """models/model_design/base/utils.py:40-52"""
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)
    elif isinstance(module, (nn.Conv3d, nn.Conv2d)):
        nn.init.xavier_uniform_(module.weight)
        nn.init.zeros_(module.bias)


class LearnedQueryTokens(nn.Module):
    """blocks.py:13-28: one learnable query per position"""

    def __init__(self, num_tokens, dim):
        super().__init__()
        self.tokens = nn.Parameter(torch.randn(1, num_tokens, dim) * (dim ** -0.5))

    def forward(self, batch_size):
        return self.tokens.expand(batch_size, -1, -1)


class _Tables:
    """the rotary tables of a module: built once on the host (titok.rope_tables = the reference's get_freqs), moved to the device on first use"""

    def _freqs(self, device):
        if self._freqs_dev is None or self._freqs_dev[0].device != device:
            self._freqs_dev = (self.freqs[0].to(device), self.freqs[1].to(device))
        return self._freqs_dev


class Encoder(nn.Module, _Tables):
    """blocks.py:35-108: Conv3d patch embed, `out_tokens` learned queries in FRONT of the patch tokens, the stack, first out_tokens rows ->
    Linear(width, token_size)"""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=3, out_channels=5, in_grid=(32, 256, 256), out_tokens=2048):
        super().__init__()
        self.patch_size, self.token_size, self.in_channels, self.out_tokens = tuple(patch_size), out_channels, in_channels, out_tokens
        self.grid = [x // y for x, y in zip(in_grid, patch_size)]
        self.grid_size = math.prod(self.grid)
        self.width, self.num_layers, self.heads, mlp_ratio = get_model_dims(model_size)
        assert patch_size[1] == patch_size[2] and in_grid[1] == in_grid[2], "square frames and patches (the reference's only geometry)"
        self.patch_embed = nn.Conv3d(in_channels, self.width, kernel_size=self.patch_size, stride=self.patch_size)
        self.query_tokens = LearnedQueryTokens(out_tokens, self.width)
        self.freqs = rope_tables(out_tokens, self.grid, head_dim=self.width // self.heads)
        self._freqs_dev = None
        self.transformer = TransformerStack(embed_dim=self.width, heads=self.heads, mlp_ratio=mlp_ratio, num_layers=self.num_layers, has_cross_attn=False)
        self.proj_out = nn.Linear(self.width, self.token_size, bias=True)
        self.apply(init_weights)

    def _embed(self, x):
        return F_.PatchEmbed.apply(x, self.patch_embed.weight, self.patch_embed.bias, None)

    def forward(self, x):
        hip.require_gpu(x)
        tok = self._embed(x)
        h = torch.cat([self.query_tokens(x.shape[0]), tok], dim=1)
        h = self.transformer(h, self._freqs(x.device))
        return F_.Linear.apply(h[:, :self.out_tokens], self.proj_out.weight, self.proj_out.bias)


class FirstFrameEncoder(Encoder):
    """blocks.py:115-190: the encoder of the first frame: a Conv2d patch embed (run as the patch GEMM with a temporal patch of 1), half the
    layers (at least 2), rotary tables for the grid [1, h, w]"""

    def __init__(self, model_size="tiny", patch_size_hw=(8, 8), in_channels=3, out_channels=5, in_hw=(128, 128), out_tokens=256):
        nn.Module.__init__(self)
        self.patch_size_hw, self.token_size, self.out_tokens = tuple(patch_size_hw), out_channels, out_tokens
        self.grid_hw = [x // y for x, y in zip(in_hw, patch_size_hw)]
        self.grid_size = math.prod(self.grid_hw)
        self.width, self.num_layers, self.heads, mlp_ratio = get_model_dims(model_size)
        assert patch_size_hw[0] == patch_size_hw[1] and in_hw[0] == in_hw[1], "square frames and patches (the reference's only geometry)"
        self.patch_embed = nn.Conv2d(in_channels, self.width, kernel_size=self.patch_size_hw, stride=self.patch_size_hw)
        self.query_tokens = LearnedQueryTokens(out_tokens, self.width)
        self.freqs = rope_tables(out_tokens, [1] + self.grid_hw, head_dim=self.width // self.heads)
        self._freqs_dev = None
        self.transformer = TransformerStack(embed_dim=self.width, heads=self.heads, mlp_ratio=mlp_ratio, num_layers=max(self.num_layers // 2, 2),
                                            has_cross_attn=False)
        self.proj_out = nn.Linear(self.width, self.token_size, bias=True)
        self.apply(init_weights)

    def _embed(self, x):
        if x.dim() == 4:
            x = x.unsqueeze(2)
        w = self.patch_embed.weight
        return F_.PatchEmbed.apply(x, w.view(w.shape[0], w.shape[1], 1, w.shape[2], w.shape[3]), self.patch_embed.bias, None)


class UnifiedDecoder(nn.Module, _Tables):
    """blocks.py:197-303: proj_in(latents) with the grid's learned queries BEHIND them through the stack; the first-frame tokens reach it through
    the blocks' cross attention as context = c + cond_adapter(c), c = proj_cond(cond); last grid_size rows -> proj_out -> the (pt ph pw c)
    rearrange into the video.  Rounding points of autocast(bf16) in the condition path: c, every adapter output and the sum are bf16."""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=5, out_channels=3, in_tokens=2048, cond_tokens=0, out_grid=(32, 256, 256)):
        super().__init__()
        self.patch_size, self.token_size, self.out_channels = tuple(patch_size), in_channels, out_channels
        self.in_tokens, self.cond_tokens = in_tokens, cond_tokens
        self.grid = [x // y for x, y in zip(out_grid, patch_size)]
        self.grid_size = math.prod(self.grid)
        self.width, self.num_layers, self.heads, mlp_ratio = get_model_dims(model_size)
        self.proj_in = nn.Linear(self.token_size, self.width, bias=True)
        if self.cond_tokens > 0:
            self.proj_cond = nn.Linear(self.token_size, self.width, bias=True)
            self.cond_adapter = nn.Sequential(RMSNorm(self.width), nn.Linear(self.width, self.width, bias=False), nn.SiLU(),
                                              nn.Linear(self.width, self.width, bias=False))
        self.query_tokens = LearnedQueryTokens(self.grid_size, self.width)
        self.freqs = rope_tables(in_tokens, self.grid, head_dim=self.width // self.heads)
        self._freqs_dev = None
        self.transformer = TransformerStack(embed_dim=self.width, heads=self.heads, mlp_ratio=mlp_ratio, num_layers=self.num_layers,
                                            has_cross_attn=(cond_tokens > 0))
        self.proj_out = nn.Linear(self.width, out_channels * math.prod(patch_size))
        self.apply(init_weights)

    def _context(self, cond):
        ad = self.cond_adapter
        c = F_.Linear.apply(cond, self.proj_cond.weight, self.proj_cond.bias)                       # bf16 values
        t = F_.Linear.apply(F_.RMSNormRows.apply(c, ad[0].weight, ad[0].eps, "rmsnorm_any"), ad[1].weight, None)
        t = F_.Linear.apply(TF.silu(t.bfloat16()).float(), ad[3].weight, None)
        return (c.bfloat16() + t.bfloat16()).float()

    def forward(self, x, cond=None):
        hip.require_gpu(x, cond)
        B = x.shape[0]
        h = F_.Linear.apply(x, self.proj_in.weight, self.proj_in.bias)
        context = None
        if self.cond_tokens > 0:
            if cond is None:
                raise ValueError(f"Model initialized with cond_tokens={self.cond_tokens}, but no cond provided in forward().")
            context = self._context(cond)
        h = torch.cat([h, self.query_tokens(B)], dim=1)
        h = self.transformer(h, self._freqs(x.device), context=context)
        rows = F_.Linear.apply(h[:, self.in_tokens:], self.proj_out.weight, self.proj_out.bias)     # [B, grid, (pt ph pw c)]
        (t, hh, w), (pt, ph, pw), c = self.grid, self.patch_size, self.out_channels
        rows = rows.reshape(B, t, hh, w, pt, ph, pw, c).permute(0, 7, 1, 4, 2, 5, 3, 6)
        return rows.reshape(B, c, t * pt, hh * ph, w * pw)


@register("autoencoder_design")
class AutoEncoder(nn.Module):
    """autoencoder.py:8-135: a video encoder (1024 tokens), a first-frame encoder (256 tokens), ONE shared FSQ([8, 8, 8, 5, 5, 5]) and the
    decoder conditioned on the first-frame codes through cross attention.  Every reference keyword is accepted and ignored (the reference
    hard-codes 16 x 128 x 128 clips, (4, 8, 8) patches and the 'small' size); `_geometry` = dict(in_grid, patch_size, tokens, cond_tokens,
    model_size) overrides that for small tests."""
    output_format = "bcthw"

    def __init__(self, bottleneck=None, prior_model=None, _geometry=None, **kwargs):
        super().__init__()
        g = dict(in_grid=[16, 128, 128], patch_size=[4, 8, 8], tokens=1024, cond_tokens=256, model_size="small")
        g.update(_geometry or {})
        grid, ps, size, token_size = list(g["in_grid"]), tuple(g["patch_size"]), g["model_size"], 6
        self.encoder = Encoder(model_size=size, patch_size=ps, in_channels=3, out_channels=token_size, in_grid=grid, out_tokens=g["tokens"])
        self.first_frame_encoder = FirstFrameEncoder(model_size=size, patch_size_hw=ps[1:], in_channels=3, out_channels=token_size, in_hw=grid[1:],
                                                     out_tokens=g["cond_tokens"])
        self.quantize = FSQ(levels=[8, 8, 8, 5, 5, 5])
        self.decoder = UnifiedDecoder(model_size=size, patch_size=ps, in_channels=token_size, out_channels=3, in_tokens=g["tokens"],
                                      cond_tokens=g["cond_tokens"], out_grid=grid)
        self.prior_model = None

    def encode(self, data, **kwargs):
        """data [B, 3, T, H, W] -> (main_q, first_q, main_indices, first_indices); the last two are the quantizer's {'indices': int32} dicts,
        as in the reference"""
        main_tokens = self.encoder(data)
        first_tokens = self.first_frame_encoder(data[:, :, 0:1])
        main_q, main_indices = self.quantize(main_tokens)
        first_q, first_indices = self.quantize(first_tokens)
        return main_q, first_q, main_indices, first_indices

    def decode(self, main_q, first_q):
        return self.decoder(main_q, cond=first_q)

    def decode_from_indices(self, main_indices, first_indices):
        """index tensors, or the dicts `encode` returns"""
        main_indices, first_indices = (i["indices"] if isinstance(i, dict) else i for i in (main_indices, first_indices))
        return self.decode(self.quantize.indices_to_codes(main_indices), self.quantize.indices_to_codes(first_indices))

    def forward(self, x):
        main_q, first_q, _, _ = self.encode(x)
        return {"pred_frames": self.decode(main_q, first_q)}
