"""Layers of the reference's `autoencoder_design` (models/model_design/base/transformer.py) on the HIP kernels.

So far: `RMSNorm` and `CrossAttention`, the layer through which the design's decoder reads the 256 first-frame tokens (2048 queries
from one tensor, keys and values from another).  The self-attention variant of the block, the Perceiver-style encoders and the
registry entry of the whole model build on the same kernels and are not here yet; nothing in this module is registered by name
(the reference registers only the whole model).

Same constructor arguments and parameter names as the reference, so its state dicts load unchanged.  No CPU path.
"""
import torch
import torch.nn as nn

from . import functional as F_
from . import hip

RMS_WIDTHS = (128, 256, 384, 512, 768, 1024, 1280, 1536, 2560)      # vt_rmsnorm_any_*


class RMSNorm(nn.Module):
    """transformer.py:18-27.  Holds the weight and eps under the reference's parameter name; the arithmetic runs inside the fused layer
    (CrossAttention: vt_rmsnorm_any_* for norm_q / norm_kv, vt_head_rmsnorm_* per head for q_norm / k_norm), so there is no stand-alone forward."""

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

    def _pack(self, *names):
        """bf16 [N, K] and [K, N] operand copies of one weight, or of several concatenated along N; re-made when a weight changes"""
        ws = [getattr(self, n).weight for n in names]
        key = tuple((w.data_ptr(), w._version) for w in ws)
        cache = self.__dict__.setdefault("_vt_pack", {})
        hit = cache.get(names)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                w = torch.cat([t.detach() for t in ws], dim=0) if len(ws) > 1 else ws[0].detach()
                hit = (key, hip.pack_weight(w.float().contiguous()))
            cache[names] = hit
        return hit[1]

    def forward(self, x, context):
        hip.require_gpu(x, context, *self.parameters())
        return F_.CrossAttentionLayer.apply(x, context, self.norm_q.weight, self.norm_kv.weight, self.to_q.weight, self.to_kv.weight,
                                            self.to_gate.weight, self.q_norm.weight, self.k_norm.weight, self.out_proj.weight, self.heads,
                                            self.norm_q.eps, self._pack("to_q", "to_gate"), self._pack("to_kv"), self._pack("out_proj"))
