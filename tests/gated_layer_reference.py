"""The gated layer stack of titok.ResidualAttentionBlock as a per-layer composition of the library's own ops, one autograd Function per layer
(about 50 launches per layer, issued from Python): the bit-exact reference of the C++ stack engine (vt_gated_stack_forward / _backward issue the
same kernels on the same operands), and the layer that tests/test_titok_gpu.py pins against the oracle.  It was the product's forward before
the engine existed; it packs its weights on every call and caches nothing.  GPU only."""
import math

import torch

from video_tokenizer_amd import hip
from video_tokenizer_amd.functional import _pad64, gated_params


def pack_layer_weights(w_qkv, w_out, w_fc1, w_fc2):
    """bf16 [N, K] copies and [K, N] transposes of a layer's four matrices; fc2's contraction dim padded to a multiple of 64"""
    with torch.no_grad():
        return (*hip.pack_weight(w_qkv), *hip.pack_weight(w_out), *hip.pack_weight(w_fc1),
                *hip.pack_weight(w_fc2, k_pad=_pad64(w_fc2.shape[1])))


class GatedLayer(torch.autograd.Function):
    """x -> (x + Attn(x) ; + ffd(.)) * scale for one layer of ResidualAttentionBlock (transformer.py:45-63, 20-29, 82-91)."""

    @staticmethod
    def forward(ctx, x, cos, sin, n_head, scale, w_qkv, q_w, q_b, k_w, k_b, w_out, ln_w, ln_b, w_fc1, w_fc2):
        hip.require_gpu(x, cos, sin, w_qkv, w_out, w_fc1, w_fc2)
        B, L, D = x.shape
        M = B * L
        if M % 64 or D != 64 * n_head:
            raise hip.HipError(f"GatedLayer: B * L = {M} must be a multiple of 64 and width {D} = 64 * heads")
        inner = w_fc2.shape[1]
        ipad = _pad64(inner)
        x2 = x.contiguous().reshape(M, D).float()
        xb = hip.cast_rows(x2)
        wqkv_b, wqkv_t, wout_b, wout_t, wfc1_b, wfc1_t, wfc2_b, wfc2_t = pack_layer_weights(w_qkv, w_out, w_fc1, w_fc2)
        qkvg = hip.gemm_nt(xb, wqkv_b, hip.EPI_BF16)
        qkv = hip.qknorm_rope_fwd(qkvg, L, n_head, q_w, q_b, k_w, k_b, 1e-5, cos, sin)
        o, lse = hip.attention_fwd(qkv, B, L, n_head, 64)
        og = hip.sigmoid_gate_fwd(o, qkvg)
        x1 = hip.gemm_nt(og, wout_b, hip.EPI_F32, residual=x2, round_bf16=True)
        y, mean, rstd = hip.layernorm_fwd(x1, ln_w, ln_b, 1e-5)
        h = hip.gemm_nt(y, wfc1_b, hip.EPI_BF16)
        a = hip.geglu_fwd(h, lda=ipad)
        out = hip.gemm_nt(a, wfc2_b, hip.EPI_F32, residual=x1, round_bf16=True)
        if scale != 1.0:
            out.mul_(scale)
        ctx.save_for_backward(xb, qkvg, qkv, o, lse, og, x1, y, mean, rstd, h, a, cos, sin, q_w, k_w, ln_w, wqkv_t, wout_t, wfc1_t, wfc2_t)
        ctx.geom = (B, L, D, n_head, scale, inner)
        return out.reshape(B, L, D)

    @staticmethod
    def backward(ctx, dout):
        xb, qkvg, qkv, o, lse, og, x1, y, mean, rstd, h, a, cos, sin, q_w, k_w, ln_w, wqkv_t, wout_t, wfc1_t, wfc2_t = ctx.saved_tensors
        B, L, D, n_head, scale, inner = ctx.geom
        M = B * L
        dev = dout.device
        d2 = dout.contiguous().reshape(M, D).float()
        if scale != 1.0:
            d2 = d2 * scale
        # ffd backward
        gb = hip.cast_rows(d2)
        da = hip.gemm_nt(gb, wfc2_t, hip.EPI_BF16)                                   # [M, ipad]
        dw_fc2 = torch.empty(D, a.shape[1], device=dev)
        dh = hip.geglu_bwd(da, h)
        dy = hip.gemm_nt(dh, wfc1_t, hip.EPI_BF16)
        dw_fc1 = torch.empty(h.shape[1], D, device=dev)
        dx1, dx1b, d_ln_w, d_ln_b, _ = hip.layernorm_bwd(dy, x1, ln_w, mean, rstd, dres=d2, want_dxsum=False)
        # attention backward
        dog = hip.gemm_nt(dx1b, wout_t, hip.EPI_BF16)
        dw_out = torch.empty(D, D, device=dev)
        dqkvg = torch.empty_like(qkvg)
        d_o = hip.sigmoid_gate_bwd(dog, o, qkvg, dqkvg)
        dqkv = hip.attention_bwd(qkv, o, d_o, lse, B, L, n_head, 64)
        dq_w, dq_b, dk_w, dk_b = hip.qknorm_rope_bwd(qkvg, dqkv, L, n_head, q_w, k_w, 1e-5, cos, sin, dqkvg)
        dx = hip.gemm_nt(dqkvg, wqkv_t, hip.EPI_F32, residual=dx1, round_bf16=True)
        dw_qkv = torch.empty(4 * D, D, device=dev)
        hip.gemm_tn_grouped([dict(A=gb, B=a, out=dw_fc2), dict(A=dh, B=y, out=dw_fc1), dict(A=dx1b, B=og, out=dw_out),
                             dict(A=dqkvg, B=xb, out=dw_qkv)])
        return (dx.reshape(B, L, D), None, None, None, None, dw_qkv, dq_w, dq_b, dk_w, dk_b, dw_out, d_ln_w, d_ln_b, dw_fc1,
                dw_fc2[:, :inner].contiguous())


def reference_stack(block, x, freqs):
    """titok.ResidualAttentionBlock.forward(x, freqs) layer by layer: layer i scaled by 1 / sqrt(i + 1); differentiable in x and the parameters"""
    cos, sin = freqs
    params = gated_params(block)
    n = len(params) // block.num_layer
    for i in range(block.num_layer):
        x = GatedLayer.apply(x, cos, sin, block.heads, 1.0 / math.sqrt(i + 1), *params[i * n:(i + 1) * n])
    return x
