"""ctypes binding of libvt_hip.so (include/vt_hip.h).  PyTorch supplies device memory and the
stream; nothing here computes on the CPU.  Loading is lazy and LOUD: if the shared library is
missing (not built), `lib()` raises -- there is no fallback path."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VT_HIP_LIB") or os.path.join(_HERE, "libvt_hip.so")   # VT_HIP_LIB: A/B timing of two builds (tools/)
_lib = None

c_i32, c_i64, c_f32, c_u64, c_vp, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t

EPI_BF16, EPI_BF16_GELU, EPI_F32, EPI_BF16_DGELU, EPI_BF16_GELU_GRAD, EPI_BF16_MULAUX = 0, 1, 2, 3, 4, 5
TN_MAX_GROUP = 16


class RowMap(ctypes.Structure):
    _fields_ = [("grp", c_i32), ("stride", c_i64), ("off", c_i64)]


IDENT = RowMap(0, 0, 0)


class GemmNT(ctypes.Structure):
    _fields_ = [("A", c_vp), ("lda", c_i64), ("B", c_vp), ("ldb", c_i64), ("M", c_i32), ("N", c_i32), ("K", c_i32),
                ("epi", c_i32), ("out", c_vp), ("ldo", c_i64), ("out2", c_vp), ("ldo2", c_i64), ("bias", c_vp),
                ("residual", c_vp), ("ldr", c_i64), ("rowmod", c_vp), ("rowmod_period", c_i32), ("aux", c_vp),
                ("ldaux", c_i64), ("omap", RowMap), ("round_bf16", c_i32), ("colsum_partial", c_vp), ("out_scale", c_f32), ("tile", c_i32),
                ("splitk_ws", c_vp), ("splitk_ws_bytes", c_i64), ("splitk", c_i32)]


class GemmTN(ctypes.Structure):
    _fields_ = [("A", c_vp), ("lda", c_i64), ("B", c_vp), ("ldb", c_i64), ("M", c_i32), ("P", c_i32), ("Q", c_i32),
                ("out", c_vp), ("ldo", c_i64), ("p_lim", c_i32), ("q_lim", c_i32), ("row_perm", c_vp), ("tile", c_i32)]

class Clip(ctypes.Structure):
    """vtClip: one clip of vt_patchify_clips / vt_unpatchify_clips, a contiguous fp32 [C, T, H, W] on the device"""
    _fields_ = [("data", c_vp), ("T", c_i32), ("H", c_i32), ("W", c_i32)]


# Tile generation the gemm_nt / gemm_tn_grouped wrappers below put into vtGemmNT.tile / vtGemmTN.tile when the caller
# passes none: 0 = the library's automatic choice.  Tests and tools set it to A/B the tile generations; it lives on the
# Python side only (the C library has no setting of its own, the field travels with every call).
GEMM_TILE = 0


# every symbol include/vt_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "vt_abi_version": (c_i32, []),
    "vt_last_error": (c_i32, [ctypes.c_char_p, c_sz]),
    "vt_gemm_nt": (c_i32, [ctypes.POINTER(GemmNT), c_vp]),
    "vt_gemm_nt_splitk_workspace_bytes": (c_sz, []),
    "vt_gemm_tn_grouped": (c_i32, [ctypes.POINTER(GemmTN), c_i32, c_vp]),
    "vt_layernorm_fwd": (c_i32, [c_vp, RowMap, c_vp, c_vp, c_f32, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vt_layernorm_bwd_workspace_bytes": (c_sz, [c_i32]),
    "vt_layernorm_bwd": (c_i32, [c_vp, c_vp, RowMap, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_colsum_workspace_bytes": (c_sz, [c_i32]),
    "vt_colsum": (c_i32, [c_vp, c_i32, c_i64, RowMap, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_batch_sum": (c_i32, [c_vp, RowMap, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_cast_rows": (c_i32, [c_vp, RowMap, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "vt_zero_rows": (c_i32, [c_vp, c_vp, RowMap, c_i64, c_i32, c_vp]),
    "vt_sum_slabs": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp]),
    "vt_assemble_rows": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vt_pack_weight": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vt_patchify": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_unpatchify": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_patchify_dual": (c_i32, [c_vp] + [c_i32] * 10 + [c_vp, c_vp, c_vp]),
    "vt_unpatchify_dual": (c_i32, [c_vp, c_vp] + [c_i32] * 10 + [c_vp, c_vp]),
    "vt_conv3d_packed_elems": (c_sz, [c_i32, c_i32]),
    "vt_conv3d_pack_weight": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_conv3d_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp] + [c_i32] * 9 + [c_vp, c_vp]),
    "vt_conv3d_dgrad": (c_i32, [c_vp, c_vp] + [c_i32] * 9 + [c_vp, c_vp]),
    "vt_conv3d_wgrad_workspace_bytes": (c_sz, [c_i32] * 11),
    "vt_conv3d_wgrad": (c_i32, [c_vp, c_vp] + [c_i32] * 11 + [c_vp, c_vp, c_vp]),
    "vt_groupnorm_workspace_bytes": (c_sz, [c_i32, c_i64, c_i32, c_i32]),
    "vt_groupnorm_fwd": (c_i32, [c_vp, c_vp, c_vp, c_f32, c_i32, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_groupnorm_bwd": (c_i32, [c_vp] * 6 + [c_i32, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_upsample_nearest_fwd": (c_i32, [c_vp] + [c_i32] * 8 + [c_vp, c_vp]),
    "vt_upsample_nearest_bwd": (c_i32, [c_vp] + [c_i32] * 8 + [c_vp, c_vp]),
    "vt_video_to_channels_last": (c_i32, [c_vp] + [c_i32] * 6 + [c_vp, c_vp]),
    "vt_channels_last_to_video": (c_i32, [c_vp] + [c_i32] * 6 + [c_vp, c_vp]),
    "vt_attention_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_causal_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_causal_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_fwd_rows": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_bwd_rows": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_cross_fwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_attention_cross_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64,
                                       c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "vt_attention_varlen_fwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp,
                                        c_vp]),
    "vt_attention_varlen_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32,
                                        c_i32, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "vt_patchify_clips": (c_i32, [ctypes.POINTER(Clip), c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "vt_unpatchify_clips": (c_i32, [c_vp, c_i64, ctypes.POINTER(Clip), c_i32, c_i32, c_i32, c_i32, c_vp]),
    "vt_packed_scatter": (c_i32, [c_vp, c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_packed_gather": (c_i32, [c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "vt_packed_segment_colsum_workspace_bytes": (c_sz, [c_i32]),
    "vt_packed_segment_colsum": (c_i32, [c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vt_vq_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32]),
    "vt_vq_forward": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_u64, c_vp, c_vp,
                              c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vt_vq_forward_ctr": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_u64, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vt_vq_backward": (c_i32, [c_vp, c_i64, c_vp, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                               c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vt_vq_prep_codebook": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vt_vq_gather": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "vt_adam_step": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp, c_f32, c_vp]),
    "vt_fsq_codebook_size": (c_i32, [ctypes.POINTER(c_i32), c_i32, ctypes.POINTER(c_i64)]),
    "vt_fsq_forward": (c_i32, [c_vp, c_i32, c_i64, c_i32, ctypes.POINTER(c_i32), c_vp, c_vp, c_vp]),
    "vt_fsq_backward": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i32, ctypes.POINTER(c_i32), c_vp, c_vp]),
    "vt_fsq_indices_to_codes": (c_i32, [c_vp, c_i64, c_i32, ctypes.POINTER(c_i32), c_vp, c_i32, c_vp]),
    "vt_stat_gate_workspace_bytes": (c_sz, [c_i32]),
    "vt_stat_gate_forward": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32, c_u64, c_vp, c_vp, c_vp,
                                     c_vp, c_vp, c_vp]),
    "vt_stat_gate_backward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_kl_forward": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_u64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "vt_kl_backward": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "vt_qknorm_rope_fwd": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "vt_qknorm_rope_bwd_workspace_bytes": (c_sz, []),
    "vt_qknorm_rope_bwd": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_qknorm_rope_gqa_fwd": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "vt_qknorm_rope_gqa_bwd_workspace_bytes": (c_sz, []),
    "vt_qknorm_rope_gqa_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_vp]),
    "vt_rope_rotate": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp]),
    "vt_sigmoid_gate_fwd": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vt_sigmoid_gate_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_sigmoid_gate_cols_fwd": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "vt_sigmoid_gate_cols_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "vt_geglu_fwd": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "vt_geglu_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vt_scale_rows": (c_i32, [c_vp, c_f32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_fwd": (c_i32, [c_vp, c_vp, c_f32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_bwd_workspace_bytes": (c_sz, [c_i32]),
    "vt_rmsnorm_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_any_fwd": (c_i32, [c_vp, c_vp, c_f32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_any_bwd_workspace_bytes": (c_sz, [c_i32]),
    "vt_rmsnorm_any_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_head_rmsnorm_fwd": (c_i32, [c_vp, c_i64, c_vp, c_f32, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "vt_head_rmsnorm_bwd_workspace_bytes": (c_sz, []),
    "vt_head_rmsnorm_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_f32, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vt_qkrms_rope_fwd": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "vt_qkrms_rope_bwd_workspace_bytes": (c_sz, []),
    "vt_qkrms_rope_bwd": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "vt_residual_scale_fwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vt_residual_scale_bwd_workspace_bytes": (c_sz, []),
    "vt_residual_scale_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_any_f32_fwd": (c_i32, [c_vp, c_vp, c_f32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vt_rmsnorm_any_f32_bwd_workspace_bytes": (c_sz, [c_i32]),
    "vt_rmsnorm_any_f32_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vt_swiglu_fwd": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vt_swiglu_bwd": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vt_decode_attention": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_vp, c_vp]),
    "vt_decode_attention_step": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_vp, c_vp, c_vp]),
    "vt_decode_norm_linear": (c_i32, [c_vp, c_vp, c_f32, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
}


class TokenizerConfig(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("B", "C", "T", "S", "pt", "p", "D", "H", "depth_enc", "depth_dec", "Nq", "d", "K", "vq_mode", "l2_normalized")] + \
               [(n, c_f32) for n in ("inv_tau", "beta", "codebook_w")] + [("freeze_codebook", c_i32)]


BLOCK_FIELDS = ("norm1_w", "norm1_b", "qkv_w", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


class BlockTensors(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in BLOCK_FIELDS]


class PackJob(ctypes.Structure):
    _fields_ = [("w", c_vp), ("N", c_i32), ("K", c_i32), ("row_perm", c_vp), ("wb", c_vp), ("ldd", c_i64), ("wt", c_vp), ("lddT", c_i64)]


class StackConfig(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("B", "L", "D", "H", "depth")]


class GatedStackConfig(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("B", "L", "D", "H", "depth", "inner")]


GATED_FIELDS = ("to_qkv_w", "q_norm_w", "q_norm_b", "k_norm_w", "k_norm_b", "out_proj_w", "ln_w", "ln_b", "fc1_w", "fc2_w")


class GatedLayerTensors(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in GATED_FIELDS]


TENSOR_FIELDS = ("pe_w", "pe_b", "enc_patch_pe", "enc_query", "dec_latent_pe", "dec_patch_query", "dec_token_type", "in_w", "in_b",
                 "out_w", "out_b", "codebook", "head_norm_w", "head_norm_b", "head_w", "head_b")


class TokenizerTensors(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in TENSOR_FIELDS] + [("enc_blocks", ctypes.POINTER(BlockTensors)), ("dec_blocks", ctypes.POINTER(BlockTensors))]


OUTPUT_FIELDS = ("pred_frames", "encoded", "indices", "projected_z", "unregularized_z", "regularized_z", "emb", "losses", "input_norms")


class TokenizerOutputs(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in OUTPUT_FIELDS]


KL_OUTPUT_FIELDS = ("encoded", "mean", "projected_z", "regularized_z", "noise", "loss_kl", "input_norms")


class TokenizerKLOutputs(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in KL_OUTPUT_FIELDS]


_TT = ctypes.POINTER(TokenizerTensors)
ENGINE_SIGNATURES = {
    "vt_pack_weights_grouped": (c_i32, [ctypes.POINTER(PackJob), c_i32, c_vp]),
    "vt_stack_create": (c_i32, [ctypes.POINTER(StackConfig), ctypes.POINTER(c_vp)]),
    "vt_stack_destroy": (None, [c_vp]),
    "vt_stack_workspace_bytes": (c_sz, [c_vp]),
    "vt_stack_init_workspace": (c_i32, [c_vp, c_vp, c_vp]),
    "vt_stack_forward": (c_i32, [c_vp, ctypes.POINTER(BlockTensors), c_vp, c_vp, c_vp, c_vp]),
    "vt_stack_backward": (c_i32, [c_vp, ctypes.POINTER(BlockTensors), c_vp, c_vp, ctypes.POINTER(BlockTensors), c_vp, c_i32, c_vp]),
    "vt_stack_forward_rotary": (c_i32, [c_vp, ctypes.POINTER(BlockTensors), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vt_stack_backward_rotary": (c_i32, [c_vp, ctypes.POINTER(BlockTensors), c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(BlockTensors), c_vp, c_i32, c_vp]),
    "vt_gated_stack_create": (c_i32, [ctypes.POINTER(GatedStackConfig), ctypes.POINTER(c_vp)]),
    "vt_gated_stack_destroy": (None, [c_vp]),
    "vt_gated_stack_workspace_bytes": (c_sz, [c_vp]),
    "vt_gated_stack_init_workspace": (c_i32, [c_vp, c_vp, c_vp]),
    "vt_gated_stack_forward": (c_i32, [c_vp, ctypes.POINTER(GatedLayerTensors), c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "vt_gated_stack_backward": (c_i32, [c_vp, ctypes.POINTER(GatedLayerTensors), c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(GatedLayerTensors), c_vp, c_vp]),
    "vt_tokenizer_create": (c_i32, [ctypes.POINTER(TokenizerConfig), ctypes.POINTER(c_vp)]),
    "vt_tokenizer_destroy": (None, [c_vp]),
    "vt_tokenizer_workspace_bytes": (c_sz, [c_vp]),
    "vt_tokenizer_init_workspace": (c_i32, [c_vp, c_vp, c_vp]),
    "vt_tokenizer_pack": (c_i32, [c_vp, _TT, c_vp, c_vp]),
    "vt_tokenizer_encode": (c_i32, [c_vp, _TT, c_vp, c_vp, ctypes.POINTER(TokenizerOutputs), c_u64, c_vp]),
    "vt_tokenizer_decode": (c_i32, [c_vp, _TT, c_vp, c_vp, c_vp, c_vp]),
    "vt_tokenizer_codes_to_encoded": (c_i32, [c_vp, _TT, c_vp, c_vp, c_vp, c_vp]),
    "vt_tokenizer_num_backward_stages": (c_i32, [c_vp]),
    "vt_tokenizer_set_seed_counter": (c_i32, [c_vp, c_vp]),
    "vt_tokenizer_set_split_k": (c_i32, [c_vp, c_i32]),
    "vt_tokenizer_set_wgrad_tail": (c_i32, [c_vp, c_i32]),
    "vt_tokenizer_set_wgrad_stream": (c_i32, [c_vp, c_vp]),
    "vt_tokenizer_set_wgrad_batch": (c_i32, [c_vp, c_i32]),
    "vt_stack_set_split_k": (c_i32, [c_vp, c_i32]),
    "vt_tokenizer_backward": (c_i32, [c_vp, _TT, c_vp, c_vp, c_vp, _TT, c_i32, c_i32, ctypes.POINTER(c_i32), c_vp]),
    "vt_tokenizer_set_data_parallel": (c_i32, [c_vp, c_i32]),
    "vt_tokenizer_backward_until_flush": (c_i32, [c_vp, _TT, c_vp, c_vp, c_vp, _TT, c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_vp]),
    "vt_tokenizer_create_kl": (c_i32, [ctypes.POINTER(TokenizerConfig), ctypes.POINTER(c_vp)]),
    "vt_tokenizer_encode_kl": (c_i32, [c_vp, _TT, c_vp, c_vp, ctypes.POINTER(TokenizerKLOutputs), c_u64, c_vp]),
}


def lib():
    """Load libvt_hip.so (built in-tree by video-tokenizer_amd/build.py).  Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python video-tokenizer_amd/build.py` "
                               "(there is no CPU fallback for the tokenizer hot path)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(ENGINE_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class HipError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        buf = ctypes.create_string_buffer(512)
        lib().vt_last_error(buf, 512)
        raise HipError(f"{what} failed ({rc}): {buf.value.decode(errors='replace')}")


def ptr(t):
    """device pointer of a tensor (None -> NULL); refuses CPU tensors loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("libvt_hip operates on GPU tensors only (no CPU path)")
    return ctypes.c_void_p(t.data_ptr())


def require_gpu(*tensors):
    """every compute entry point of this package is GPU-only: refuse CPU tensors before anything is allocated"""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipError("libvt_hip operates on GPU tensors only (no CPU path)")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------
# thin op-level wrappers (used by tests and by the module for the few ops outside the engine)
# ---------------------------------------------------------------------------------------------

GEMM_SPLITK = True       # False: gemm_nt never hands vt_gemm_nt a split-K workspace (A/B switch of tools and tests)
_SPLITK_WS = {}


def splitk_workspace(dev):
    """the zeroed split-K workspace of vt_gemm_nt for the current stream of `dev` (one per stream: the arrival counters in its
    first 4 KiB belong to one launch at a time)"""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = torch.zeros(lib().vt_gemm_nt_splitk_workspace_bytes(), device=dev, dtype=torch.uint8)
        _SPLITK_WS[key] = ws
    return ws


def gemm_nt(A, B, epi=EPI_BF16, bias=None, out=None, out2=None, residual=None, rowmod=None, rowmod_period=0,
            aux=None, omap=None, round_bf16=False, out_rows=None, colsum_partial=None, tile=None, out_scale=0.0, splitk=1):
    """C = A @ B.T with the fused epilogue `epi`; A [M,K] bf16, B [N,K] bf16 (row-major, contiguous).
    splitk: 1 = never split K (default: the result's bits do not depend on how many rows share the launch), None = the library's
    automatic split for launches that leave most CUs idle (vtGemmNT.splitk_ws; a workspace per device and stream is kept here),
    2..8 = forced (tests)."""
    require_gpu(A, B)
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    M, K = A.shape
    N = B.shape[0]
    dev = A.device
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty(rows, N, device=dev, dtype=torch.float32 if epi == EPI_F32 else torch.bfloat16)
    if epi in (EPI_BF16_GELU, EPI_BF16_GELU_GRAD) and out2 is None:
        out2 = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    p = GemmNT()
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0)
    p.M, p.N, p.K, p.epi = M, N, K, epi
    p.out, p.ldo = out.data_ptr(), out.stride(0)
    p.out2, p.ldo2 = (out2.data_ptr(), out2.stride(0)) if out2 is not None else (None, 0)
    p.bias = bias.data_ptr() if bias is not None else None
    p.residual, p.ldr = (residual.data_ptr(), residual.stride(0)) if residual is not None else (None, 0)
    p.rowmod, p.rowmod_period = (rowmod.data_ptr(), rowmod_period) if rowmod is not None else (None, 0)
    p.aux, p.ldaux = (aux.data_ptr(), aux.stride(0)) if aux is not None else (None, 0)
    p.omap = omap if omap is not None else IDENT
    p.round_bf16 = int(round_bf16)
    p.colsum_partial = colsum_partial.data_ptr() if colsum_partial is not None else None
    p.tile = GEMM_TILE if tile is None else tile
    p.out_scale = float(out_scale)
    if splitk != 1 and GEMM_SPLITK:
        ws = splitk_workspace(dev)
        p.splitk_ws, p.splitk_ws_bytes, p.splitk = ws.data_ptr(), ws.numel(), 0 if splitk is None else int(splitk)
    else:
        p.splitk_ws, p.splitk_ws_bytes, p.splitk = None, 0, 1
    check(lib().vt_gemm_nt(ctypes.byref(p), stream()), "vt_gemm_nt")
    return (out, out2) if epi in (EPI_BF16_GELU, EPI_BF16_GELU_GRAD) else out


def gemm_tn_grouped(problems):
    """problems: list of dicts(A=dY [M,P] bf16, B=X [M,Q] bf16, out fp32 [p_lim, >=q_lim], p_lim, q_lim, row_perm)."""
    arr = (GemmTN * len(problems))()
    for i, pr in enumerate(problems):
        A, B, out = pr["A"], pr["B"], pr["out"]
        g = arr[i]
        g.A, g.lda, g.B, g.ldb = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0)
        g.M, g.P, g.Q = A.shape[0], A.shape[1], B.shape[1]
        g.out, g.ldo = out.data_ptr(), out.stride(0)
        g.p_lim = pr.get("p_lim", A.shape[1])
        g.q_lim = pr.get("q_lim", B.shape[1])
        rp = pr.get("row_perm")
        g.row_perm = rp.data_ptr() if rp is not None else None
        g.tile = pr.get("tile", GEMM_TILE)
    check(lib().vt_gemm_tn_grouped(arr, len(problems), stream()), "vt_gemm_tn_grouped")


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def layernorm_fwd(x, gamma, beta, eps, rows=None, xmap=None, y=None):
    dim = x.shape[-1]
    rows = rows if rows is not None else x.numel() // dim
    y = torch.empty(rows, dim, device=x.device, dtype=torch.bfloat16) if y is None else y
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    check(lib().vt_layernorm_fwd(ptr(x), xmap or IDENT, ptr(gamma), ptr(beta), eps, rows, dim, ptr(y), ptr(mean), ptr(rstd), stream()), "vt_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, xmap=None, dx=None, dxb=None, want_dxsum=True, want_dxb=True):
    rows, dim = dy.shape
    dev = x.device
    dx = torch.empty_like(x) if dx is None else dx
    dxb = torch.empty(x.shape, device=dev, dtype=torch.bfloat16) if dxb is None and want_dxb else dxb
    dg, db = torch.empty(dim, device=dev), torch.empty(dim, device=dev)
    ds = torch.empty(dim, device=dev) if want_dxsum else None
    ws = _ws(lib().vt_layernorm_bwd_workspace_bytes(dim), dev)
    check(lib().vt_layernorm_bwd(ptr(dy), ptr(x), xmap or IDENT, ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), rows, dim, ptr(dx),
                                 ptr(dxb), ptr(dg), ptr(db), ptr(ds), ptr(ws), stream()), "vt_layernorm_bwd")
    return dx, dxb, dg, db, ds


def colsum(src, rows=None, rmap=None):
    width = src.shape[-1]
    rows = rows if rows is not None else src.numel() // width
    out = torch.empty(width, device=src.device, dtype=torch.float32)
    ws = _ws(lib().vt_colsum_workspace_bytes(width), src.device)
    check(lib().vt_colsum(ptr(src), int(src.dtype == torch.bfloat16), src.stride(-2), rmap or IDENT, rows, width, ptr(out), ptr(ws), stream()), "vt_colsum")
    return out


def batch_sum(src, batch, n, rmap=None):
    dim = src.shape[-1]
    out = torch.empty(n, dim, device=src.device, dtype=torch.float32)
    check(lib().vt_batch_sum(ptr(src), rmap or IDENT, batch, n, dim, ptr(out), stream()), "vt_batch_sum")
    return out


def cast_rows(src, rows=None, rmap=None, ldd=None, dst=None):
    dim = src.shape[-1]
    rows = rows if rows is not None else src.numel() // dim
    ldd = ldd or (dst.stride(0) if dst is not None else dim)
    if dst is None:     # pad columns (ldd > dim) must read as zeros; a dense destination is fully overwritten
        dst = (torch.zeros if ldd != dim else torch.empty)(rows, ldd, device=src.device, dtype=torch.bfloat16)
    check(lib().vt_cast_rows(ptr(src), rmap or IDENT, rows, dim, ptr(dst), ldd, stream()), "vt_cast_rows")
    return dst


def assemble_rows(dst, seq, off, batch, n, src=None, table=None, vec=None):
    check(lib().vt_assemble_rows(ptr(dst), seq, off, batch, n, dst.shape[-1], ptr(src), ptr(table), ptr(vec), stream()), "vt_assemble_rows")


def zero_rows(a=None, b=None, rows=None, rmap=None):
    """zeroes rows rmap(r), r < rows, of the fp32 matrix `a` [*, dim] and / or its bf16 twin `b`, in place"""
    require_gpu(a, b)
    t = a if a is not None else b
    dim = t.shape[-1]
    rows = rows if rows is not None else t.numel() // dim
    check(lib().vt_zero_rows(ptr(a), ptr(b), rmap or IDENT, rows, dim, stream()), "vt_zero_rows")


def sum_slabs(slabs, nslab, width, slab_stride=None):
    """out[c] = sum_s slabs[s * slab_stride + c] (fp32, fixed order); slab_stride defaults to width (dense slabs)"""
    require_gpu(slabs)
    out = torch.empty(width, device=slabs.device, dtype=torch.float32)
    check(lib().vt_sum_slabs(ptr(slabs), nslab, slab_stride or width, width, ptr(out), stream()), "vt_sum_slabs")
    return out


def scale_rows(src, scale, dst=None, dstb=None):
    """dst = scale * src (fp32; dst may be src) and / or dstb = its bf16 copy; at least one of the two"""
    require_gpu(src, dst, dstb)
    dim = src.shape[-1]
    check(lib().vt_scale_rows(ptr(src), scale, src.numel() // dim, dim, ptr(dst), ptr(dstb), stream()), "vt_scale_rows")


def pack_weight(w, row_perm=None, want_t=True, ldd=None, lddT=None, n_pad=None, k_pad=None):
    w2 = w.reshape(w.shape[0], -1)
    N, K = w2.shape
    ldd = ldd or (k_pad or K)
    lddT = lddT or (n_pad or N)
    dense = (n_pad or N) == N and (k_pad or K) == K and ldd == K and lddT == N      # no padding anywhere: fully overwritten
    alloc = torch.empty if dense else torch.zeros
    wb = alloc(n_pad or N, ldd, device=w.device, dtype=torch.bfloat16)
    wt = alloc(k_pad or K, lddT, device=w.device, dtype=torch.bfloat16) if want_t else None
    check(lib().vt_pack_weight(ptr(w2), N, K, ptr(row_perm), ptr(wb), ldd, ptr(wt), lddT, stream()), "vt_pack_weight")
    return wb, wt


def dual_grids(T, H, W, T0, pt0, pt1, ph, pw):
    """tokens per clip of the two temporal segments of vt_patchify_dual: (N0, N1)"""
    return (T0 // pt0) * (H // ph) * (W // pw), ((T - T0) // pt1) * (H // ph) * (W // pw)


def _patch_ends(shape, pts, ph, pw, video, rows, rows_dtype):
    """the shapes and allocations of the four dense patch wrappers: video fp32 [B, C, T, H, W] and, per temporal segment of `frames` frames and
    temporal patch pt in pts = ((frames, pt), ...), a row matrix [B * (frames / pt)(H / ph)(W / pw), C pt ph pw] of rows_dtype.  What is None is
    allocated, what is given must be contiguous, of that dtype and large enough; -> (video, rows)"""
    B, C, T, H, W = shape
    dev = (video if video is not None else rows[0]).device
    sizes = [(B * (frames // pt) * (H // ph) * (W // pw), C * pt * ph * pw) for frames, pt in pts]
    video = torch.empty(shape, device=dev, dtype=torch.float32) if video is None else video
    rows = [torch.empty(size, device=dev, dtype=rows_dtype) if r is None else r for r, size in zip(rows, sizes)]
    assert video.dtype == torch.float32 and video.is_contiguous() and video.numel() >= B * C * T * H * W
    for r, (n, kp) in zip(rows, sizes):
        assert r.dtype == rows_dtype and r.is_contiguous() and r.numel() >= n * kp
    return video, rows


def patchify(video, pt, p, rows=None):
    """video fp32 [B, C, T, S, S] -> rows bf16 [B * (T / pt)(S / p)^2, C pt p p]"""
    B, C, T, S, _ = video.shape
    video, (rows,) = _patch_ends(video.shape, ((T, pt),), p, p, video, (rows,), torch.bfloat16)
    check(lib().vt_patchify(ptr(video), B, C, T, S, pt, p, ptr(rows), stream()), "vt_patchify")
    return rows


def unpatchify(rows, B, C, T, S, pt, p, video=None):
    """the inverse on an fp32 row matrix -> video fp32 [B, C, T, S, S]"""
    video, (rows,) = _patch_ends((B, C, T, S, S), ((T, pt),), p, p, video, (rows,), torch.float32)
    check(lib().vt_unpatchify(ptr(rows), B, C, T, S, pt, p, ptr(video), stream()), "vt_unpatchify")
    return video


def patchify_dual(video, T0, pt0, pt1, ph, pw, rows0=None, rows1=None):
    """video fp32 [B, C, T, H, W] -> (rows0 bf16 [B * N0, C pt0 ph pw], rows1 bf16 [B * N1, C pt1 ph pw]): frames [0, T0) and [T0, T), one launch"""
    B, C, T, H, W = video.shape
    video, (rows0, rows1) = _patch_ends(video.shape, ((T0, pt0), (T - T0, pt1)), ph, pw, video, (rows0, rows1), torch.bfloat16)
    check(lib().vt_patchify_dual(ptr(video), B, C, T, H, W, T0, pt0, pt1, ph, pw, ptr(rows0), ptr(rows1), stream()), "vt_patchify_dual")
    return rows0, rows1


def unpatchify_dual(rows0, rows1, B, C, T, H, W, T0, pt0, pt1, ph, pw, video=None):
    """the inverse on two fp32 row matrices -> video fp32 [B, C, T, H, W], one launch"""
    video, (rows0, rows1) = _patch_ends((B, C, T, H, W), ((T0, pt0), (T - T0, pt1)), ph, pw, video, (rows0, rows1), torch.float32)
    check(lib().vt_unpatchify_dual(ptr(rows0), ptr(rows1), B, C, T, H, W, T0, pt0, pt1, ph, pw, ptr(video), stream()), "vt_unpatchify_dual")
    return video


def attention_fwd(qkv, B, L, H, hd=64, o=None, q_begin=0):
    """q_begin > 0: only the queries q_begin..L-1; o is then compact [B * (L - q_begin), H * hd]"""
    o = torch.empty(B * (L - q_begin), H * hd, device=qkv.device, dtype=torch.bfloat16) if o is None else o
    lse2 = torch.zeros(B, H, L, device=qkv.device, dtype=torch.float32) if q_begin else torch.empty(B, H, L, device=qkv.device, dtype=torch.float32)
    check(lib().vt_attention_fwd_rows(ptr(qkv), B, L, H, hd, q_begin, ptr(o), ptr(lse2), stream()), "vt_attention_fwd")
    return o, lse2


def attention_bwd(qkv, o, dO, lse2, B, L, H, hd=64, dqkv=None, q_begin=0):
    """the two-kernel backward (dQ + dK/dV, recompute from lse2); dqkv in the packed layout of qkv"""
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    delta = torch.zeros(B, H, L, device=qkv.device, dtype=torch.float32)
    check(lib().vt_attention_bwd_rows(ptr(qkv), ptr(o), ptr(dO), ptr(lse2), B, L, H, hd, q_begin, ptr(dqkv), ptr(delta), stream()), "vt_attention_bwd")
    return dqkv


def attention_causal_fwd(qkv, B, L, H):
    """F.scaled_dot_product_attention(q, k, v, is_causal=True) on the packed projection [B * L, 3 * H * 64]"""
    o = torch.empty(B * L, H * 64, device=qkv.device, dtype=torch.bfloat16)
    lse2 = torch.empty(B, H, L, device=qkv.device, dtype=torch.float32)
    check(lib().vt_attention_causal_fwd(ptr(qkv), B, L, H, ptr(o), ptr(lse2), stream()), "vt_attention_causal_fwd")
    return o, lse2


def attention_causal_bwd(qkv, o, dO, lse2, B, L, H):
    dqkv = torch.empty_like(qkv)
    delta = torch.zeros(B, H, L, device=qkv.device, dtype=torch.float32)
    check(lib().vt_attention_causal_bwd(ptr(qkv), ptr(o), ptr(dO), ptr(lse2), B, L, H, ptr(dqkv), ptr(delta), stream()), "vt_attention_causal_bwd")
    return dqkv


def _rows_view(t, what):
    """a bf16 matrix view with unit column stride (rows of a wider buffer allowed) -> its row stride in elements"""
    if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
        raise HipError(f"{what}: expected a 2-D bf16 view with unit column stride, got {t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
    return t.stride(0)


def attention_cross_fwd(q, k, v, B, Lq, Lk, H, hd=64):
    """softmax(q k^T / 8) v with the queries and the keys / values in separate (strided) operands: q a view [B * Lq, 64 H] of any wider
    bf16 buffer, k and v views [B * Lk, 64 H] likewise -> (o bf16 [B * Lq, 64 H], lse2 fp32 [B, H, Lq])"""
    require_gpu(q, k, v)
    D = H * hd
    assert tuple(q.shape) == (B * Lq, D) and tuple(k.shape) == (B * Lk, D) == tuple(v.shape)
    o = torch.empty(B * Lq, D, device=q.device, dtype=torch.bfloat16)
    lse2 = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32)
    check(lib().vt_attention_cross_fwd(ptr(q), _rows_view(q, "q"), ptr(k), _rows_view(k, "k"), ptr(v), _rows_view(v, "v"), B, Lq, Lk, H, hd,
                                       ptr(o), ptr(lse2), stream()), "vt_attention_cross_fwd")
    return o, lse2


def attention_cross_bwd(q, k, v, o, dO, lse2, B, Lq, Lk, H, hd=64, dq=None, dk=None, dv=None):
    """-> (dq, dk, dv); each may be passed as a view [rows, 64 H] of a wider bf16 buffer, whose other columns are left alone"""
    require_gpu(q, k, v, o, dO, lse2, dq, dk, dv)
    D = H * hd
    assert tuple(q.shape) == (B * Lq, D) and tuple(k.shape) == (B * Lk, D) == tuple(v.shape)
    assert o.is_contiguous() and dO.is_contiguous() and tuple(o.shape) == (B * Lq, D) == tuple(dO.shape)
    dq = torch.empty(B * Lq, D, device=q.device, dtype=torch.bfloat16) if dq is None else dq
    dk = torch.empty(B * Lk, D, device=q.device, dtype=torch.bfloat16) if dk is None else dk
    dv = torch.empty(B * Lk, D, device=q.device, dtype=torch.bfloat16) if dv is None else dv
    assert tuple(dq.shape) == (B * Lq, D) and tuple(dk.shape) == (B * Lk, D) == tuple(dv.shape)
    delta = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32)
    check(lib().vt_attention_cross_bwd(ptr(q), _rows_view(q, "q"), ptr(k), _rows_view(k, "k"), ptr(v), _rows_view(v, "v"), ptr(o), ptr(dO), ptr(lse2),
                                       B, Lq, Lk, H, hd, ptr(dq), _rows_view(dq, "dq"), ptr(dk), _rows_view(dk, "dk"), ptr(dv), _rows_view(dv, "dv"),
                                       ptr(delta), stream()), "vt_attention_cross_bwd")
    return dq, dk, dv


VARLEN_MAX_SEQ = 64      # VT_VARLEN_MAX_SEQ


def cu_seqlens_list(cu_seqlens):
    """sequence boundaries as a list of Python ints: from a list / tuple of ints, or a CPU or device int32 / int64 tensor.  THE conversion
    of the package (VarlenAttend, varlen.Attn and cu_seqlens_host all go through it), so a float tensor or a float in a list is refused
    here and nowhere truncated.  A DEVICE tensor is read back, which costs one synchronisation: build the list on the host where that matters."""
    if isinstance(cu_seqlens, torch.Tensor):
        if cu_seqlens.dim() != 1 or cu_seqlens.dtype not in (torch.int32, torch.int64):
            raise HipError(f"cu_seqlens: expected a 1-D int32 / int64 tensor, got {cu_seqlens.dtype} {tuple(cu_seqlens.shape)}")
        cu_seqlens = cu_seqlens.tolist()
    cu = []
    for c in cu_seqlens:
        if isinstance(c, bool) or int(c) != c or isinstance(c, float):
            raise HipError(f"cu_seqlens: boundaries must be integers, got {c!r}")
        cu.append(int(c))
    if len(cu) < 2:
        raise HipError("cu_seqlens: need at least one sequence (two boundaries)")
    if any(not -2**31 <= c < 2**31 for c in cu):
        raise HipError("cu_seqlens: a boundary does not fit int32")
    return cu


def cu_seqlens_host(cu_seqlens):
    """-> (the host int32 array the C ABI takes, n_seq, M).  The library validates the values (cu[0] == 0, strictly increasing, cu[n] == M, at
    most VARLEN_MAX_SEQ sequences)."""
    cu = cu_seqlens_list(cu_seqlens)
    return (c_i32 * len(cu))(*cu), len(cu) - 1, cu[-1]


def attention_varlen_fwd(q, k, v, cu_seqlens, Hq, Hkv, hd=64, o=None, lse2=None):
    """softmax(q k^T / 8) v inside every sequence of a packed batch: q a view [M, 64 Hq], k and v views [M, 64 Hkv] of wider bf16 buffers,
    sequence b = rows cu_seqlens[b] .. cu_seqlens[b+1]-1, query head h reads KV head h // (Hq // Hkv) -> (o bf16 [M, 64 Hq], lse2 fp32 [Hq, M])"""
    require_gpu(q, k, v)
    cu, n, _ = cu_seqlens_host(cu_seqlens)
    M = q.shape[0]
    assert tuple(q.shape) == (M, Hq * hd) and tuple(k.shape) == (M, Hkv * hd) == tuple(v.shape)
    o = torch.empty(M, Hq * hd, device=q.device, dtype=torch.bfloat16) if o is None else o
    lse2 = torch.empty(Hq, M, device=q.device, dtype=torch.float32) if lse2 is None else lse2
    assert o.is_contiguous() and tuple(o.shape) == (M, Hq * hd) and lse2.is_contiguous() and tuple(lse2.shape) == (Hq, M)
    check(lib().vt_attention_varlen_fwd(ptr(q), _rows_view(q, "q"), ptr(k), _rows_view(k, "k"), ptr(v), _rows_view(v, "v"), cu, n, M, Hq, Hkv, hd,
                                        ptr(o), ptr(lse2), stream()), "vt_attention_varlen_fwd")
    return o, lse2


def attention_varlen_bwd(q, k, v, o, dO, lse2, cu_seqlens, Hq, Hkv, hd=64, dq=None, dk=None, dv=None):
    """-> (dq [M, 64 Hq], dk, dv [M, 64 Hkv]); each may be passed as a view of a wider bf16 buffer, whose other columns are left alone"""
    require_gpu(q, k, v, o, dO, lse2, dq, dk, dv)
    cu, n, _ = cu_seqlens_host(cu_seqlens)
    M = q.shape[0]
    assert tuple(q.shape) == (M, Hq * hd) and tuple(k.shape) == (M, Hkv * hd) == tuple(v.shape)
    assert o.is_contiguous() and dO.is_contiguous() and tuple(o.shape) == (M, Hq * hd) == tuple(dO.shape)
    assert lse2.is_contiguous() and tuple(lse2.shape) == (Hq, M) and lse2.dtype == torch.float32
    dq = torch.empty(M, Hq * hd, device=q.device, dtype=torch.bfloat16) if dq is None else dq
    dk = torch.empty(M, Hkv * hd, device=q.device, dtype=torch.bfloat16) if dk is None else dk
    dv = torch.empty(M, Hkv * hd, device=q.device, dtype=torch.bfloat16) if dv is None else dv
    assert tuple(dq.shape) == (M, Hq * hd) and tuple(dk.shape) == (M, Hkv * hd) == tuple(dv.shape)
    delta = torch.empty(Hq, M, device=q.device, dtype=torch.float32)
    check(lib().vt_attention_varlen_bwd(ptr(q), _rows_view(q, "q"), ptr(k), _rows_view(k, "k"), ptr(v), _rows_view(v, "v"), ptr(o), ptr(dO), ptr(lse2),
                                        cu, n, M, Hq, Hkv, hd, ptr(dq), _rows_view(dq, "dq"), ptr(dk), _rows_view(dk, "dk"), ptr(dv),
                                        _rows_view(dv, "dv"), ptr(delta), stream()), "vt_attention_varlen_bwd")
    return dq, dk, dv


# ---- data movement of the packed titok model (csrc/vt_packed.hip) ----
PACKED_LEAD, PACKED_TAIL = 0, 1      # VT_PACKED_LEAD / VT_PACKED_TAIL: which segment of every [lead | tail] sequence a call works on


def _clip_table(clips, C):
    """the vtClip host array of a list of fp32 [C, T, H, W] device tensors (the library validates sizes and alignment)"""
    require_gpu(*clips)
    for v in clips:
        if v.dim() != 4 or v.shape[0] != C or v.dtype != torch.float32 or not v.is_contiguous():
            raise HipError(f"clips: expected contiguous fp32 [{C}, T, H, W] tensors, got {v.dtype} {tuple(v.shape)} strides {tuple(v.stride())}")
    arr = (Clip * max(len(clips), 1))()
    for a, v in zip(arr, clips):
        a.data, a.T, a.H, a.W = v.data_ptr(), v.shape[1], v.shape[2], v.shape[3]
    return arr


def clip_grids(sizes, pt, p):
    """token grids [(T / pt, H / p, W / p)] of clips of the given (T, H, W)"""
    return [(int(T) // pt, int(H) // p, int(W) // p) for T, H, W in sizes]


def patchify_clips(clips, pt, p, out=None):
    """a list of fp32 [C, T_b, H_b, W_b] clips -> bf16 patch rows [sum_b G_b, C * pt * p * p], clip after clip, in ONE launch; columns
    (c, dt, dy, dx), tokens (t, h, w): per clip the rearrange of the reference's TiTokEncoder.forward"""
    C = clips[0].shape[0] if len(clips) else 0
    arr = _clip_table(clips, C)
    G = sum(t * h * w for t, h, w in clip_grids([v.shape[1:] for v in clips], pt, p))
    rows = torch.empty(G, C * pt * p * p, device=clips[0].device if len(clips) else None, dtype=torch.bfloat16) if out is None else out
    if out is not None and (out.dtype != torch.bfloat16 or tuple(out.shape) != (G, C * pt * p * p) or not out.is_contiguous() or not out.is_cuda):
        raise HipError(f"patchify_clips: out must be a contiguous bf16 device matrix [{G}, {C * pt * p * p}], got {out.dtype} {tuple(out.shape)}")
    check(lib().vt_patchify_clips(arr, len(clips), C, pt, p, ptr(rows), G, stream()), "vt_patchify_clips")
    return rows


def unpatchify_clips(rows, sizes, C, pt, p, out=None):
    """fp32 rows [sum_b G_b, C * pt * p * p] -> a list of fp32 [C, T_b, H_b, W_b] clips, sizes = [(T_b, H_b, W_b)], in ONE launch"""
    require_gpu(rows)
    if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous() or rows.shape[1] != C * pt * p * p:
        raise HipError(f"unpatchify_clips: expected contiguous fp32 rows [*, {C * pt * p * p}], got {rows.dtype} {tuple(rows.shape)}")
    clips = [torch.empty(C, int(T), int(H), int(W), device=rows.device, dtype=torch.float32) for T, H, W in sizes] if out is None else out
    check(lib().vt_unpatchify_clips(ptr(rows), rows.shape[0], _clip_table(clips, C), len(clips), C, pt, p, stream()), "vt_unpatchify_clips")
    return clips


def _packed_tables(cu_seqlens, lead):
    cu, n, M = cu_seqlens_host(cu_seqlens)
    ld = cu_seqlens_list([0] + list(lead))[1:]           # the one conversion: floats are refused, not truncated
    if len(ld) != n:
        raise HipError(f"packed rows: {len(ld)} lead counts for {n} sequences")
    return cu, (c_i32 * max(n, 1))(*ld), n, M, ld


def _segment_rows(cu, ld, n, which):
    return sum(ld) if which == PACKED_LEAD else cu[n] - sum(ld)


def _f32_rows(t, what, rows=None):
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or (rows is not None and t.shape[0] != rows):
        raise HipError(f"{what}: expected a contiguous fp32 matrix" + (f" of {rows} rows" if rows is not None else "") + f", got {t.dtype} {tuple(t.shape)}")
    return t.shape[1]


def packed_scatter(src, cu_seqlens, lead, which, vec=None, out=None):
    """dst fp32 [M, D]: sequence b = rows cu[b] .. cu[b+1]-1 = [lead[b] lead rows | tail rows]; the `which` segments take the rows of the
    compact src in order, the other segments vec [D] (zeros when None)"""
    require_gpu(src, vec, out)
    cu, ld, n, M, lst = _packed_tables(cu_seqlens, lead)
    D = _f32_rows(src, "packed_scatter: src", _segment_rows(cu, lst, n, which) if which in (PACKED_LEAD, PACKED_TAIL) else None)
    if vec is not None and (vec.dtype != torch.float32 or vec.numel() != D or not vec.is_contiguous()):
        raise HipError(f"packed_scatter: vec must be contiguous fp32 with {D} elements, got {vec.dtype} {tuple(vec.shape)}")
    out = torch.empty(M, D, device=src.device, dtype=torch.float32) if out is None else out
    if _f32_rows(out, "packed_scatter: out", M) != D:
        raise HipError(f"packed_scatter: out has {out.shape[1]} columns, src has {D}")
    check(lib().vt_packed_scatter(ptr(src), ptr(vec), cu, ld, n, M, D, which, ptr(out), stream()), "vt_packed_scatter")
    return out


def packed_gather(packed, cu_seqlens, lead, which, out=None):
    """the `which` segments' rows of a packed fp32 [M, D], in order -> compact fp32 [sum_b |segment_b|, D]"""
    require_gpu(packed, out)
    cu, ld, n, M, lst = _packed_tables(cu_seqlens, lead)
    D = _f32_rows(packed, "packed_gather: packed", M)
    R = max(_segment_rows(cu, lst, n, which), 0) if which in (PACKED_LEAD, PACKED_TAIL) else 0
    out = torch.empty(R, D, device=packed.device, dtype=torch.float32) if out is None else out
    if _f32_rows(out, "packed_gather: out", R) != D:
        raise HipError(f"packed_gather: out has {out.shape[1]} columns, packed has {D}")
    check(lib().vt_packed_gather(ptr(packed), cu, ld, n, M, D, which, ptr(out), stream()), "vt_packed_gather")
    return out


def packed_segment_colsum(packed, cu_seqlens, lead, which):
    """out fp32 [D] = the sum of every row of the `which` segments of a packed fp32 [M, D], in a fixed order, read in place"""
    require_gpu(packed)
    cu, ld, n, M, _ = _packed_tables(cu_seqlens, lead)
    D = _f32_rows(packed, "packed_segment_colsum: packed", M)
    out = torch.empty(D, device=packed.device, dtype=torch.float32)
    ws = _ws(lib().vt_packed_segment_colsum_workspace_bytes(D), packed.device)
    check(lib().vt_packed_segment_colsum(ptr(packed), cu, ld, n, M, D, which, ptr(out), ptr(ws), stream()), "vt_packed_segment_colsum")
    return out


def _gqa_tables_ok(cos, sin, M):
    return (tuple(cos.shape) == (M, 32) == tuple(sin.shape) and cos.dtype == torch.float32 == sin.dtype and cos.is_contiguous()
            and sin.is_contiguous())


def qknorm_rope_gqa_fwd(qkv, Hq, Hkv, q_w, q_b, k_w, k_b, eps, cos, sin, out=None):
    """qkv: a bf16 view [M, 64 (Hq + 2 Hkv)] (columns q | k | v) -> the same layout with q and k LayerNorm_64'd and rotated by table row m
    (cos / sin fp32 [M, 32]), v copied"""
    require_gpu(qkv, q_w, q_b, k_w, k_b, cos, sin, out)
    M, W = qkv.shape
    assert W == 64 * (Hq + 2 * Hkv) and _gqa_tables_ok(cos, sin, M)
    out = torch.empty(M, W, device=qkv.device, dtype=torch.bfloat16) if out is None else out
    assert tuple(out.shape) == (M, W)
    check(lib().vt_qknorm_rope_gqa_fwd(ptr(qkv), _rows_view(qkv, "qkv"), M, Hq, Hkv, ptr(q_w), ptr(q_b), ptr(k_w), ptr(k_b), eps, ptr(cos), ptr(sin),
                                       ptr(out), _rows_view(out, "out"), stream()), "vt_qknorm_rope_gqa_fwd")
    return out


def qknorm_rope_gqa_bwd(qkv, dout, Hq, Hkv, q_w, k_w, eps, cos, sin, dqkv=None):
    """dout: gradient of qknorm_rope_gqa_fwd's output -> (dqkv, [dq_w, dq_b, dk_w, dk_b] fp32 [64] each)"""
    require_gpu(qkv, dout, q_w, k_w, cos, sin, dqkv)
    M, W = qkv.shape
    assert W == 64 * (Hq + 2 * Hkv) and tuple(dout.shape) == (M, W) and _gqa_tables_ok(cos, sin, M)
    dqkv = torch.empty(M, W, device=qkv.device, dtype=torch.bfloat16) if dqkv is None else dqkv
    assert tuple(dqkv.shape) == (M, W)
    grads = [torch.empty(64, device=qkv.device, dtype=torch.float32) for _ in range(4)]
    ws = _ws(lib().vt_qknorm_rope_gqa_bwd_workspace_bytes(), qkv.device)
    check(lib().vt_qknorm_rope_gqa_bwd(ptr(qkv), _rows_view(qkv, "qkv"), ptr(dout), _rows_view(dout, "dout"), M, Hq, Hkv, ptr(q_w), ptr(k_w), eps,
                                       ptr(cos), ptr(sin), ptr(dqkv), _rows_view(dqkv, "dqkv"), ptr(grads[0]), ptr(grads[1]), ptr(grads[2]),
                                       ptr(grads[3]), ptr(ws), stream()), "vt_qknorm_rope_gqa_bwd")
    return dqkv, grads


def head_rmsnorm_fwd(x, w, eps, H):
    """RMSNorm over each 64-element head vector: x a bf16 view [M, 64 H] (rows of a wider buffer allowed), w fp32 [64] -> y bf16 [M, 64 H]"""
    require_gpu(x, w)
    M = x.shape[0]
    assert x.shape[1] == 64 * H and w.dtype == torch.float32 and w.numel() == 64 and w.is_contiguous()
    y = torch.empty(M, 64 * H, device=x.device, dtype=torch.bfloat16)
    check(lib().vt_head_rmsnorm_fwd(ptr(x), _rows_view(x, "x"), ptr(w), eps, M, H, ptr(y), y.stride(0), stream()), "vt_head_rmsnorm_fwd")
    return y


def head_rmsnorm_bwd(dy, x, w, eps, H, dx=None):
    """-> (dx, dw fp32 [64]); dx defaults to a new dense matrix and may be `dy` itself (in place) or a view of a wider buffer"""
    require_gpu(dy, x, w, dx)
    M = x.shape[0]
    assert x.shape[1] == 64 * H and tuple(dy.shape) == tuple(x.shape) and w.dtype == torch.float32 and w.numel() == 64 and w.is_contiguous()
    dx = torch.empty(M, 64 * H, device=x.device, dtype=torch.bfloat16) if dx is None else dx
    assert tuple(dx.shape) == tuple(x.shape)
    dw = torch.empty(64, device=x.device, dtype=torch.float32)
    ws = _ws(lib().vt_head_rmsnorm_bwd_workspace_bytes(), x.device)
    check(lib().vt_head_rmsnorm_bwd(ptr(dy), _rows_view(dy, "dy"), ptr(x), _rows_view(x, "x"), ptr(w), eps, M, H, ptr(dx), _rows_view(dx, "dx"),
                                    ptr(dw), ptr(ws), stream()), "vt_head_rmsnorm_bwd")
    return dx, dw


def sigmoid_gate_cols_fwd(o, gate):
    """og = o * sigmoid(gate): o bf16 [M, D] dense, gate a bf16 view [M, D] of any wider buffer"""
    require_gpu(o, gate)
    M, D = o.shape
    assert o.is_contiguous() and o.dtype == torch.bfloat16 and tuple(gate.shape) == (M, D)
    og = torch.empty_like(o)
    check(lib().vt_sigmoid_gate_cols_fwd(ptr(o), ptr(gate), _rows_view(gate, "gate"), M, D, ptr(og), stream()), "vt_sigmoid_gate_cols_fwd")
    return og


def sigmoid_gate_cols_bwd(dog, o, gate, dgate):
    """returns d_o; writes the gate's gradient into the view `dgate` [M, D] (other columns of its buffer are left alone)"""
    require_gpu(dog, o, gate, dgate)
    M, D = o.shape
    assert dog.is_contiguous() and o.is_contiguous() and dog.shape == o.shape and tuple(gate.shape) == (M, D) == tuple(dgate.shape)
    d_o = torch.empty_like(o)
    check(lib().vt_sigmoid_gate_cols_bwd(ptr(dog), ptr(o), ptr(gate), _rows_view(gate, "gate"), M, D, ptr(d_o), ptr(dgate), _rows_view(dgate, "dgate"),
                                         stream()), "vt_sigmoid_gate_cols_bwd")
    return d_o


def _rmsnorm_fwd(family, x, w, eps, out_dtype=torch.bfloat16):
    """the forward of one RMSNorm entry-point family (`vt_rmsnorm`, `vt_rmsnorm_any`, `vt_rmsnorm_any_f32`) -> (y out_dtype, rstd fp32 [rows])"""
    rows, dim = x.shape
    y = torch.empty(rows, dim, device=x.device, dtype=out_dtype)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(getattr(lib(), family + "_fwd")(ptr(x), ptr(w), eps, rows, dim, ptr(y), ptr(rstd), stream()), family + "_fwd")
    return y, rstd


def _rmsnorm_bwd(family, dy, x, w, rstd, dres=None, want_bf16=False):
    """the backward of one family -> (dx, dxb, dw).  The fp32 family's C signature has neither dres nor the bf16 copy dxb"""
    rows, dim = x.shape
    bf16 = not family.endswith("_f32")
    dx = torch.empty_like(x)
    dxb = torch.empty(rows, dim, device=x.device, dtype=torch.bfloat16) if want_bf16 else None
    dw = torch.empty(dim, device=x.device, dtype=torch.float32)
    ws = _ws(getattr(lib(), family + "_bwd_workspace_bytes")(dim), x.device)
    args = (ptr(dy), ptr(x), ptr(w), ptr(rstd)) + ((ptr(dres),) if bf16 else ()) + (rows, dim, ptr(dx)) + ((ptr(dxb),) if bf16 else ())
    check(getattr(lib(), family + "_bwd")(*args, ptr(dw), ptr(ws), stream()), family + "_bwd")
    return dx, dxb, dw


def rmsnorm_any_fwd(x, w, eps):
    """vt_rmsnorm_fwd at the widths of model_design as well (128, 256, 512)"""
    require_gpu(x, w)
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous()
    return _rmsnorm_fwd("vt_rmsnorm_any", x, w, eps)


def rmsnorm_any_bwd(dy, x, w, rstd, dres=None, want_bf16=False):
    require_gpu(dy, x, w, rstd, dres)
    assert dy.is_contiguous() and dy.dtype == torch.bfloat16 and tuple(dy.shape) == tuple(x.shape)
    return _rmsnorm_bwd("vt_rmsnorm_any", dy, x, w, rstd, dres, want_bf16)


def rmsnorm_fwd(x, w, eps):
    require_gpu(x, w)
    return _rmsnorm_fwd("vt_rmsnorm", x, w, eps)


def rmsnorm_bwd(dy, x, w, rstd, dres=None, want_bf16=False):
    require_gpu(dy, x, w, rstd)
    return _rmsnorm_bwd("vt_rmsnorm", dy, x, w, rstd, dres, want_bf16)


def swiglu_fwd(h):
    require_gpu(h)
    M, I2 = h.shape
    a = torch.empty(M, I2 // 2, device=h.device, dtype=torch.bfloat16)
    check(lib().vt_swiglu_fwd(ptr(h), M, I2 // 2, ptr(a), stream()), "vt_swiglu_fwd")
    return a


def swiglu_bwd(da, h):
    require_gpu(da, h)
    M, I2 = h.shape
    dh = torch.empty_like(h)
    check(lib().vt_swiglu_bwd(ptr(da), ptr(h), M, I2 // 2, ptr(dh), stream()), "vt_swiglu_bwd")
    return dh


def decode_attention(q, k_cache, v_cache, n_keys):
    """q bf16 [B, H, 64]; caches bf16 [Bmax, H, Lmax, 64] (contiguous); keys 0..n_keys-1 visible -> o bf16 [B, H, 64]"""
    require_gpu(q, k_cache, v_cache)
    B, H, _ = q.shape
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape[1] == H and k_cache.shape[3] == 64 and k_cache.shape[0] >= B
    o = torch.empty_like(q)
    check(lib().vt_decode_attention(ptr(q), ptr(k_cache), ptr(v_cache), B, H, k_cache.shape[2], n_keys, ptr(o), stream()), "vt_decode_attention")
    return o


def decode_attention_step(qkv, k_cache, v_cache, pos_dev):
    """qkv bf16 [B, 3 * H * 64] = [q | k | v] of the new token; pos_dev int32 device tensor [1] = its position.  Stores k, v into the
    caches at that position and returns o bf16 [B, H * 64] over keys 0..pos.  No host synchronisation (graph-capturable)."""
    require_gpu(qkv, k_cache, v_cache, pos_dev)
    B = qkv.shape[0]
    H = k_cache.shape[1]
    assert qkv.is_contiguous() and qkv.shape[1] == 3 * H * 64 and k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape[0] >= B
    assert pos_dev.dtype == torch.int32 and pos_dev.numel() == 1
    o = torch.empty(B, H * 64, device=qkv.device, dtype=torch.bfloat16)
    check(lib().vt_decode_attention_step(ptr(qkv), ptr(k_cache), ptr(v_cache), B, H, k_cache.shape[2], ptr(pos_dev), ptr(o), stream()), "vt_decode_attention_step")
    return o


def decode_norm_linear(x, norm_w, eps, W, mode=0, out=None):
    """Linear(RMSNorm(x)) for M <= 64 rows in one launch.  x fp32 [M, K]; W bf16 [N, K]; mode 0 -> bf16 [M, N]; mode 1 (W = [w3 ; w1] in
    8 + 8-row slabs) -> SwiGLU output bf16 [M, N / 2]; mode 2 -> fp32 [M, N] of the bf16-rounded values.  out: optional destination of
    that shape and type, rows stride(0) apart (a view of a wider buffer; unit column stride)."""
    require_gpu(x, norm_w, W)
    M, K = x.shape
    N = W.shape[0]
    if norm_w is None:
        assert x.dtype == torch.bfloat16           # already normalised operand: only the Linear and its epilogue are fused
    else:
        assert x.dtype == torch.float32 and norm_w.dtype == torch.float32
    assert W.dtype == torch.bfloat16 and x.is_contiguous() and W.is_contiguous() and W.shape[1] == K
    cols = N // 2 if mode == 1 else N
    dtype = torch.float32 if mode == 2 else torch.bfloat16
    if out is None:
        out = torch.empty(M, cols, device=x.device, dtype=dtype)
    require_gpu(out)
    assert out.dtype == dtype and tuple(out.shape) == (M, cols) and out.stride(1) == 1
    ldo = out.stride(0) if M > 1 else max(out.stride(0), cols)
    check(lib().vt_decode_norm_linear(ptr(x), ptr(norm_w), eps, ptr(W), M, N, K, mode, ptr(out), ldo, stream()), "vt_decode_norm_linear")
    return out


def vq_forward(z_in, codebook, mode, l2_normalized=True, inv_tau=1.0, beta=0.25, codebook_w=1.0, seed=0, ldp=0):
    """z_in fp32 [N, ldz] (first d columns used). Returns dict of saved tensors."""
    N = z_in.shape[0]
    K, d = codebook.shape
    dev = z_in.device
    o = {
        "E": torch.empty(K, d, device=dev), "wnorm": torch.empty(K, device=dev), "zn": torch.empty(N, d, device=dev),
        "znorm": torch.empty(N, device=dev), "idx": torch.empty(N, device=dev, dtype=torch.int64),
        "rz": torch.empty(N, d, device=dev), "losses": torch.empty(4, device=dev),
        "rz_pad": torch.zeros(N, ldp, device=dev, dtype=torch.bfloat16) if ldp else None,
    }
    ws = _ws(lib().vt_vq_workspace_bytes(N, K, d), dev)
    check(lib().vt_vq_forward(ptr(z_in), z_in.stride(0), ptr(codebook), N, K, d, mode, int(l2_normalized), inv_tau, beta, codebook_w,
                              seed, ptr(o["E"]), ptr(o["wnorm"]), ptr(o["zn"]), ptr(o["znorm"]), ptr(o["idx"]), ptr(o["rz"]),
                              ptr(o["rz_pad"]), ldp, ptr(o["losses"]), ptr(ws), stream()), "vt_vq_forward")
    return o


def vq_backward(g_rz, gscal, saved, beta=0.25, codebook_w=1.0, l2_normalized=True, ldp=0, need_dW=True):
    zn, E = saved["zn"], saved["E"]
    N, d = zn.shape
    K = E.shape[0]
    dev = zn.device
    dz = torch.empty(N, d, device=dev)
    dz_pad = torch.zeros(N, ldp, device=dev, dtype=torch.bfloat16) if ldp else None
    dW = torch.empty(K, d, device=dev) if need_dW else None          # frozen codebook: the dense K x d gradient is skipped
    ws = _ws(lib().vt_vq_workspace_bytes(N, K, d) if need_dW else 64, dev)
    check(lib().vt_vq_backward(ptr(g_rz), g_rz.stride(0) if g_rz is not None else 0, ptr(gscal), beta, codebook_w, ptr(zn),
                               ptr(saved["znorm"]), ptr(E), ptr(saved["wnorm"]), ptr(saved["idx"]), N, K, d, int(l2_normalized),
                               ptr(dz), ptr(dz_pad), ldp, ptr(dW), ptr(ws), stream()), "vt_vq_backward")
    return dz, dz_pad, dW


def _levels(levels):
    return (c_i32 * len(levels))(*[int(v) for v in levels])


def _fsq_dtype(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"FSQ kernels take fp32 or bf16, got {t.dtype}")
    return int(t.dtype == torch.bfloat16)


def fsq_codebook_size(levels):
    """host-only (no GPU needed): prod(levels), with the library's own validation of the level list"""
    size = c_i64(0)
    check(lib().vt_fsq_codebook_size(_levels(levels), len(levels), ctypes.byref(size)), "vt_fsq_codebook_size")
    return size.value


def fsq_forward(z, levels, want_indices=True):
    """z [..., d] fp32/bf16 contiguous -> (codes like z, indices int32 [...])"""
    require_gpu(z)
    d = len(levels)
    assert z.is_contiguous() and z.shape[-1] == d
    N = z.numel() // d
    codes = torch.empty_like(z)
    idx = torch.empty(z.shape[:-1], device=z.device, dtype=torch.int32) if want_indices else None
    check(lib().vt_fsq_forward(ptr(z), _fsq_dtype(z), N, d, _levels(levels), ptr(codes), ptr(idx), stream()), "vt_fsq_forward")
    return codes, idx


def fsq_backward(z, dcodes, levels):
    require_gpu(z, dcodes)
    d = len(levels)
    assert z.is_contiguous() and dcodes.is_contiguous() and z.shape == dcodes.shape and z.dtype == dcodes.dtype
    dz = torch.empty_like(z)
    check(lib().vt_fsq_backward(ptr(z), ptr(dcodes), _fsq_dtype(z), z.numel() // d, d, _levels(levels), ptr(dz), stream()), "vt_fsq_backward")
    return dz


def fsq_indices_to_codes(indices, levels, dtype=torch.float32):
    require_gpu(indices)
    d = len(levels)
    idx = indices.to(torch.int32).contiguous()
    codes = torch.empty(*idx.shape, d, device=idx.device, dtype=dtype)
    check(lib().vt_fsq_indices_to_codes(ptr(idx), idx.numel(), d, _levels(levels), ptr(codes), _fsq_dtype(codes), stream()), "vt_fsq_indices_to_codes")
    return codes


# ---- token gate of autoencoder_stat (csrc/vt_stat.hip) ----
STAT_SAMPLE, STAT_THRESHOLD, STAT_ONES, STAT_FORCED = 0, 1, 2, 3


def stat_gate_forward(g, w2, b2, z, levels, mode, seed=0, mask_in=None):
    """g bf16 [M, W] (gelu of the head's fc1), w2 fp32 [W], b2 fp32 [1], z fp32 [M, d] or None -> (probs, mask fp32 [M],
    codes fp32 [M, d], indices int32 [M]); codes / indices are None when z is None"""
    require_gpu(g, w2, b2, z, mask_in)
    M, W = g.shape
    assert g.dtype == torch.bfloat16 and g.stride(1) == 1 and w2.is_contiguous() and w2.dtype == torch.float32
    dev = g.device
    probs, mask = torch.empty(M, device=dev), torch.empty(M, device=dev)
    codes = idx = None
    d = len(levels) if levels is not None else 0
    if z is not None:
        assert z.is_contiguous() and z.dtype == torch.float32 and tuple(z.shape) == (M, d)
        codes = torch.empty_like(z)
        idx = torch.empty(M, device=dev, dtype=torch.int32)
    check(lib().vt_stat_gate_forward(ptr(g), g.stride(0), ptr(w2), ptr(b2), ptr(z), M, W, d, _levels(levels or []), int(mode),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(mask_in), ptr(probs), ptr(mask), ptr(codes), ptr(idx), stream()),
          "vt_stat_gate_forward")
    return probs, mask, codes, idx


def stat_gate_backward(dcodes, dprobs, dmask, z, mask, probs, u, g, w2, levels, ste):
    """-> (dU bf16 [M, W], dz fp32 [M, d] or None, dw2 fp32 [W], db2 fp32 [1]); dprobs / dmask may be None"""
    require_gpu(dcodes, dprobs, dmask, z, mask, probs, u, g, w2)
    M, W = g.shape
    assert u.shape == g.shape and u.is_contiguous() and g.is_contiguous() and u.dtype == g.dtype == torch.bfloat16
    dev = g.device
    dU = torch.empty(M, W, device=dev, dtype=torch.bfloat16)
    dz = torch.empty_like(z) if z is not None else None
    dw2, db2 = torch.empty(W, device=dev), torch.empty(1, device=dev)
    d = len(levels) if levels is not None else 0
    ws = _ws(lib().vt_stat_gate_workspace_bytes(W), dev)
    check(lib().vt_stat_gate_backward(ptr(dcodes), ptr(dprobs), ptr(dmask), ptr(z), ptr(mask), ptr(probs), ptr(u), ptr(g), W, ptr(w2), M, W, d,
                                      _levels(levels or []), int(bool(ste)), ptr(dU), ptr(dz), ptr(dw2), ptr(db2), ptr(ws), stream()),
          "vt_stat_gate_backward")
    return dU, dz, dw2, db2


# ---- KL bottleneck 'skl' (csrc/vt_kl.hip) ----
KL_WORKSPACE_BYTES = 4096    # VT_KL_WORKSPACE_BYTES


def kl_forward(z, seed=0, seed_counter=None, ldp=0):
    """z fp32 [B, N, 2d] (mean, logvar interleaved) -> (mean, sample, noise fp32 [B, N, d], loss_kl fp32 [1], sample_pad bf16 [B*N, ldp]
    or None when ldp == 0)"""
    require_gpu(z, seed_counter)
    assert z.dim() == 3 and z.shape[-1] % 2 == 0 and z.dtype == torch.float32
    z = z.contiguous()
    B, N, d = z.shape[0], z.shape[1], z.shape[2] // 2
    dev = z.device
    mean, sample, noise = (torch.empty(B, N, d, device=dev) for _ in range(3))
    loss = torch.empty(1, device=dev)
    pad = torch.empty(B * N, ldp, device=dev, dtype=torch.bfloat16) if ldp else None
    ws = _ws(KL_WORKSPACE_BYTES, dev)
    check(lib().vt_kl_forward(ptr(z), 2 * d, B * N, d, B, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seed_counter), ptr(mean), ptr(sample), ptr(pad),
                              ldp, ptr(noise), ptr(loss), ptr(ws), stream()), "vt_kl_forward")
    return mean, sample, noise, loss, pad


def kl_backward(z, noise, g_sample=None, g_mean=None, gkl=None, ldp=0):
    """-> dz fp32 [B, N, 2d] (and its bf16 copy [B*N, ldp] when ldp > 0); any gradient may be None (zero)"""
    require_gpu(z, noise, g_sample, g_mean, gkl)
    B, N, d = z.shape[0], z.shape[1], z.shape[2] // 2
    z, noise = z.contiguous(), noise.contiguous()
    g_sample = g_sample.contiguous().float() if g_sample is not None else None
    g_mean = g_mean.contiguous().float() if g_mean is not None else None
    gkl = gkl.contiguous().float().reshape(-1) if gkl is not None else None
    dz = torch.empty_like(z)
    pad = torch.empty(B * N, ldp, device=z.device, dtype=torch.bfloat16) if ldp else None
    check(lib().vt_kl_backward(ptr(g_sample), d, ptr(g_mean), ptr(gkl), ptr(z), 2 * d, ptr(noise), B * N, d, B, ptr(dz), ptr(pad), ldp, stream()),
          "vt_kl_backward")
    return (dz, pad) if ldp else dz


# ---- glue of the TiTok-style block (csrc/vt_gated.hip) ----
def qknorm_rope_fwd(qkvg, L, H, q_w, q_b, k_w, k_b, eps, cos, sin):
    """qkvg bf16 [M, 4 * 64 H] -> packed bf16 [M, 3 * 64 H] (q, k normalised per head and rotated; v copied)"""
    require_gpu(qkvg, q_w, q_b, k_w, k_b, cos, sin)
    M = qkvg.shape[0]
    assert qkvg.dtype == torch.bfloat16 and qkvg.is_contiguous() and qkvg.shape[1] == 4 * 64 * H and cos.shape == (L, 32) == sin.shape
    out = torch.empty(M, 3 * 64 * H, device=qkvg.device, dtype=torch.bfloat16)
    check(lib().vt_qknorm_rope_fwd(ptr(qkvg), M, L, H, ptr(q_w), ptr(q_b), ptr(k_w), ptr(k_b), eps, ptr(cos), ptr(sin), ptr(out), stream()),
          "vt_qknorm_rope_fwd")
    return out


def rope_rotate(qkv, L, H, cos, sin, conjugate=False, rows=None):
    """vt_rope_rotate (csrc/vt_rope.hip): rotates the q and k columns of the packed bf16 [M, 3 * 64 H] operand IN PLACE (the first `rows`
    rows, default all) by the [L, 32] tables, or by their conjugate; returns qkv"""
    require_gpu(qkv, cos, sin)
    assert qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[1] >= 2 * 64 * H
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and cos.shape == (L, 32) == sin.shape
    M = qkv.shape[0] if rows is None else rows
    assert 0 < M <= qkv.shape[0]
    check(lib().vt_rope_rotate(ptr(qkv), qkv.stride(0), M, L, H, ptr(cos), ptr(sin), int(bool(conjugate)), stream()), "vt_rope_rotate")
    return qkv


def qknorm_rope_bwd(qkvg, dqkv, L, H, q_w, k_w, eps, cos, sin, dqkvg):
    """writes columns 0..3D of dqkvg in place; returns (dq_w, dq_b, dk_w, dk_b)"""
    require_gpu(qkvg, dqkv, dqkvg)
    M = qkvg.shape[0]
    assert dqkv.is_contiguous() and dqkvg.is_contiguous() and dqkvg.shape == qkvg.shape and dqkv.shape == (M, 3 * 64 * H)
    grads = torch.empty(4, 64, device=qkvg.device)
    ws = _ws(lib().vt_qknorm_rope_bwd_workspace_bytes(), qkvg.device)
    check(lib().vt_qknorm_rope_bwd(ptr(qkvg), ptr(dqkv), M, L, H, ptr(q_w), ptr(k_w), eps, ptr(cos), ptr(sin), ptr(dqkvg), ptr(grads[0]),
                                   ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(ws), stream()), "vt_qknorm_rope_bwd")
    return grads[0], grads[1], grads[2], grads[3]


def sigmoid_gate_fwd(o, qkvg):
    require_gpu(o, qkvg)
    M, D = o.shape
    assert o.is_contiguous() and qkvg.shape == (M, 4 * D)
    og = torch.empty_like(o)
    check(lib().vt_sigmoid_gate_fwd(ptr(o), ptr(qkvg), M, D, ptr(og), stream()), "vt_sigmoid_gate_fwd")
    return og


def sigmoid_gate_bwd(dog, o, qkvg, dqkvg):
    """returns d_o; writes columns 3D..4D of dqkvg in place"""
    require_gpu(dog, o, qkvg, dqkvg)
    M, D = o.shape
    assert dog.is_contiguous() and dog.shape == o.shape and dqkvg.shape == qkvg.shape
    d_o = torch.empty_like(o)
    check(lib().vt_sigmoid_gate_bwd(ptr(dog), ptr(o), ptr(qkvg), M, D, ptr(d_o), ptr(dqkvg), stream()), "vt_sigmoid_gate_bwd")
    return d_o


def geglu_fwd(h, lda=None):
    require_gpu(h)
    M, I2 = h.shape
    I = I2 // 2
    lda = I if lda is None else lda
    a = torch.empty(M, lda, device=h.device, dtype=torch.bfloat16) if lda == I else torch.zeros(M, lda, device=h.device, dtype=torch.bfloat16)
    check(lib().vt_geglu_fwd(ptr(h), M, I, ptr(a), lda, stream()), "vt_geglu_fwd")
    return a


def geglu_bwd(da, h):
    require_gpu(da, h)
    M, I2 = h.shape
    assert da.shape[0] == M and da.is_contiguous()
    dh = torch.empty_like(h)
    check(lib().vt_geglu_bwd(ptr(da), da.shape[1], ptr(h), M, I2 // 2, ptr(dh), stream()), "vt_geglu_bwd")
    return dh


# ---- row passes of model_design's self-attention block and stack (csrc/vt_design.hip; its final norm csrc/vt_rmsnorm.hip) ----
def _tables_ok(cos, sin, L):
    return cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and cos.shape == (L, 32) == sin.shape


def qkrms_rope_fwd(qkvg, L, H, q_w, k_w, eps, cos, sin, rows=None, out=None):
    """qkvg a bf16 view [>= M, >= 3 * 64 H] (rows of the wider [M, 4D] projection) -> packed bf16 [M, 3 * 64 H]: q, k RMS-normalised per head
    and rotated, v copied; the first `rows` rows (default all)"""
    require_gpu(qkvg, q_w, k_w, cos, sin, out)
    M = qkvg.shape[0] if rows is None else rows
    assert qkvg.dtype == torch.bfloat16 and qkvg.dim() == 2 and qkvg.shape[1] >= 3 * 64 * H and 0 < M <= qkvg.shape[0] and _tables_ok(cos, sin, L)
    assert q_w.dtype == torch.float32 and k_w.dtype == torch.float32 and q_w.numel() == 64 == k_w.numel() and q_w.is_contiguous() and k_w.is_contiguous()
    out = torch.empty(M, 3 * 64 * H, device=qkvg.device, dtype=torch.bfloat16) if out is None else out
    assert out.dtype == torch.bfloat16 and out.shape[0] >= M and out.shape[1] >= 3 * 64 * H
    check(lib().vt_qkrms_rope_fwd(ptr(qkvg), _rows_view(qkvg, "qkvg"), M, L, H, ptr(q_w), ptr(k_w), eps, ptr(cos), ptr(sin), ptr(out),
                                  _rows_view(out, "out"), stream()), "vt_qkrms_rope_fwd")
    return out


def qkrms_rope_bwd(qkvg, dqkv, L, H, q_w, k_w, eps, cos, sin, dqkvg, want_dw=True):
    """writes columns 0..3D of the bf16 view dqkvg in place; returns (dq_w, dk_w) fp32 [64] each, or (None, None)"""
    require_gpu(qkvg, dqkv, dqkvg, q_w, k_w, cos, sin)
    M = dqkv.shape[0]
    assert dqkv.dtype == torch.bfloat16 and dqkv.is_contiguous() and dqkv.shape == (M, 3 * 64 * H) and qkvg.shape[0] >= M and dqkvg.shape[0] >= M
    assert qkvg.dtype == torch.bfloat16 and dqkvg.dtype == torch.bfloat16 and qkvg.shape[1] >= 3 * 64 * H and dqkvg.shape[1] >= 3 * 64 * H and _tables_ok(cos, sin, L)
    dw = torch.empty(2, 64, device=qkvg.device) if want_dw else None
    ws = _ws(lib().vt_qkrms_rope_bwd_workspace_bytes(), qkvg.device)
    check(lib().vt_qkrms_rope_bwd(ptr(qkvg), _rows_view(qkvg, "qkvg"), ptr(dqkv), M, L, H, ptr(q_w), ptr(k_w), eps, ptr(cos), ptr(sin), ptr(dqkvg),
                                  _rows_view(dqkvg, "dqkvg"), ptr(dw[0]) if want_dw else None, ptr(dw[1]) if want_dw else None, ptr(ws), stream()),
          "vt_qkrms_rope_bwd")
    return (dw[0], dw[1]) if want_dw else (None, None)


def residual_scale_fwd(x, y, scale):
    """x + float(bf16(scale * y)): x, y fp32 [rows, dim] (y holding bf16 values), scale a 0-dim fp32 DEVICE tensor"""
    require_gpu(x, y, scale)
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape and x.dim() == 2
    assert scale.dtype == torch.float32 and scale.numel() == 1
    out = torch.empty_like(x)
    check(lib().vt_residual_scale_fwd(ptr(x), ptr(y), ptr(scale), x.shape[0], x.shape[1], ptr(out), stream()), "vt_residual_scale_fwd")
    return out


def residual_scale_bwd(dout, y, scale, want_ds=True):
    """-> (dy fp32 holding bf16 values, dscale 0-dim fp32 or None)"""
    require_gpu(dout, y, scale)
    assert dout.dtype == torch.float32 and dout.is_contiguous() and dout.dim() == 2 and scale.dtype == torch.float32 and scale.numel() == 1
    assert y is None or (y.dtype == torch.float32 and y.is_contiguous() and y.shape == dout.shape)
    dy = torch.empty_like(dout)
    ds = torch.empty((), device=dout.device, dtype=torch.float32) if want_ds else None
    ws = _ws(lib().vt_residual_scale_bwd_workspace_bytes(), dout.device) if want_ds else None
    check(lib().vt_residual_scale_bwd(ptr(dout), ptr(y), ptr(scale), dout.shape[0], dout.shape[1], ptr(dy), ptr(ds), ptr(ws), stream()),
          "vt_residual_scale_bwd")
    return dy, ds


def rmsnorm_any_f32_fwd(x, w, eps):
    """RMSNorm with an fp32, unrounded output (final_norm of model_design's stack): -> (y fp32, rstd fp32 [rows])"""
    require_gpu(x, w)
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous()
    return _rmsnorm_fwd("vt_rmsnorm_any_f32", x, w, eps, out_dtype=torch.float32)


def rmsnorm_any_f32_bwd(dy, x, w, rstd):
    """dy fp32 -> (dx fp32, dw fp32 [dim])"""
    require_gpu(dy, x, w, rstd)
    assert dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == tuple(x.shape)
    dx, _, dw = _rmsnorm_bwd("vt_rmsnorm_any_f32", dy, x, w, rstd)
    return dx, dw


# ---- the 3D ResNet ends of autoencoder_cnnvit (csrc/vt_conv3d.hip, vt_groupnorm.hip): activations bf16 channels-last [B, T, H, W, C] ----------
def conv3d_out_dims(T, H, W, stride):
    return tuple((n - 1) // s + 1 for n, s in zip((T, H, W), stride))


def conv3d_pack_weight(w, cout_abi, cin_abi, for_dgrad=False):
    """fp32 [Cout, Cin, 3, 3, 3] -> the bf16 operand image of vt_conv3d_fwd (or of vt_conv3d_dgrad), channel counts padded to the ABI's"""
    require_gpu(w)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape[2:] == (3, 3, 3)
    n, k = (cin_abi, cout_abi) if for_dgrad else (cout_abi, cin_abi)
    packed = torch.empty(lib().vt_conv3d_packed_elems(n, k), device=w.device, dtype=torch.bfloat16)
    check(lib().vt_conv3d_pack_weight(ptr(w), w.shape[0], w.shape[1], cout_abi, cin_abi, int(for_dgrad), ptr(packed), stream()), "vt_conv3d_pack_weight")
    return packed


def _cl_dims(x):
    assert x.dtype == torch.bfloat16 and x.dim() == 5 and x.is_contiguous()
    return x.shape


def conv3d_fwd(x, w_packed, bias, cout, stride=(1, 1, 1), residual=None, out=None):
    """x bf16 [B, T, H, W, Cin] -> bf16 [B, T', H', W', cout]; bias fp32 [cout]; residual bf16 like the output"""
    B, T, H, W, Cin = _cl_dims(x)
    To, Ho, Wo = conv3d_out_dims(T, H, W, stride)
    out = torch.empty(B, To, Ho, Wo, cout, device=x.device, dtype=torch.bfloat16) if out is None else out
    assert bias.dtype == torch.float32 and bias.numel() == cout and out.numel() >= B * To * Ho * Wo * cout
    assert residual is None or (residual.dtype == torch.bfloat16 and residual.numel() >= B * To * Ho * Wo * cout)
    check(lib().vt_conv3d_fwd(ptr(x), ptr(w_packed), ptr(bias), ptr(residual), B, T, H, W, Cin, cout, *stride, ptr(out), stream()), "vt_conv3d_fwd")
    return out


def conv3d_dgrad(dy, w_packed_dgrad, in_dims, cin, stride=(1, 1, 1), dx=None):
    """dy bf16 [B, T', H', W', Cout] -> dx bf16 [B, T, H, W, cin]; in_dims = (T, H, W) of the convolution's input"""
    B, To, Ho, Wo, Cout = _cl_dims(dy)
    T, H, W = in_dims
    assert (To, Ho, Wo) == conv3d_out_dims(T, H, W, stride)
    dx = torch.empty(B, T, H, W, cin, device=dy.device, dtype=torch.bfloat16) if dx is None else dx
    assert dx.numel() >= B * T * H * W * cin
    check(lib().vt_conv3d_dgrad(ptr(dy), ptr(w_packed_dgrad), B, T, H, W, cin, Cout, *stride, ptr(dx), stream()), "vt_conv3d_dgrad")
    return dx


def conv3d_wgrad(x, dy, stride=(1, 1, 1), cout_lim=None, cin_lim=None, dw=None):
    """dW fp32 [cout_lim, cin_lim, 3, 3, 3] from x bf16 [B, T, H, W, Cin] and dy bf16 [B, T', H', W', Cout]"""
    B, T, H, W, Cin = _cl_dims(x)
    Cout = _cl_dims(dy)[-1]
    assert tuple(dy.shape[:4]) == (B,) + conv3d_out_dims(T, H, W, stride)
    cout_lim, cin_lim = cout_lim or Cout, cin_lim or Cin
    dw = torch.empty(cout_lim, cin_lim, 3, 3, 3, device=x.device, dtype=torch.float32) if dw is None else dw
    ws = _ws(lib().vt_conv3d_wgrad_workspace_bytes(B, T, H, W, Cin, Cout, *stride, cout_lim, cin_lim), x.device)
    check(lib().vt_conv3d_wgrad(ptr(x), ptr(dy), B, T, H, W, Cin, Cout, *stride, cout_lim, cin_lim, ptr(dw), ptr(ws), stream()), "vt_conv3d_wgrad")
    return dw


def groupnorm_fwd(x, gamma, beta, eps, G, swish, y=None):
    """x bf16 [B, ..., C] channels-last -> (y bf16 like x, mean fp32 [B, G], rstd fp32 [B, G])"""
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, C = x.shape[0], x.shape[-1]
    P = x.numel() // (B * C)
    y = torch.empty_like(x) if y is None else y
    mean, rstd = torch.empty(B, G, device=x.device), torch.empty(B, G, device=x.device)
    ws = _ws(lib().vt_groupnorm_workspace_bytes(B, P, C, G), x.device)
    check(lib().vt_groupnorm_fwd(ptr(x), ptr(gamma), ptr(beta), eps, B, P, C, G, int(swish), ptr(y), ptr(mean), ptr(rstd), ptr(ws), stream()),
          "vt_groupnorm_fwd")
    return y, mean, rstd


def groupnorm_bwd(dz, x, gamma, beta, mean, rstd, G, swish, dx=None):
    """-> (dx bf16 like x, dgamma fp32 [C], dbeta fp32 [C])"""
    assert x.dtype == torch.bfloat16 == dz.dtype and x.is_contiguous() and dz.is_contiguous()
    B, C = x.shape[0], x.shape[-1]
    P = x.numel() // (B * C)
    dx = torch.empty_like(x) if dx is None else dx
    dg, db = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    ws = _ws(lib().vt_groupnorm_workspace_bytes(B, P, C, G), x.device)
    check(lib().vt_groupnorm_bwd(ptr(dz), ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), B, P, C, G, int(swish), ptr(dx), ptr(dg), ptr(db), ptr(ws),
                                 stream()), "vt_groupnorm_bwd")
    return dx, dg, db


def upsample_nearest_fwd(x, scale, out=None):
    B, T, H, W, C = _cl_dims(x)
    out = torch.empty(B, T * scale[0], H * scale[1], W * scale[2], C, device=x.device, dtype=torch.bfloat16) if out is None else out
    check(lib().vt_upsample_nearest_fwd(ptr(x), B, T, H, W, C, *scale, ptr(out), stream()), "vt_upsample_nearest_fwd")
    return out


def upsample_nearest_bwd(dout, scale, dx=None):
    B, To, Ho, Wo, C = _cl_dims(dout)
    T, H, W = To // scale[0], Ho // scale[1], Wo // scale[2]
    assert (T * scale[0], H * scale[1], W * scale[2]) == (To, Ho, Wo)
    dx = torch.empty(B, T, H, W, C, device=dout.device, dtype=torch.bfloat16) if dx is None else dx
    check(lib().vt_upsample_nearest_bwd(ptr(dout), B, T, H, W, C, *scale, ptr(dx), stream()), "vt_upsample_nearest_bwd")
    return dx


def video_to_channels_last(video, cpad=16, out=None):
    """fp32 [B, C, T, H, W] -> bf16 [B, T, H, W, cpad], channels C.. zero"""
    assert video.dtype == torch.float32 and video.is_contiguous()
    B, C, T, H, W = video.shape
    out = torch.empty(B, T, H, W, cpad, device=video.device, dtype=torch.bfloat16) if out is None else out
    check(lib().vt_video_to_channels_last(ptr(video), B, C, T, H, W, cpad, ptr(out), stream()), "vt_video_to_channels_last")
    return out


def channels_last_to_video(x, C, video=None):
    """bf16 [B, T, H, W, cpad] -> fp32 [B, C, T, H, W] holding the bf16 values of the first C channels"""
    B, T, H, W, cpad = _cl_dims(x)
    video = torch.empty(B, C, T, H, W, device=x.device, dtype=torch.float32) if video is None else video
    check(lib().vt_channels_last_to_video(ptr(x), B, C, T, H, W, cpad, ptr(video), stream()), "vt_channels_last_to_video")
    return video
