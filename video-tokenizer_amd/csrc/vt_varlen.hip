// Row pass of the packed, grouped-query attention layer (Attn of models/model_titok/base/transformer.py:32-62) for gfx950:
//   q, k, v = to_qkv(x).split([64 Hq, 64 Hkv, 64 Hkv]); q, k = LayerNorm_64(q), LayerNorm_64(k); rotary(q), rotary(k)
// on the [M, 64 (Hq + 2 Hkv)] projection of a packed batch of M = sum L_b rows, whose row m takes the rotary factors of table row m: a
// packed batch has no period.  The output keeps the projection's layout (q | k | v), which is what vt_attention_varlen_* reads through
// three column views; the backward writes the projection's gradient in the same layout.  The kernels are those of vt_qknorm_rope_*
// (vt_qknorm.h): with Hq == Hkv and L = M the two passes are the same code on the same vectors.  Rounding points follow autocast(bf16).
#include "vt_common.h"
#include "vt_headvec.h"
#include "vt_qknorm.h"

static int gqa_check(const char* who, int64_t M, int Hq, int Hkv) {
    VT_CHECK_ARG(M > 0 && Hq > 0 && Hkv > 0, "%s: bad shape M=%lld Hq=%d Hkv=%d", who, (long long)M, Hq, Hkv);
    VT_CHECK_ARG(Hq % Hkv == 0, "%s: Hq=%d is not a multiple of Hkv=%d", who, Hq, Hkv);
    return VT_OK;
}
static int gqa_stride_check(const char* who, const char* what, int64_t rs, int Hq, int Hkv) {
    VT_CHECK_ARG(rs >= (int64_t)HD * (Hq + 2 * Hkv) && rs % 8 == 0, "%s: row stride %lld of %s must cover 64 x (%d + 2 x %d) columns and be a multiple of 8",
                 who, (long long)rs, what, Hq, Hkv);
    return VT_OK;
}

extern "C" int vt_qknorm_rope_gqa_fwd(const void* qkv, int64_t in_rs, int64_t M, int32_t Hq, int32_t Hkv, const float* q_w, const float* q_b,
                                      const float* k_w, const float* k_b, float eps, const float* cos_tab, const float* sin_tab, void* qkv_out,
                                      int64_t out_rs, vtStream stream) {
    const char* who = "vt_qknorm_rope_gqa_fwd";
    VT_CHECK_ARG(qkv && qkv_out && q_w && q_b && k_w && k_b && cos_tab && sin_tab, "%s: null pointer", who);
    TRY(gqa_check(who, M, Hq, Hkv));
    TRY(gqa_stride_check(who, "qkv", in_rs, Hq, Hkv));
    TRY(gqa_stride_check(who, "qkv_out", out_rs, Hq, Hkv));
    VT_CHECK_ARG(aligned16(qkv) && aligned16(qkv_out) && aligned16(cos_tab) && aligned16(sin_tab), "%s: buffers must be 16-byte aligned", who);
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel, dim3(qkn_fwd_grid(M, Hq), 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, in_rs, M, M, Hq, Hkv,
                       q_w, q_b, k_w, k_b, eps, cos_tab, sin_tab, (bf16_t*)qkv_out, out_rs);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" size_t vt_qknorm_rope_gqa_bwd_workspace_bytes(void) { return (size_t)QKN_NBLK * 256 * sizeof(float); }

extern "C" int vt_qknorm_rope_gqa_bwd(const void* qkv, int64_t in_rs, const void* dqkv_out, int64_t g_rs, int64_t M, int32_t Hq, int32_t Hkv,
                                      const float* q_w, const float* k_w, float eps, const float* cos_tab, const float* sin_tab, void* dqkv,
                                      int64_t d_rs, float* dq_w, float* dq_b, float* dk_w, float* dk_b, void* workspace, vtStream stream) {
    const char* who = "vt_qknorm_rope_gqa_bwd";
    VT_CHECK_ARG(qkv && dqkv_out && dqkv && q_w && k_w && cos_tab && sin_tab && workspace, "%s: null pointer", who);
    TRY(gqa_check(who, M, Hq, Hkv));
    TRY(gqa_stride_check(who, "qkv", in_rs, Hq, Hkv));
    TRY(gqa_stride_check(who, "dqkv_out", g_rs, Hq, Hkv));
    TRY(gqa_stride_check(who, "dqkv", d_rs, Hq, Hkv));
    VT_CHECK_ARG(aligned16(qkv) && aligned16(dqkv_out) && aligned16(dqkv) && aligned16(cos_tab) && aligned16(sin_tab) && aligned16(workspace),
                 "%s: buffers must be 16-byte aligned", who);
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel, dim3(QKN_NBLK, 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, in_rs, (const bf16_t*)dqkv_out,
                       g_rs, M, M, Hq, Hkv, q_w, k_w, eps, cos_tab, sin_tab, (bf16_t*)dqkv, d_rs, (float*)workspace);
    VT_CHECK_LAUNCH(who);
    return vt_reduce_waves("vt_qknorm_rope_gqa_bwd(reduce)", (const float*)workspace, QKN_NBLK, 4 * HD, 4 * HD, dq_w, dq_b, dk_w, dk_b, stream);
}
