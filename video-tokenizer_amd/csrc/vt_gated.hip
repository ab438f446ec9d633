// Elementwise pieces of the reference's TiTok-style transformer block (models/model_new/base/transformer.py) for gfx950:
//   Attn.forward :45-63   q, k, v, gate = to_qkv(x).chunk(4); q, k = LayerNorm_hd(q), LayerNorm_hd(k); rotary(q), rotary(k);
//                         x = flash_attn(q, k, v); x = x * sigmoid(gate); out_proj(x)
//   ffd / GEGLU  :11-29   LayerNorm -> Linear(D, 2 I) -> gelu(gate) * x -> Linear(I, D)
//   apply_rotary_emb      models/model_new/base/rope.py:18-24 (adjacent pairs as complex numbers times freqs_cis[pos])
// The GEMMs, the LayerNorm over D and the attention itself are the kernels of the LARP path; what is new here is
// HBM-bound glue, each a single pass with 16-byte accesses:
//   qknorm_rope   reads q|k|v of the packed [M, 4D] projection, writes the packed [M, 3D] operand of vt_attention_*
//   sigmoid_gate  o * sigmoid(gate), gate read in place from columns 3D..4D of the projection (vt_sigmoid_gate_cols_*: from any
//                 column block of any projection -- CrossAttention of model_design reads it from columns D..2D of [to_q ; to_gate])
//   geglu         gelu(h[:, I:]) * h[:, :I]
// and their backward passes, which write straight into the [M, 4D] / [M, 2I] gradient of the projection so no torch
// cat/chunk copies are needed.  Rounding points follow autocast(bf16): LayerNorm output, rotary output, sigmoid, gelu and
// every product are rounded to bf16 where the reference materialises a bf16 tensor; statistics and products are fp32.
#include "vt_common.h"
#include "vt_headvec.h"
#include "vt_qknorm.h"

namespace {
// (the q/k LayerNorm + rotary kernels are in vt_qknorm.h, shared with the grouped pass of vt_varlen.hip)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// gate: first gate column of row 0, gate_rs its row stride (the block's gate is qkvg + 3D with stride 4D; vt_sigmoid_gate_cols_* takes any)
__global__ __launch_bounds__(256) void gate_fwd_kernel(const bf16_t* __restrict__ o, const bf16_t* __restrict__ gate, int64_t gate_rs, int64_t M, int D,
                                                        bf16_t* __restrict__ og) {
    const int64_t per_row = D / 8, total = M * per_row;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
        const int64_t row = u / per_row;
        const int col = (int)(u % per_row) * 8;
        const Vec8 a = load8(o + row * D + col), g = load8(gate + row * gate_rs + col);
        Vec8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.v[i] = a.v[i] * round_bf16(sigmoidf_(g.v[i]));
        store8(og + row * D + col, r);
    }
}

__global__ __launch_bounds__(256) void gate_bwd_kernel(const bf16_t* __restrict__ dog, const bf16_t* __restrict__ o, const bf16_t* __restrict__ gate,
                                                        int64_t gate_rs, int64_t M, int D, bf16_t* __restrict__ d_o, bf16_t* __restrict__ dgate,
                                                        int64_t dgate_rs) {
    const int64_t per_row = D / 8, total = M * per_row;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
        const int64_t row = u / per_row;
        const int col = (int)(u % per_row) * 8;
        const Vec8 dy = load8(dog + row * D + col), a = load8(o + row * D + col), g = load8(gate + row * gate_rs + col);
        Vec8 da, dg;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float sg = round_bf16(sigmoidf_(g.v[i]));
            da.v[i] = dy.v[i] * sg;
            dg.v[i] = round_bf16(dy.v[i] * a.v[i]) * ((1.0f - sg) * sg);
        }
        store8(d_o + row * D + col, da);
        store8(dgate + row * dgate_rs + col, dg);
    }
}

__global__ __launch_bounds__(256) void geglu_fwd_kernel(const bf16_t* __restrict__ h, int64_t M, int I, bf16_t* __restrict__ a, int64_t lda) {
    const int64_t per_row = I / 8, total = M * per_row;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
        const int64_t row = u / per_row;
        const int col = (int)(u % per_row) * 8;
        const Vec8 x = load8(h + row * 2 * I + col), g = load8(h + row * 2 * I + I + col);
        Vec8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.v[i] = round_bf16(gelu_erf(g.v[i])) * x.v[i];
        store8(a + row * lda + col, r);
    }
}

__global__ __launch_bounds__(256) void geglu_bwd_kernel(const bf16_t* __restrict__ da, int64_t lda, const bf16_t* __restrict__ h, int64_t M, int I,
                                                         bf16_t* __restrict__ dh) {
    const int64_t per_row = I / 8, total = M * per_row;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
        const int64_t row = u / per_row;
        const int col = (int)(u % per_row) * 8;
        const Vec8 dy = load8(da + row * lda + col), x = load8(h + row * 2 * I + col), g = load8(h + row * 2 * I + I + col);
        Vec8 dx, dg;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dx.v[i] = dy.v[i] * round_bf16(gelu_erf(g.v[i]));
            dg.v[i] = round_bf16(dy.v[i] * x.v[i]) * gelu_erf_grad(g.v[i]);
        }
        store8(dh + row * 2 * I + col, dx);
        store8(dh + row * 2 * I + I + col, dg);
    }
}

int grid_for(int64_t units) {
    const int64_t b = (units + 255) / 256;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}
}  // namespace

extern "C" int vt_qknorm_rope_fwd(const void* qkvg, int64_t M, int32_t L, int32_t H, const float* q_w, const float* q_b, const float* k_w,
                                  const float* k_b, float eps, const float* cos_tab, const float* sin_tab, void* qkv_out, vtStream stream) {
    VT_CHECK_ARG(qkvg && qkv_out && q_w && q_b && k_w && k_b && cos_tab && sin_tab, "vt_qknorm_rope_fwd: null pointer");
    VT_CHECK_ARG(M > 0 && L > 0 && H > 0 && M % L == 0, "vt_qknorm_rope_fwd: need M = B * L rows, H heads of 64");
    VT_CHECK_ARG(aligned16(qkvg) && aligned16(qkv_out) && aligned16(cos_tab) && aligned16(sin_tab), "vt_qknorm_rope_fwd: buffers must be 16-byte aligned");
    const int64_t D = (int64_t)H * HD;
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel, dim3(qkn_fwd_grid(M, H), 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkvg, 4 * D, M, (int64_t)L,
                       H, H, q_w, q_b, k_w, k_b, eps, cos_tab, sin_tab, (bf16_t*)qkv_out, 3 * D);
    VT_CHECK_LAUNCH("vt_qknorm_rope_fwd");
    return VT_OK;
}

extern "C" size_t vt_qknorm_rope_bwd_workspace_bytes(void) { return (size_t)QKN_NBLK * 256 * sizeof(float); }

extern "C" int vt_qknorm_rope_bwd(const void* qkvg, const void* dqkv, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w, float eps,
                                  const float* cos_tab, const float* sin_tab, void* dqkvg, float* dq_w, float* dq_b, float* dk_w, float* dk_b,
                                  void* workspace, vtStream stream) {
    VT_CHECK_ARG(qkvg && dqkv && dqkvg && q_w && k_w && cos_tab && sin_tab && workspace, "vt_qknorm_rope_bwd: null pointer");
    VT_CHECK_ARG(M > 0 && L > 0 && H > 0 && M % L == 0, "vt_qknorm_rope_bwd: need M = B * L rows, H heads of 64");
    VT_CHECK_ARG(aligned16(qkvg) && aligned16(dqkv) && aligned16(dqkvg) && aligned16(cos_tab) && aligned16(sin_tab) && aligned16(workspace),
                 "vt_qknorm_rope_bwd: buffers must be 16-byte aligned");
    const int64_t D = (int64_t)H * HD;
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel, dim3(QKN_NBLK, 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkvg, 4 * D, (const bf16_t*)dqkv, 3 * D, M,
                       (int64_t)L, H, H, q_w, k_w, eps, cos_tab, sin_tab, (bf16_t*)dqkvg, 4 * D, (float*)workspace);
    VT_CHECK_LAUNCH("vt_qknorm_rope_bwd");
    return vt_reduce_waves("vt_qknorm_rope_bwd(reduce)", (const float*)workspace, QKN_NBLK, 4 * HD, 4 * HD, dq_w, dq_b, dk_w, dk_b, stream);
}

// `who`: the entry point's name, so that a refusal or a launch failure is reported under the caller's own name
static int gate_cols_fwd(const char* who, const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* og, vtStream stream) {
    VT_CHECK_ARG(o && gate && og && M > 0 && D > 0 && D % 8 == 0, "%s: null pointer or D %% 8 != 0", who);
    VT_CHECK_ARG(gate_rs >= D && gate_rs % 8 == 0, "%s: gate row stride %lld must be >= D = %d and a multiple of 8", who, (long long)gate_rs, D);
    VT_CHECK_ARG(aligned16(o) && aligned16(gate) && aligned16(og), "%s: buffers must be 16-byte aligned", who);
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(grid_for(M * (D / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)o, (const bf16_t*)gate, gate_rs, M, D,
                       (bf16_t*)og);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
extern "C" int vt_sigmoid_gate_cols_fwd(const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* og, vtStream stream) {
    return gate_cols_fwd("vt_sigmoid_gate_cols_fwd", o, gate, gate_rs, M, D, og, stream);
}

static int gate_cols_bwd(const char* who, const void* dog, const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* d_o, void* dgate,
                         int64_t dgate_rs, vtStream stream) {
    VT_CHECK_ARG(dog && o && gate && d_o && dgate && M > 0 && D > 0 && D % 8 == 0, "%s: null pointer or D %% 8 != 0", who);
    VT_CHECK_ARG(gate_rs >= D && gate_rs % 8 == 0 && dgate_rs >= D && dgate_rs % 8 == 0, "%s: gate row strides %lld, %lld must be >= D = %d and multiples of 8", who,
                 (long long)gate_rs, (long long)dgate_rs, D);
    VT_CHECK_ARG(aligned16(dog) && aligned16(o) && aligned16(gate) && aligned16(d_o) && aligned16(dgate), "%s: buffers must be 16-byte aligned", who);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(grid_for(M * (D / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dog, (const bf16_t*)o,
                       (const bf16_t*)gate, gate_rs, M, D, (bf16_t*)d_o, (bf16_t*)dgate, dgate_rs);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
extern "C" int vt_sigmoid_gate_cols_bwd(const void* dog, const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* d_o, void* dgate,
                                        int64_t dgate_rs, vtStream stream) {
    return gate_cols_bwd("vt_sigmoid_gate_cols_bwd", dog, o, gate, gate_rs, M, D, d_o, dgate, dgate_rs, stream);
}

// the block's layout: the gate is columns 3D..4D of the [M, 4D] projection, its gradient the same columns of dqkvg
extern "C" int vt_sigmoid_gate_fwd(const void* o, const void* qkvg, int64_t M, int32_t D, void* og, vtStream stream) {
    VT_CHECK_ARG(o && qkvg && og && M > 0 && D > 0 && D % 8 == 0, "vt_sigmoid_gate_fwd: null pointer or D %% 8 != 0");
    VT_CHECK_ARG(aligned16(o) && aligned16(qkvg) && aligned16(og), "vt_sigmoid_gate_fwd: buffers must be 16-byte aligned");
    return gate_cols_fwd("vt_sigmoid_gate_fwd", o, (const bf16_t*)qkvg + 3 * (int64_t)D, 4 * (int64_t)D, M, D, og, stream);
}

extern "C" int vt_sigmoid_gate_bwd(const void* dog, const void* o, const void* qkvg, int64_t M, int32_t D, void* d_o, void* dqkvg, vtStream stream) {
    VT_CHECK_ARG(dog && o && qkvg && d_o && dqkvg && M > 0 && D > 0 && D % 8 == 0, "vt_sigmoid_gate_bwd: null pointer or D %% 8 != 0");
    VT_CHECK_ARG(aligned16(dog) && aligned16(o) && aligned16(qkvg) && aligned16(d_o) && aligned16(dqkvg), "vt_sigmoid_gate_bwd: buffers must be 16-byte aligned");
    return gate_cols_bwd("vt_sigmoid_gate_bwd", dog, o, (const bf16_t*)qkvg + 3 * (int64_t)D, 4 * (int64_t)D, M, D, d_o, (bf16_t*)dqkvg + 3 * (int64_t)D, 4 * (int64_t)D, stream);
}

extern "C" int vt_geglu_fwd(const void* h, int64_t M, int32_t I, void* a, int64_t lda, vtStream stream) {
    VT_CHECK_ARG(h && a && M > 0 && I > 0 && I % 8 == 0 && lda >= I && lda % 8 == 0, "vt_geglu_fwd: null pointer, I %% 8 != 0 or bad lda");
    VT_CHECK_ARG(aligned16(h) && aligned16(a), "vt_geglu_fwd: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(geglu_fwd_kernel, dim3(grid_for(M * (I / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h, M, I, (bf16_t*)a, lda);
    VT_CHECK_LAUNCH("vt_geglu_fwd");
    return VT_OK;
}

extern "C" int vt_geglu_bwd(const void* da, int64_t lda, const void* h, int64_t M, int32_t I, void* dh, vtStream stream) {
    VT_CHECK_ARG(da && h && dh && M > 0 && I > 0 && I % 8 == 0 && lda >= I && lda % 8 == 0, "vt_geglu_bwd: null pointer, I %% 8 != 0 or bad lda");
    VT_CHECK_ARG(aligned16(da) && aligned16(h) && aligned16(dh), "vt_geglu_bwd: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(geglu_bwd_kernel, dim3(grid_for(M * (I / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)da, lda, (const bf16_t*)h, M, I, (bf16_t*)dh);
    VT_CHECK_LAUNCH("vt_geglu_bwd");
    return VT_OK;
}
