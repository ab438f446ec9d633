// Row passes of model_design's self-attention block and stack (models/model_design/base/transformer.py:46-85, 148-216) for gfx950.
// The GEMMs, the attention, the gate, GEGLU and the whole-row RMSNorms (vt_rmsnorm_any_*, vt_rmsnorm_any_f32_* for final_norm: vt_rmsnorm.hip)
// are the kernels the other layers already use; new here:
//   qkrms_rope      q_norm / k_norm (RMSNorm per 64-wide head, weight only, :76-77) and the rotary embedding (:79-80) of q and k, v copied:
//                   reads columns q | k | v of the [M, 4D] output of ONE GEMM on [to_qkv ; to_gate], writes the packed [M, 3D] operand of
//                   vt_attention_fwd.  The RMS twin of vt_qknorm_rope_* (vt_gated.hip); bit for bit vt_head_rmsnorm_* + vt_rope_rotate: the
//                   norm's statistics and backward step are the same functions of vt_headvec.h that vt_cross.hip calls.
//   residual_scale  x + res_scale * f(x) (:176-183) with res_scale a 0-dim PARAMETER read from device memory (no host read, capturable),
//                   and its backward with the full-reduction gradient of the scale from fixed-order partial sums.
// HBM-bound single passes, 16 bytes per lane and access, no float atomics, no device trigonometry (cos / sin come from the tables).
#include "vt_common.h"
#include "vt_headvec.h"

namespace {
constexpr int NBLK = 512;     // blocks per operand of the q/k backward = partial sums of dq_w / dk_w: [NBLK, 2, 64] fp32
constexpr int RS_BLOCKS = 256;   // blocks of the scaled-residual backward = partial sums of d(res_scale)

// the rotation of vt_rope_rotate (vt_rope.hip): x holds bf16 values, sgn = 1 (forward) or -1 (conjugate).  That kernel rounds b sin in the
// first and a sin in the second component and fuses the cos products (read off its ISA); the same here
__device__ __forceinline__ Vec8 rotate8(const Vec8& x, const float* __restrict__ ct, const float* __restrict__ st, int lane, float sgn) {
    const f32x4 co = *(const f32x4*)(ct + lane * 4);
    const f32x4 si = *(const f32x4*)(st + lane * 4) * sgn;
    Vec8 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = x.v[2 * i], b = x.v[2 * i + 1];
        y.v[2 * i] = fmaf(a, co[i], -(b * si[i]));
        y.v[2 * i + 1] = fmaf(b, co[i], a * si[i]);
    }
    return y;
}

// grid (blocks, 3): y = 0 -> q, 1 -> k, 2 -> v (copy).  Rows M .. of a padded buffer and the columns past 3D of the input are not touched.
__global__ __launch_bounds__(256) void qkrms_rope_fwd_kernel(const bf16_t* __restrict__ qkvg, int64_t in_rs, int64_t M, int L, int H,
                                                              const float* __restrict__ q_w, const float* __restrict__ k_w, float eps,
                                                              const float* __restrict__ cs, const float* __restrict__ sn, bf16_t* __restrict__ out,
                                                              int64_t out_rs, float sgn) {
    const int which = blockIdx.y, lane = threadIdx.x & 7;
    const int64_t D = (int64_t)H * HD, nvec = M * H;
    float wr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wr[i] = which < 2 ? (which == 0 ? q_w : k_w)[lane * 8 + i] : 0.f;
    for (int64_t vec = (int64_t)blockIdx.x * VPB + (threadIdx.x >> 3); vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int64_t col = which * D + (vec % H) * HD + lane * 8;
        const bf16_t* src = qkvg + row * in_rs + col;
        bf16_t* dst = out + row * out_rs + col;
        if (which == 2) {
            *(bf16x8*)dst = *(const bf16x8*)src;
            continue;
        }
        const Vec8 xv = load8(src);
        const float rstd = head_rstd(xv, eps);
        Vec8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t.v[i] = round_bf16(round_bf16(xv.v[i] * rstd) * wr[i]);     // = the bf16 tensor q_norm(q) of the reference
        const int64_t pos = row % L;
        store8(dst, rotate8(t, cs + pos * (HD / 2), sn + pos * (HD / 2), lane, sgn));
    }
}

// grid (NBLK, 3).  part: [NBLK, 2(which), 64].  dq / dk: conjugate rotation rounded to bf16 (autograd rounds there), then the backward step of
// vt_head_rmsnorm_bwd with rstd recomputed from qkvg.
__global__ __launch_bounds__(256) void qkrms_rope_bwd_kernel(const bf16_t* __restrict__ qkvg, int64_t in_rs, const bf16_t* __restrict__ dqkv, int64_t M, int L,
                                                              int H, const float* __restrict__ q_w, const float* __restrict__ k_w, float eps,
                                                              const float* __restrict__ cs, const float* __restrict__ sn, bf16_t* __restrict__ dqkvg,
                                                              int64_t out_rs, float sgn, float* __restrict__ part) {
    __shared__ float red[VPB][HD];
    const int which = blockIdx.y, lane = threadIdx.x & 7, vslot = threadIdx.x >> 3;
    const int64_t D = (int64_t)H * HD, nvec = M * H;
    float wr[8], aw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) aw[i] = 0.f, wr[i] = which < 2 ? (which == 0 ? q_w : k_w)[lane * 8 + i] : 0.f;
    for (int64_t vec = (int64_t)blockIdx.x * VPB + vslot; vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int64_t col = which * D + (vec % H) * HD + lane * 8;
        const bf16_t* gsrc = dqkv + row * 3 * D + col;
        bf16_t* dst = dqkvg + row * out_rs + col;
        if (which == 2) {
            *(bf16x8*)dst = *(const bf16x8*)gsrc;
            continue;
        }
        const Vec8 xv = load8(qkvg + row * in_rs + col);
        const int64_t pos = row % L;
        Vec8 gy = rotate8(load8(gsrc), cs + pos * (HD / 2), sn + pos * (HD / 2), lane, sgn);
#pragma unroll
        for (int i = 0; i < 8; ++i) gy.v[i] = round_bf16(gy.v[i]);
        store8(dst, head_rmsnorm_bwd_step(xv, gy, wr, head_rstd(xv, eps), aw));
    }
    if (which == 2) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) red[vslot][lane * 8 + i] = aw[i];
    __syncthreads();
    if (threadIdx.x < HD) {
        float t = 0.f;
#pragma unroll 8
        for (int v = 0; v < VPB; ++v) t += red[v][threadIdx.x];
        part[((int64_t)blockIdx.x * 2 + which) * HD + threadIdx.x] = t;
    }
}

// ---- scaled residual.  torch multiplies the bf16 tensor y by the 0-dim fp32 parameter in bf16: the parameter is converted to the common
// dtype first, the product is formed in fp32 and rounded once; the fp32 stream x is added after.
__global__ __launch_bounds__(256) void residual_scale_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ s_ptr,
                                                                  int64_t n4, float* __restrict__ out) {
    const float s = round_bf16(*s_ptr);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 xv = ((const f32x4*)x)[i], yv = ((const f32x4*)y)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = xv[j] + round_bf16(s * round_bf16(yv[j]));
        ((f32x4*)out)[i] = o;
    }
}

// g = bf16(dout); dy = bf16(s g); part[block] = sum over the block's elements of g y, every thread's terms in index order, then a
// fixed butterfly and the four waves in order
__global__ __launch_bounds__(256) void residual_scale_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ s_ptr,
                                                                  int64_t n4, float* __restrict__ dy, float* __restrict__ part) {
    __shared__ float red[4];
    const float s = round_bf16(*s_ptr);
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 gv = ((const f32x4*)dout)[i];
        f32x4 o;
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = round_bf16(gv[j]), o[j] = round_bf16(s * g[j]);
        ((f32x4*)dy)[i] = o;
        if (part) {
            const f32x4 yv = ((const f32x4*)y)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fmaf(g[j], round_bf16(yv[j]), acc);
        }
    }
    if (!part) return;
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

bool stride_ok(int64_t rs, int H) { return rs >= (int64_t)3 * HD * H && rs % 8 == 0; }
}  // namespace

extern "C" int vt_qkrms_rope_fwd(const void* qkvg, int64_t in_rs, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w, float eps,
                                 const float* cos_tab, const float* sin_tab, void* qkv_out, int64_t out_rs, vtStream stream) {
    VT_CHECK_ARG(qkvg && qkv_out && q_w && k_w && cos_tab && sin_tab, "vt_qkrms_rope_fwd: null pointer");
    VT_CHECK_ARG(M > 0 && L > 0 && H > 0 && H <= 1024 && M % L == 0, "vt_qkrms_rope_fwd: need M = B * L rows, H heads of 64 (M=%lld L=%d H=%d)", (long long)M, L, H);
    VT_CHECK_ARG(stride_ok(in_rs, H) && stride_ok(out_rs, H), "vt_qkrms_rope_fwd: row strides %lld, %lld must cover 3 x 64 x %d columns and be multiples of 8",
                 (long long)in_rs, (long long)out_rs, H);
    VT_CHECK_ARG(aligned16(qkvg) && aligned16(qkv_out) && aligned16(cos_tab) && aligned16(sin_tab), "vt_qkrms_rope_fwd: buffers must be 16-byte aligned");
    const int64_t nvec = M * H;
    const int gx = (int)((nvec + VPB - 1) / VPB < 2048 ? (nvec + VPB - 1) / VPB : 2048);
    hipLaunchKernelGGL(qkrms_rope_fwd_kernel, dim3(gx, 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkvg, in_rs, M, L, H, q_w, k_w, eps, cos_tab,
                       sin_tab, (bf16_t*)qkv_out, out_rs, 1.0f);
    VT_CHECK_LAUNCH("vt_qkrms_rope_fwd");
    return VT_OK;
}

extern "C" size_t vt_qkrms_rope_bwd_workspace_bytes(void) { return (size_t)NBLK * 2 * HD * sizeof(float); }

extern "C" int vt_qkrms_rope_bwd(const void* qkvg, int64_t in_rs, const void* dqkv, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w,
                                 float eps, const float* cos_tab, const float* sin_tab, void* dqkvg, int64_t out_rs, float* dq_w, float* dk_w,
                                 void* workspace, vtStream stream) {
    VT_CHECK_ARG(qkvg && dqkv && dqkvg && q_w && k_w && cos_tab && sin_tab && workspace, "vt_qkrms_rope_bwd: null pointer");
    VT_CHECK_ARG(M > 0 && L > 0 && H > 0 && H <= 1024 && M % L == 0, "vt_qkrms_rope_bwd: need M = B * L rows, H heads of 64 (M=%lld L=%d H=%d)", (long long)M, L, H);
    VT_CHECK_ARG(stride_ok(in_rs, H) && stride_ok(out_rs, H), "vt_qkrms_rope_bwd: row strides %lld, %lld must cover 3 x 64 x %d columns and be multiples of 8",
                 (long long)in_rs, (long long)out_rs, H);
    VT_CHECK_ARG(aligned16(qkvg) && aligned16(dqkv) && aligned16(dqkvg) && aligned16(cos_tab) && aligned16(sin_tab) && aligned16(workspace),
                 "vt_qkrms_rope_bwd: buffers must be 16-byte aligned");
    VT_CHECK_ARG(dqkvg != qkvg && dqkvg != dqkv, "vt_qkrms_rope_bwd: not in place (dqkvg is a buffer of its own)");
    hipLaunchKernelGGL(qkrms_rope_bwd_kernel, dim3(NBLK, 3), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkvg, in_rs, (const bf16_t*)dqkv, M, L, H, q_w,
                       k_w, eps, cos_tab, sin_tab, (bf16_t*)dqkvg, out_rs, -1.0f, (float*)workspace);
    VT_CHECK_LAUNCH("vt_qkrms_rope_bwd");
    if (!dq_w && !dk_w) return VT_OK;
    return vt_reduce_waves("vt_qkrms_rope_bwd(reduce)", (const float*)workspace, NBLK, 2 * HD, 2 * HD, dq_w, dk_w, nullptr, nullptr, stream);
}

static int rs_grid(int64_t n4, int cap) {
    const int64_t b = (n4 + 255) / 256;
    return (int)(b < cap ? b : cap);
}

extern "C" int vt_residual_scale_fwd(const float* x, const float* y, const float* scale_dev, int64_t rows, int32_t dim, float* out, vtStream stream) {
    VT_CHECK_ARG(x && y && scale_dev && out, "vt_residual_scale_fwd: null pointer");
    VT_CHECK_ARG(rows > 0 && dim > 0 && dim % 4 == 0, "vt_residual_scale_fwd: rows=%lld dim=%d: need rows > 0 and dim %% 4 == 0", (long long)rows, dim);
    VT_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(out), "vt_residual_scale_fwd: buffers must be 16-byte aligned");
    VT_CHECK_ARG(out != x && out != y, "vt_residual_scale_fwd: not in place (out is a buffer of its own)");
    const int64_t n4 = rows * dim / 4;
    hipLaunchKernelGGL(residual_scale_fwd_kernel, dim3(rs_grid(n4, 4096)), dim3(256), 0, (hipStream_t)stream, x, y, scale_dev, n4, out);
    VT_CHECK_LAUNCH("vt_residual_scale_fwd");
    return VT_OK;
}

extern "C" size_t vt_residual_scale_bwd_workspace_bytes(void) { return (size_t)RS_BLOCKS * sizeof(float); }

extern "C" int vt_residual_scale_bwd(const float* dout, const float* y, const float* scale_dev, int64_t rows, int32_t dim, float* dy, float* dscale,
                                     void* workspace, vtStream stream) {
    VT_CHECK_ARG(dout && scale_dev && dy && (!dscale || (y && workspace)), "vt_residual_scale_bwd: null pointer");
    VT_CHECK_ARG(rows > 0 && dim > 0 && dim % 4 == 0, "vt_residual_scale_bwd: rows=%lld dim=%d: need rows > 0 and dim %% 4 == 0", (long long)rows, dim);
    VT_CHECK_ARG(aligned16(dout) && aligned16(y) && aligned16(dy) && aligned16(workspace), "vt_residual_scale_bwd: buffers must be 16-byte aligned");
    VT_CHECK_ARG(dy != dout && dy != y, "vt_residual_scale_bwd: not in place (dy is a buffer of its own)");
    const int64_t n4 = rows * dim / 4;
    const int grid = rs_grid(n4, RS_BLOCKS);
    hipLaunchKernelGGL(residual_scale_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dout, y, scale_dev, n4, dy, dscale ? (float*)workspace : nullptr);
    VT_CHECK_LAUNCH("vt_residual_scale_bwd");
    if (!dscale) return VT_OK;
    return vt_reduce_waves("vt_residual_scale_bwd(reduce)", (const float*)workspace, grid, 1, 1, dscale, nullptr, nullptr, nullptr, stream);
}
