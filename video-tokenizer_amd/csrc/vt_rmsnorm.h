// RMSNorm over the rows of an fp32 [rows, dim] matrix (models/norm.py:6-17; RMSNorm of models/model_design/base/transformer.py:18-27 on an
// fp32 input): the kernel templates behind the three entry-point families of vt_rmsnorm.hip.  T is the type of the forward's output and of the
// backward's incoming gradient: bf16_t (vt_rmsnorm_*, vt_rmsnorm_any_*: a bf16 GEMM reads y) or float (vt_rmsnorm_any_f32_*: unrounded).  One
// source, so the families agree bit for bit wherever two of them accept the same problem.
#pragma once
#include "vt_common.h"

namespace {

// one wave per row; lane l owns the float2 pieces (j * 64 + l), j < J = dim / 128: every load instruction of the wave is a
// contiguous 512-byte run.  J in {3, 6, 8, 10, 12, 20} <=> dim in {384, 768, 1024, 1280, 1536, 2560} (every llama-abs size); J in {1, 2, 4}
// <=> dim in {128, 256, 512} for the widths of model_design.
template <int J, typename T>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float eps, int64_t rows,
                                                           T* __restrict__ y, float* __restrict__ rstd_out) {
    constexpr int dim = J * 128;
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const f32x2* xr = (const f32x2*)(x + r * dim);
        f32x2 v[J];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            v[j] = xr[j * 64 + lane];
            ss = fmaf(v[j][0], v[j][0], ss);
            ss = fmaf(v[j][1], v[j][1], ss);
        }
        ss = wave_sum(ss);
        const float rstd = __builtin_amdgcn_rsqf(ss * (1.0f / dim) + eps);
        if (lane == 0 && rstd_out) rstd_out[r] = rstd;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const f32x2 o = v[j] * rstd * ((const f32x2*)w)[j * 64 + lane];
            if constexpr (sizeof(T) == 4) ((f32x2*)(y + r * dim))[j * 64 + lane] = o;
            else ((bf16x2*)(y + r * dim))[j * 64 + lane] = (bf16x2){f2bf(o[0]), f2bf(o[1])};
        }
    }
}

// dx = rstd * g - x * rstd^3 / dim * sum(x * g) (+ dres), g = w * dy; per-block partial sums of dw = sum_rows dy * x * rstd.  The residual
// gradient dres, the bf16 copy dxb and an absent dx are the bf16 family's (each optional); with T = float they are compiled out and dx is written.
template <int J, typename T>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ rstd_in, const float* __restrict__ dres, int64_t rows,
                                                           float* __restrict__ dx, bf16_t* __restrict__ dxb, float* __restrict__ dw_part) {
    constexpr int dim = J * 128;
    constexpr bool kF32 = sizeof(T) == 4;
    __shared__ float red[4][dim];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    f32x2 dwacc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) dwacc[j] = (f32x2){0.f, 0.f};
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {
        const f32x2* xr = (const f32x2*)(x + r * dim);
        const float rstd = rstd_in[r];
        f32x2 xv[J], g[J];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            xv[j] = xr[j * 64 + lane];
            f32x2 dyf;
            if constexpr (kF32) {
                dyf = ((const f32x2*)(dy + r * dim))[j * 64 + lane];
            } else {
                const bf16x2 d = ((const bf16x2*)(dy + r * dim))[j * 64 + lane];
                dyf = (f32x2){bf2f(d[0]), bf2f(d[1])};
            }
            g[j] = dyf * ((const f32x2*)w)[j * 64 + lane];
            dot = fmaf(xv[j][0], g[j][0], dot);
            dot = fmaf(xv[j][1], g[j][1], dot);
            dwacc[j] += dyf * xv[j] * rstd;
        }
        dot = wave_sum(dot);
        const float k = dot * rstd * rstd * rstd * (1.0f / dim);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            f32x2 o = g[j] * rstd - xv[j] * k;
            if constexpr (kF32) {
                ((f32x2*)(dx + r * dim))[j * 64 + lane] = o;
            } else {
                if (dres) o += ((const f32x2*)(dres + r * dim))[j * 64 + lane];
                if (dx) ((f32x2*)(dx + r * dim))[j * 64 + lane] = o;
                if (dxb) ((bf16x2*)(dxb + r * dim))[j * 64 + lane] = (bf16x2){f2bf(o[0]), f2bf(o[1])};
            }
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) ((f32x2*)red[wv])[j * 64 + lane] = dwacc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < dim; c += 256) dw_part[(int64_t)blockIdx.x * dim + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

constexpr int RMS_BLOCKS = 256;   // partial-sum rows of the weight gradient (fixed: the reduction order does not depend on the row count)

}  // namespace
