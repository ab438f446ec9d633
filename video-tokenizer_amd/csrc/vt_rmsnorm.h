// RMSNorm over the rows of an fp32 [rows, dim] matrix (models/norm.py:6-17; RMSNorm of models/model_design/base/transformer.py:18-27 on an
// fp32 input): the kernel templates behind vt_rmsnorm_* (vt_ar.hip, the llama-abs widths) and vt_rmsnorm_any_* (vt_cross.hip, those plus
// 128 / 256 / 512).  One source, so the two families agree bit for bit at the widths both accept.
#pragma once
#include "vt_common.h"

namespace {

// one wave per row; lane l owns the float2 pieces (j * 64 + l), j < J = dim / 128: every load instruction of the wave is a
// contiguous 512-byte run.  J in {3, 6, 8, 10, 12, 20} <=> dim in {384, 768, 1024, 1280, 1536, 2560} (every llama-abs size); J in {1, 2, 4}
// <=> dim in {128, 256, 512} for vt_rmsnorm_any_*.
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int J>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float eps, int64_t rows,
                                                           bf16_t* __restrict__ y, float* __restrict__ rstd_out) {
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
        bf16x2* yr = (bf16x2*)(y + r * dim);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const f32x2 ww = ((const f32x2*)w)[j * 64 + lane];
            yr[j * 64 + lane] = (bf16x2){f2bf(v[j][0] * rstd * ww[0]), f2bf(v[j][1] * rstd * ww[1])};
        }
    }
}

// dx = rstd * g - x * rstd^3 / dim * sum(x * g) (+ dres), g = w * dy; per-block partial sums of dw = sum_rows dy * x * rstd
template <int J>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ rstd_in, const float* __restrict__ dres, int64_t rows,
                                                           float* __restrict__ dx, bf16_t* __restrict__ dxb, float* __restrict__ dw_part) {
    constexpr int dim = J * 128;
    __shared__ float red[4][dim];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    f32x2 dwacc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) dwacc[j] = (f32x2){0.f, 0.f};
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {
        const f32x2* xr = (const f32x2*)(x + r * dim);
        const bf16x2* dyr = (const bf16x2*)(dy + r * dim);
        const float rstd = rstd_in[r];
        f32x2 xv[J], g[J];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            xv[j] = xr[j * 64 + lane];
            const bf16x2 d = dyr[j * 64 + lane];
            const f32x2 ww = ((const f32x2*)w)[j * 64 + lane];
            const f32x2 dyf = {bf2f(d[0]), bf2f(d[1])};
            g[j] = dyf * ww;
            dot = fmaf(xv[j][0], g[j][0], dot);
            dot = fmaf(xv[j][1], g[j][1], dot);
            dwacc[j] += dyf * xv[j] * rstd;
        }
        dot = wave_sum(dot);
        const float k = dot * rstd * rstd * rstd * (1.0f / dim);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            f32x2 o = g[j] * rstd - xv[j] * k;
            if (dres) o += ((const f32x2*)(dres + r * dim))[j * 64 + lane];
            if (dx) ((f32x2*)(dx + r * dim))[j * 64 + lane] = o;
            if (dxb) ((bf16x2*)(dxb + r * dim))[j * 64 + lane] = (bf16x2){f2bf(o[0]), f2bf(o[1])};
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) ((f32x2*)red[wv])[j * 64 + lane] = dwacc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < dim; c += 256) dw_part[(int64_t)blockIdx.x * dim + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

constexpr int RMS_BLOCKS = 256;   // partial-sum rows of the weight gradient (fixed: the reduction order does not depend on the row count)

}  // namespace
