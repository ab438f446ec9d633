// A 64-element head vector spread over 8 lanes x 8 elements, and the per-head RMSNorm on it: the device helpers shared by the row passes of
// vt_gated.hip (qknorm_rope, the gates, GEGLU), vt_cross.hip (head_rmsnorm) and vt_design.hip (qkrms_rope).  One source, so that the fused
// q/k pass of vt_design.hip and the chain vt_head_rmsnorm_* + vt_rope_rotate agree bit for bit by construction: every multiply-add is an
// explicit fmaf (the contraction hipcc chose when the products were left to it), none is left for the compiler to fuse or not.
#pragma once
#include "vt_common.h"

namespace {
constexpr int HD = 64;       // head_dim (dim = 64 * heads at every model size)
constexpr int VPB = 32;      // head vectors per 256-thread block: 8 lanes x 8 elements = one head vector

// sum over the 8 lanes of a head vector
__device__ __forceinline__ float sum8(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

struct Vec8 {
    float v[8];
};
__device__ __forceinline__ Vec8 load8(const bf16_t* p) {
    const bf16x8 r = *(const bf16x8*)p;
    Vec8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] = bf2f(r[i]);
    return o;
}
__device__ __forceinline__ void store8(bf16_t* p, const Vec8& a) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = f2bf(a.v[i]);
    *(bf16x8*)p = r;
}

// rsqrt(mean(x^2) + eps) of one head vector
__device__ __forceinline__ float head_rstd(const Vec8& x, float eps) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss = fmaf(x.v[i], x.v[i], ss);
    return __builtin_amdgcn_rsqf(fmaf(sum8(ss), 1.0f / HD, eps));
}

// backward of y = x * rstd * w on one head vector, all in fp32: returns dx = rstd g - x rstd^3 / 64 sum(x g), g = w gy, and adds this
// vector's gy * (x rstd) to the lane's 8 weight-gradient accumulators aw (the forward's rounding of x * rstd is not replayed)
__device__ __forceinline__ Vec8 head_rmsnorm_bwd_step(const Vec8& xv, const Vec8& gy, const float (&wr)[8], float rstd, float (&aw)[8]) {
    float g[8], dot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        g[i] = gy.v[i] * wr[i];
        dot = fmaf(xv.v[i], g[i], dot);
        aw[i] = fmaf(gy.v[i], xv.v[i] * rstd, aw[i]);
    }
    const float k = sum8(dot) * rstd * rstd * rstd * (1.0f / HD);
    Vec8 dx;
#pragma unroll
    for (int i = 0; i < 8; ++i) dx.v[i] = fmaf(g[i], rstd, -(xv.v[i] * k));
    return dx;
}
}  // namespace
