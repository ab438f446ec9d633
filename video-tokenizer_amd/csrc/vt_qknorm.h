// Per-head LayerNorm + rotary on the q and k column blocks of a projection, v copied, and the backward of that pass: the kernels behind
// vt_qknorm_rope_* (vt_gated.hip: [M, 4D] -> [M, 3D], one head count, row m at position m % L) and behind their grouped twin
// vt_qknorm_rope_gqa_* (vt_varlen.hip: [M, 64 (Hq + 2 Hkv)] with row strides, Hq query heads and Hkv KV heads, row m at table row m).
// ONE kernel source for both, so that the two entry points agree bit for bit wherever they see the same vectors: the dense caller passes
// Hq = Hkv = H, the grouped one L = M.  Built on the head-vector helpers of vt_headvec.h.
#pragma once
#include "vt_common.h"
#include "vt_headvec.h"

namespace {
constexpr int QKN_NBLK = 512;    // blocks per operand in the backward (partial sums: [QKN_NBLK, 2, 2, 64] fp32)

// LayerNorm statistics of one 64-vector spread over 8 lanes (biased variance, two passes in registers)
__device__ __forceinline__ void ln_stats(const Vec8& x, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += x.v[i];
    mean = sum8(s) * (1.0f / HD);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) q += (x.v[i] - mean) * (x.v[i] - mean);
    rstd = 1.0f / sqrtf(sum8(q) * (1.0f / HD) + eps);
}

// The column blocks q | k | v of a row: block `which` has Hw heads and starts at column coff (the same in the input, the output and both
// gradients; only the row strides differ).
struct QknBlock {
    int Hw;
    int64_t coff;
};
__device__ __forceinline__ QknBlock qkn_block(int which, int Hq, int Hkv) {
    QknBlock b;
    b.Hw = which == 0 ? Hq : Hkv;
    b.coff = which == 0 ? 0 : which == 1 ? (int64_t)Hq * HD : (int64_t)(Hq + Hkv) * HD;
    return b;
}

// grid (blocks, 3): y = 0 -> q, 1 -> k, 2 -> v (copy)
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const bf16_t* __restrict__ qkvg, int64_t in_rs, int64_t M, int64_t L, int Hq, int Hkv,
                                                               const float* __restrict__ q_w, const float* __restrict__ q_b,
                                                               const float* __restrict__ k_w, const float* __restrict__ k_b, float eps,
                                                               const float* __restrict__ cs, const float* __restrict__ sn, bf16_t* __restrict__ out,
                                                               int64_t out_rs) {
    const int which = blockIdx.y, lane = threadIdx.x & 7;
    const QknBlock blk = qkn_block(which, Hq, Hkv);
    const int H = blk.Hw;
    const int64_t nvec = M * H;
    const float* w = which == 0 ? q_w : k_w;
    const float* b = which == 0 ? q_b : k_b;
    float wr[8], br[8];
    if (which < 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wr[i] = w[lane * 8 + i], br[i] = b[lane * 8 + i];
    }
    for (int64_t vec = (int64_t)blockIdx.x * VPB + (threadIdx.x >> 3); vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int head = (int)(vec % H);
        const bf16_t* src = qkvg + row * in_rs + blk.coff + head * HD + lane * 8;
        bf16_t* dst = out + row * out_rs + blk.coff + head * HD + lane * 8;
        if (which == 2) {
            *(bf16x8*)dst = *(const bf16x8*)src;
            continue;
        }
        Vec8 x = load8(src);
        float mean, rstd;
        ln_stats(x, eps, mean, rstd);
        const int64_t pos = row % L;
        const f32x4 c = *(const f32x4*)(cs + pos * (HD / 2) + lane * 4);
        const f32x4 s = *(const f32x4*)(sn + pos * (HD / 2) + lane * 4);
        Vec8 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = round_bf16((x.v[2 * j] - mean) * rstd * wr[2 * j] + br[2 * j]);
            const float bb = round_bf16((x.v[2 * j + 1] - mean) * rstd * wr[2 * j + 1] + br[2 * j + 1]);
            y.v[2 * j] = a * c[j] - bb * s[j];
            y.v[2 * j + 1] = a * s[j] + bb * c[j];
        }
        store8(dst, y);
    }
}

// grid (QKN_NBLK, 3).  part: [QKN_NBLK, 2(which), 2(w|b), 64].  dqkv: gradient of the pass's output (row stride g_rs); dqkvg: gradient of its input
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const bf16_t* __restrict__ qkvg, int64_t in_rs, const bf16_t* __restrict__ dqkv,
                                                               int64_t g_rs, int64_t M, int64_t L, int Hq, int Hkv, const float* __restrict__ q_w,
                                                               const float* __restrict__ k_w, float eps, const float* __restrict__ cs,
                                                               const float* __restrict__ sn, bf16_t* __restrict__ dqkvg, int64_t d_rs,
                                                               float* __restrict__ part) {
    __shared__ float red[2][VPB][HD];
    const int which = blockIdx.y, lane = threadIdx.x & 7, vslot = threadIdx.x >> 3;
    const QknBlock blk = qkn_block(which, Hq, Hkv);
    const int H = blk.Hw;
    const int64_t nvec = M * H;
    float wr[8], aw[8], ab[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) aw[i] = 0.f, ab[i] = 0.f, wr[i] = which < 2 ? (which == 0 ? q_w : k_w)[lane * 8 + i] : 0.f;
    for (int64_t vec = (int64_t)blockIdx.x * VPB + vslot; vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int head = (int)(vec % H);
        const bf16_t* gsrc = dqkv + row * g_rs + blk.coff + head * HD + lane * 8;
        bf16_t* dst = dqkvg + row * d_rs + blk.coff + head * HD + lane * 8;
        if (which == 2) {
            *(bf16x8*)dst = *(const bf16x8*)gsrc;
            continue;
        }
        const Vec8 x = load8(qkvg + row * in_rs + blk.coff + head * HD + lane * 8);
        const Vec8 gy = load8(gsrc);
        float mean, rstd;
        ln_stats(x, eps, mean, rstd);
        const int64_t pos = row % L;
        const f32x4 c = *(const f32x4*)(cs + pos * (HD / 2) + lane * 4);
        const f32x4 s = *(const f32x4*)(sn + pos * (HD / 2) + lane * 4);
        // transpose of the rotation, rounded to bf16 (the gradient of a bf16 tensor), then LayerNorm backward in fp32
        float g[8], xh[8], m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[2 * j] = round_bf16(gy.v[2 * j] * c[j] + gy.v[2 * j + 1] * s[j]);
            g[2 * j + 1] = round_bf16(gy.v[2 * j + 1] * c[j] - gy.v[2 * j] * s[j]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            xh[i] = (x.v[i] - mean) * rstd;
            aw[i] += g[i] * xh[i];
            ab[i] += g[i];
            m1 += g[i] * wr[i];
            m2 += g[i] * wr[i] * xh[i];
        }
        m1 = sum8(m1) * (1.0f / HD);
        m2 = sum8(m2) * (1.0f / HD);
        Vec8 dx;
#pragma unroll
        for (int i = 0; i < 8; ++i) dx.v[i] = rstd * (g[i] * wr[i] - m1 - xh[i] * m2);
        store8(dst, dx);
    }
    if (which == 2) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) red[0][vslot][lane * 8 + i] = aw[i], red[1][vslot][lane * 8 + i] = ab[i];
    __syncthreads();
    if (threadIdx.x < 2 * HD) {
        const int wb = threadIdx.x >> 6, e = threadIdx.x & 63;
        float t = 0.f;
#pragma unroll 8
        for (int v = 0; v < VPB; ++v) t += red[wb][v][e];
        part[(((int64_t)blockIdx.x * 2 + which) * 2 + wb) * HD + e] = t;
    }
}

// blocks along x of the forward: one per 32 head vectors of the larger operand, at most 2048
inline int qkn_fwd_grid(int64_t M, int H) {
    const int64_t nvec = M * H;
    return (int)((nvec + VPB - 1) / VPB < 2048 ? (nvec + VPB - 1) / VPB : 2048);
}
}  // namespace
