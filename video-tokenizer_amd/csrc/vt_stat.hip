// Token gate of `autoencoder_stat` for gfx950 (models/model_stat/autoencoder.py:69-138, base/blocks.py:11-24,89): the
// probability head's second Linear + sigmoid, the keep mask, and FSQ of the masked latents in one row pass; its backward in one.
//
// Forward, per latent row m (M = B * 1280 rows, W = 768 head width, d = 6 FSQ channels):
//   logit = bf16( g[m,:] . w2 + b2 )       g = gelu(fc1(x)), the bf16 output of the head's first GEMM (vt_gemm_nt VT_EPI_BF16_GELU)
//   p     = bf16( sigmoid(logit) )         autocast rounds the Linear's output and runs the sigmoid on that bf16 tensor
//   mask  = sample: u < p with u a counter-hash uniform of (seed, m) | threshold: p > 0.5 | all ones | forced (given)
//   codes, indices = FSQ(z[m,:] * mask)    per-element arithmetic of vt_fsq_device.h: bit-equal to vt_fsq_forward of z * mask
// Backward (the straight-through estimator `(mask - p).detach() + p` of the sampled / forced mask, :77-80):
//   dz    = fsq_grad(z * mask, dcodes) * mask
//   dp    = [ste] (sum_c fsq_grad(z * mask, dcodes)_c * z_c + dmask) + dprobs
//   dlogit = dp * p * (1 - p)
//   dU[m,:] = bf16( dlogit * w2 * gelu'(u[m,:]) )     the operand of the fc1 dgrad / wgrad GEMMs and the fc1 bias column sum
//   dw2 = sum_m dlogit_m g[m,:], db2 = sum_m dlogit_m: per-workgroup partials in a fixed row order, summed over workgroups in a
//   fixed order by a second launch -- no float atomics, bit-identical run to run.
//
// Both are HBM-bound row passes: a 16-lane group per row, 16-byte bf16 loads / stores (W / 128 per lane), a shfl_xor tree
// inside the group.  W % 128 == 0, W <= 1024 (the per-lane column count is a template parameter: no dynamically indexed
// register arrays, no scratch).
#include "vt_common.h"
#include "vt_fsq_device.h"

namespace {

constexpr int kGroup = 16;                    // lanes per row
constexpr int kRowsPerBlock = 256 / kGroup;   // 16 rows per 256-thread workgroup
constexpr int kMaxBwdBlocks = 512;            // partial-sum slabs of the backward (workspace = kMaxBwdBlocks * (W + 1) floats)

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// uniform in (0, 1) from (seed, row): the same hash chain as the stochastic codebook search's Gumbel noise (vt_vq.hip)
__device__ __forceinline__ float row_uniform(unsigned seed_lo, unsigned seed_hi, unsigned row) {
    const unsigned h = pcg_hash(pcg_hash(pcg_hash(seed_lo) + row) + seed_hi);
    return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int CH>
__global__ __launch_bounds__(256) void stat_gate_fwd_kernel(const bf16_t* __restrict__ g, int64_t ldg, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, const float* __restrict__ z, int64_t M, FsqConsts k,
                                                             int mode, unsigned seed_lo, unsigned seed_hi, const float* __restrict__ mask_in,
                                                             float* __restrict__ probs, float* __restrict__ mask, float* __restrict__ codes,
                                                             int32_t* __restrict__ indices) {
    const int lane = threadIdx.x % kGroup;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
    if (row >= M) return;                     // whole 16-lane groups leave together: the shuffles below stay inside a group
    const bf16x8* gr = (const bf16x8*)(g + row * ldg);
    const f32x4* w4 = (const f32x4*)w2;
    bf16x8 gv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) gv[i] = ld_stream_any(gr + lane + kGroup * i);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c8 = lane + kGroup * i;
        const f32x4 wa = w4[2 * c8], wb = w4[2 * c8 + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf((float)gv[i][e], wa[e], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf((float)gv[i][4 + e], wb[e], acc);
    }
    acc = group_sum(acc);
    const float logit = round_bf16(acc + b2[0]);
    const float p = round_bf16(sigmoid_f(logit));
    float m;
    if (mode == VT_STAT_SAMPLE) m = row_uniform(seed_lo, seed_hi, (unsigned)row) < p ? 1.0f : 0.0f;
    else if (mode == VT_STAT_THRESHOLD) m = p > 0.5f ? 1.0f : 0.0f;
    else if (mode == VT_STAT_ONES) m = 1.0f;
    else m = mask_in[row];
    if (lane == 0) {
        probs[row] = p;
        mask[row] = m;
    }
    if (z) {
        float term = 0.0f;
        if (lane < k.d) {
            const float code = fsq_code(z[row * k.d + lane] * m, k, lane);
            codes[row * k.d + lane] = code;
            term = fsq_index_term(code, k, lane);
        }
        term = group_sum(term);               // integers below 2^24: exact in any order
        if (lane == 0 && indices) indices[row] = (int32_t)term;
    }
}

template <int CH>
__global__ __launch_bounds__(256) void stat_gate_bwd_kernel(const float* __restrict__ dcodes, const float* __restrict__ dprobs,
                                                             const float* __restrict__ dmask, const float* __restrict__ z,
                                                             const float* __restrict__ mask, const float* __restrict__ probs,
                                                             const bf16_t* __restrict__ u, const bf16_t* __restrict__ g, int64_t ld,
                                                             const float* __restrict__ w2, int64_t M, int64_t rows_per_block, FsqConsts k,
                                                             int ste, bf16_t* __restrict__ dU, float* __restrict__ dz,
                                                             float* __restrict__ part) {
    constexpr int W = CH * 8 * kGroup;
    __shared__ float red[4][W + 1];
    const int lane = threadIdx.x % kGroup;
    const int grp = threadIdx.x / kGroup;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
    const f32x4* w4 = (const f32x4*)w2;
    float dw[CH][8];
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) dw[i][e] = 0.0f;
    float db = 0.0f;
    for (int64_t row = r0 + grp; row < r1; row += kRowsPerBlock) {
        const bf16x8* ur = (const bf16x8*)(u + row * ld);
        const bf16x8* gr = (const bf16x8*)(g + row * ld);
        bf16x8 uv[CH], gv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            uv[i] = ld_stream_any(ur + lane + kGroup * i);
            gv[i] = ld_stream_any(gr + lane + kGroup * i);
        }
        const float m = mask[row], p = probs[row];
        float term = 0.0f;
        if (z && lane < k.d) {
            const float zc = z[row * k.d + lane];
            const float dzm = fsq_grad(zc * m, dcodes[row * k.d + lane], k, lane);
            dz[row * k.d + lane] = dzm * m;
            term = dzm * zc;
        }
        term = group_sum(term);
        float dp = ste ? term + (dmask ? dmask[row] : 0.0f) : 0.0f;
        if (dprobs) dp += dprobs[row];
        const float dlogit = dp * p * (1.0f - p);
        db += dlogit;
        bf16x8* dr = (bf16x8*)(dU + row * ld);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c8 = lane + kGroup * i;
            const f32x4 wa = w4[2 * c8], wb = w4[2 * c8 + 1];
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float we = e < 4 ? wa[e] : wb[e - 4];
                o[e] = f2bf(dlogit * we * gelu_erf_grad((float)uv[i][e]));
                dw[i][e] = fmaf(dlogit, (float)gv[i][e], dw[i][e]);
            }
            st_stream_any(dr + c8, o);
        }
    }
    // the block's four row groups of a wave (lanes l, l + 16, l + 32, l + 48), then the four waves, in a fixed order
    const int wave = threadIdx.x / 64;
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = dw[i][e];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            dw[i][e] = v;
        }
    db += __shfl_xor(db, 16);
    db += __shfl_xor(db, 32);
    if ((threadIdx.x % 64) < kGroup) {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wave][(lane + kGroup * i) * 8 + e] = dw[i][e];
        if (lane == 0) red[wave][W] = db;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= W; c += 256)
        part[(int64_t)blockIdx.x * (W + 1) + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// dw2[c] = sum_b part[b][c] (c < W), db2 = sum_b part[b][W], in a fixed order: a workgroup owns 16 consecutive columns; thread t sums
// the slabs b = t / 16, t / 16 + 16, ... of column t % 16 in ascending order, then the 16 slab classes of a column are added by a fixed
// shfl_xor tree inside each wave (classes 4w .. 4w + 3) and the four waves' sums in wave order.  (One thread walking all slabs of a
// column was latency-bound: 77 us for 320 slabs at W = 768.)
__global__ __launch_bounds__(256) void stat_partial_sum_kernel(const float* __restrict__ part, int nblk, int W, float* __restrict__ dw2,
                                                                float* __restrict__ db2) {
    __shared__ float red[4][16];
    const int col = blockIdx.x * 16 + (threadIdx.x % 16);
    const int cls = threadIdx.x / 16;
    float s = 0.0f;
    if (col <= W) {
#pragma unroll 4
        for (int b = cls; b < nblk; b += 16) s += part[(int64_t)b * (W + 1) + col];
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if ((threadIdx.x % 64) < 16) red[threadIdx.x / 64][threadIdx.x % 16] = s;
    __syncthreads();
    if (threadIdx.x < 16 && col <= W) {
        const float t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        if (col < W) dw2[col] = t;
        else db2[0] = t;
    }
}


int check_common(const char* name, const void* z, int64_t M, int32_t W, int32_t d, const int32_t* levels_host, int64_t ld, FsqConsts& k) {
    VT_CHECK_ARG(M > 0 && W >= 128 && W <= 1024 && W % 128 == 0, "%s: need M > 0 and W a multiple of 128 in [128, 1024] (M = %lld, W = %d)", name,
                 (long long)M, W);
    VT_CHECK_ARG(ld >= W && ld % 8 == 0, "%s: row stride %lld must be >= W and a multiple of 8", name, (long long)ld);
    k.d = 0;
    if (z) {
        VT_CHECK_ARG(d >= 1 && d <= FSQ_MAX_D && levels_host, "%s: need 1 <= d <= %d and a host levels array (d = %d)", name, FSQ_MAX_D, d);
        VT_CHECK_ARG(fsq_make_consts(levels_host, d, k), "%s: every level must be >= 2 and prod(levels) <= 2^24", name);
    }
    return VT_OK;
}

#define VT_STAT_DISPATCH(CH_VAR, LAUNCH) \
    switch (CH_VAR) {                    \
        case 1: LAUNCH(1); break;        \
        case 2: LAUNCH(2); break;        \
        case 3: LAUNCH(3); break;        \
        case 4: LAUNCH(4); break;        \
        case 5: LAUNCH(5); break;        \
        case 6: LAUNCH(6); break;        \
        case 7: LAUNCH(7); break;        \
        default: LAUNCH(8); break;       \
    }
}  // namespace

extern "C" size_t vt_stat_gate_workspace_bytes(int32_t W) { return (size_t)kMaxBwdBlocks * (size_t)(W + 1) * sizeof(float); }

extern "C" int vt_stat_gate_forward(const void* g, int64_t ldg, const float* w2, const float* b2, const float* z, int64_t M, int32_t W, int32_t d,
                                    const int32_t* levels_host, int32_t mode, uint64_t seed, const float* mask_in, float* probs, float* mask,
                                    float* codes, int32_t* indices, vtStream stream) {
    FsqConsts k;
    if (int rc = check_common("vt_stat_gate_forward", z, M, W, d, levels_host, ldg, k)) return rc;
    VT_CHECK_ARG(g && w2 && b2 && probs && mask, "vt_stat_gate_forward: null g / w2 / b2 / probs / mask");
    VT_CHECK_ARG(!z || codes, "vt_stat_gate_forward: z given without codes");
    VT_CHECK_ARG(mode >= VT_STAT_SAMPLE && mode <= VT_STAT_FORCED, "vt_stat_gate_forward: unknown mode %d", mode);
    VT_CHECK_ARG(mode != VT_STAT_FORCED || mask_in, "vt_stat_gate_forward: forced mode needs mask_in");
    VT_CHECK_ARG(aligned16(g) && aligned16(w2), "vt_stat_gate_forward: g and w2 must be 16-byte aligned");
    const dim3 grid((unsigned)((M + kRowsPerBlock - 1) / kRowsPerBlock));
    const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
#define VT_STAT_FWD(CH)                                                                                                                   \
    hipLaunchKernelGGL(stat_gate_fwd_kernel<CH>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g, ldg, w2, b2, z, M, k, (int)mode, \
                       lo, hi, mask_in, probs, mask, codes, indices)
    VT_STAT_DISPATCH(W / 128, VT_STAT_FWD)
#undef VT_STAT_FWD
    VT_CHECK_LAUNCH("vt_stat_gate_forward");
    return VT_OK;
}

extern "C" int vt_stat_gate_backward(const float* dcodes, const float* dprobs, const float* dmask, const float* z, const float* mask,
                                     const float* probs, const void* u, const void* g, int64_t ld, const float* w2, int64_t M, int32_t W, int32_t d,
                                     const int32_t* levels_host, int32_t ste, void* dU, float* dz, float* dw2, float* db2, void* workspace,
                                     vtStream stream) {
    FsqConsts k;
    if (int rc = check_common("vt_stat_gate_backward", z, M, W, d, levels_host, ld, k)) return rc;
    VT_CHECK_ARG(mask && probs && u && g && w2 && dU && dw2 && db2 && workspace, "vt_stat_gate_backward: null pointer");
    VT_CHECK_ARG(!z || (dcodes && dz), "vt_stat_gate_backward: z given without dcodes / dz");
    VT_CHECK_ARG(aligned16(u) && aligned16(g) && aligned16(dU) && aligned16(w2), "vt_stat_gate_backward: u, g, dU and w2 must be 16-byte aligned");
    const int64_t groups = (M + kRowsPerBlock - 1) / kRowsPerBlock;
    const int64_t per = (groups + kMaxBwdBlocks - 1) / kMaxBwdBlocks * kRowsPerBlock;   // rows per workgroup, a multiple of 16
    const int nblk = (int)((M + per - 1) / per);
    float* part = (float*)workspace;
#define VT_STAT_BWD(CH)                                                                                                                       \
    hipLaunchKernelGGL(stat_gate_bwd_kernel<CH>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, dcodes, dprobs, dmask, z, mask, probs,        \
                       (const bf16_t*)u, (const bf16_t*)g, ld, w2, M, per, k, (int)(ste != 0), (bf16_t*)dU, dz, part)
    VT_STAT_DISPATCH(W / 128, VT_STAT_BWD)
#undef VT_STAT_BWD
    VT_CHECK_LAUNCH("vt_stat_gate_backward");
    hipLaunchKernelGGL(stat_partial_sum_kernel, dim3((unsigned)((W + 1 + 15) / 16)), dim3(256), 0, (hipStream_t)stream, part, nblk, (int)W, dw2, db2);
    VT_CHECK_LAUNCH("vt_stat_gate_backward");
    return VT_OK;
}
