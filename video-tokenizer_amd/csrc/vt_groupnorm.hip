// GroupNorm(G, C, eps) with an optional fused swish over bf16 channels-last activations [B, P, C] (P = T*H*W positions of one clip): the
// `Normalize` + `nonlinearity` pair of the reference's 3D ResNet ends (models/model_cnnvit/base/cnnvit.py:5-10).
//
// Statistics are per (clip, group) over C/G channels x P positions, fp32 from the bf16 input, in two passes: the mean first, then the mean of
// squared deviations from it, so a mean far above the standard deviation costs no bits.  A clip is cut into chunks of positions, one workgroup
// each (at 32 channels and 262 144 positions a group has 524 288 elements); every workgroup re-adds the chunk partials of its clip in chunk
// order, so all of them hold the same mean / rstd bits and no extra launch sits between the passes.  No atomics; every sum has a fixed order.
//   forward : sum pass, deviation pass, apply pass (y = (x - mean) rstd gamma + beta, z = y sigmoid(y) if swish; rounded to bf16 once)
//   backward: partial pass (per chunk and channel: sum g, sum g xhat; g = dz dz/dy), apply pass (dx), and a small pass for dgamma / dbeta.
// A thread owns 8 consecutive channels (16 bytes) of a position; C/8 threads cover a position, 256 / (C/8) positions are in flight per workgroup.
#include "vt_common.h"

namespace {

constexpr int GN_CHUNK_ELEMS = 32768;   // elements (positions x C) of a chunk, unless that gives more than GN_MAX_CHUNKS chunks per clip
constexpr int GN_MAX_CHUNKS = 256;

struct GNGeom {
    int B, C, G, cg, lpp, ppi, nchunk, swish;
    int64_t P, chunk_pos;
    float eps, inv_n;
};

// per-channel sums of the workgroup: every thread's acc[8] (channels 8 * (tid % lpp) ..) -> chan[C] in LDS, added in slot order
__device__ __forceinline__ void block_channel_sums(const float (&acc)[8], float* red, float* chan, const GNGeom& g, int tid) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid * 8 + j] = acc[j];
    __syncthreads();
    for (int c = tid; c < g.C; c += 256) {
        float s = 0.f;
        for (int p = 0; p < g.ppi; ++p) s += red[(p * g.lpp + (c >> 3)) * 8 + (c & 7)];
        chan[c] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void chunk_range(const GNGeom& g, int chunk, int64_t& p0, int64_t& p1) {
    p0 = chunk * g.chunk_pos;
    p1 = p0 + g.chunk_pos < g.P ? p0 + g.chunk_pos : g.P;
}

__device__ __forceinline__ float sigmoidf_(float y) { return 1.0f / (1.0f + __expf(-y)); }

// pass 1 (DEV = false): part[(b, chunk, g)] = sum x.  pass 2 (DEV = true): mean from the pass-1 partials, part2 = sum (x - mean)^2.
template <bool DEV>
__global__ __launch_bounds__(256) void gn_stats_kernel(const bf16_t* __restrict__ x, const float* __restrict__ part1, float* __restrict__ part_out,
                                                       const GNGeom g) {
    __shared__ float red[256 * 8];
    __shared__ float chan[1024];
    __shared__ float smean[1024];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    if (DEV) {
        for (int gi = tid; gi < g.G; gi += 256) {
            float s = 0.f;
            for (int k = 0; k < g.nchunk; ++k) s += part1[((int64_t)b * g.nchunk + k) * g.G + gi];
            smean[gi] = s * g.inv_n;
        }
        __syncthreads();
    }
    const int slot = tid / g.lpp, lp = tid % g.lpp, c0 = lp * 8;
    float m[8], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = DEV ? smean[(c0 + j) / g.cg] : 0.f;
    int64_t p0, p1;
    chunk_range(g, chunk, p0, p1);
    if (slot < g.ppi) {
        for (int64_t p = p0 + slot; p < p1; p += g.ppi) {
            const bf16x8 v = *(const bf16x8*)(x + ((int64_t)b * g.P + p) * g.C + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = bf2f(v[j]) - m[j];
                acc[j] += DEV ? d * d : d;
            }
        }
    }
    block_channel_sums(acc, red, chan, g, tid);
    for (int gi = tid; gi < g.G; gi += 256) {
        float s = 0.f;
        for (int j = 0; j < g.cg; ++j) s += chan[gi * g.cg + j];
        part_out[((int64_t)b * g.nchunk + chunk) * g.G + gi] = s;
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ part1, const float* __restrict__ part2, bf16_t* __restrict__ y,
                                                       float* __restrict__ mean, float* __restrict__ rstd, const GNGeom g) {
    __shared__ float smean[1024];
    __shared__ float srstd[1024];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    for (int gi = tid; gi < g.G; gi += 256) {
        float s = 0.f, s2 = 0.f;
        for (int k = 0; k < g.nchunk; ++k) s += part1[((int64_t)b * g.nchunk + k) * g.G + gi];
        for (int k = 0; k < g.nchunk; ++k) s2 += part2[((int64_t)b * g.nchunk + k) * g.G + gi];
        const float mu = s * g.inv_n, rs = 1.0f / sqrtf(s2 * g.inv_n + g.eps);
        smean[gi] = mu, srstd[gi] = rs;
        if (chunk == 0) mean[b * g.G + gi] = mu, rstd[b * g.G + gi] = rs;
    }
    __syncthreads();
    const int slot = tid / g.lpp, lp = tid % g.lpp, c0 = lp * 8;
    if (slot >= g.ppi) return;
    float mu[8], rs[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) mu[j] = smean[(c0 + j) / g.cg], rs[j] = srstd[(c0 + j) / g.cg], ga[j] = gamma[c0 + j], be[j] = beta[c0 + j];
    int64_t p0, p1;
    chunk_range(g, chunk, p0, p1);
    for (int64_t p = p0 + slot; p < p1; p += g.ppi) {
        const int64_t off = ((int64_t)b * g.P + p) * g.C + c0;
        const bf16x8 v = *(const bf16x8*)(x + off);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = (bf2f(v[j]) - mu[j]) * rs[j] * ga[j] + be[j];
            if (g.swish) t = t * sigmoidf_(t);
            o[j] = f2bf(t);
        }
        *(bf16x8*)(y + off) = o;
    }
}

// g = dz * dz/dy and xhat of one element
__device__ __forceinline__ void gn_grad_terms(float xv, float dz, float mu, float rs, float ga, float be, int swish, float& gy, float& xhat) {
    xhat = (xv - mu) * rs;
    gy = dz;
    if (swish) {
        const float t = xhat * ga + be, s = sigmoidf_(t);
        gy = dz * (s * (1.0f + t * (1.0f - s)));
    }
}

// partb[(b, chunk)][0][c] = sum g, [1][c] = sum g xhat over the chunk
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ partb, const GNGeom g) {
    __shared__ float red[256 * 8];
    __shared__ float chan[1024];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    const int slot = tid / g.lpp, lp = tid % g.lpp, c0 = lp * 8;
    float a0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (slot < g.ppi) {
        float mu[8], rs[8], ga[8], be[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int gi = (c0 + j) / g.cg;
            mu[j] = mean[b * g.G + gi], rs[j] = rstd[b * g.G + gi], ga[j] = gamma[c0 + j], be[j] = beta[c0 + j];
        }
        int64_t p0, p1;
        chunk_range(g, chunk, p0, p1);
        for (int64_t p = p0 + slot; p < p1; p += g.ppi) {
            const int64_t off = ((int64_t)b * g.P + p) * g.C + c0;
            const bf16x8 xv = *(const bf16x8*)(x + off), dv = *(const bf16x8*)(dz + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float gy, xhat;
                gn_grad_terms(bf2f(xv[j]), bf2f(dv[j]), mu[j], rs[j], ga[j], be[j], g.swish, gy, xhat);
                a0[j] += gy, a1[j] += gy * xhat;
            }
        }
    }
    float* dst = partb + ((int64_t)b * g.nchunk + chunk) * 2 * g.C;
    block_channel_sums(a0, red, chan, g, tid);
    for (int c = tid; c < g.C; c += 256) dst[c] = chan[c];
    block_channel_sums(a1, red, chan, g, tid);
    for (int c = tid; c < g.C; c += 256) dst[g.C + c] = chan[c];
}

__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ partb, bf16_t* __restrict__ dx, const GNGeom g) {
    __shared__ float chA[1024];
    __shared__ float chB[1024];
    __shared__ float sm1[1024];
    __shared__ float sm2[1024];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    for (int c = tid; c < g.C; c += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int k = 0; k < g.nchunk; ++k) {
            const float* src = partb + ((int64_t)b * g.nchunk + k) * 2 * g.C;
            s0 += src[c], s1 += src[g.C + c];
        }
        chA[c] = s0 * gamma[c], chB[c] = s1 * gamma[c];
    }
    __syncthreads();
    for (int gi = tid; gi < g.G; gi += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int j = 0; j < g.cg; ++j) s0 += chA[gi * g.cg + j], s1 += chB[gi * g.cg + j];
        sm1[gi] = s0 * g.inv_n, sm2[gi] = s1 * g.inv_n;
    }
    __syncthreads();
    const int slot = tid / g.lpp, lp = tid % g.lpp, c0 = lp * 8;
    if (slot >= g.ppi) return;
    float mu[8], rs[8], ga[8], be[8], m1[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int gi = (c0 + j) / g.cg;
        mu[j] = mean[b * g.G + gi], rs[j] = rstd[b * g.G + gi], ga[j] = gamma[c0 + j], be[j] = beta[c0 + j], m1[j] = sm1[gi], m2[j] = sm2[gi];
    }
    int64_t p0, p1;
    chunk_range(g, chunk, p0, p1);
    for (int64_t p = p0 + slot; p < p1; p += g.ppi) {
        const int64_t off = ((int64_t)b * g.P + p) * g.C + c0;
        const bf16x8 xv = *(const bf16x8*)(x + off), dv = *(const bf16x8*)(dz + off);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float gy, xhat;
            gn_grad_terms(bf2f(xv[j]), bf2f(dv[j]), mu[j], rs[j], ga[j], be[j], g.swish, gy, xhat);
            o[j] = f2bf(rs[j] * (gy * ga[j] - m1[j] - xhat * m2[j]));
        }
        *(bf16x8*)(dx + off) = o;
    }
}

// dbeta[c] = sum over clips and chunks of sum g, dgamma[c] = the same of sum g xhat, in (clip, chunk) order
__global__ __launch_bounds__(256) void gn_bwd_params_kernel(const float* __restrict__ partb, int nslab, int C, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < nslab; ++k) s0 += partb[(int64_t)k * 2 * C + c], s1 += partb[(int64_t)k * 2 * C + C + c];
    dbeta[c] = s0, dgamma[c] = s1;
}

int make_geom(const char* who, GNGeom& g, int B, int64_t P, int C, int G, float eps, int swish) {
    VT_CHECK_ARG(B > 0 && B <= 65535, "%s: B=%d outside 1..65535", who, B);
    VT_CHECK_ARG(P > 0 && P <= 0x7fffffff, "%s: P=%lld outside 1..2^31-1", who, (long long)P);
    VT_CHECK_ARG(C > 0 && C % 16 == 0 && C <= 1024, "%s: C=%d must be a multiple of 16 in 16..1024", who, C);
    VT_CHECK_ARG(G > 0 && C % G == 0, "%s: G=%d does not divide C=%d", who, G, C);
    VT_CHECK_ARG(eps > 0.f, "%s: eps=%g must be positive", who, (double)eps);
    VT_CHECK_ARG(swish == 0 || swish == 1, "%s: swish=%d is neither 0 nor 1", who, swish);
    g.B = B, g.C = C, g.G = G, g.cg = C / G, g.lpp = C / 8, g.ppi = 256 / g.lpp, g.swish = swish, g.P = P, g.eps = eps;
    int64_t cp = GN_CHUNK_ELEMS / C, floor_cp = (P + GN_MAX_CHUNKS - 1) / GN_MAX_CHUNKS;
    g.chunk_pos = cp > floor_cp ? cp : floor_cp;
    g.nchunk = (int)((P + g.chunk_pos - 1) / g.chunk_pos);
    g.inv_n = (float)(1.0 / ((double)P * g.cg));
    return VT_OK;
}

size_t ws_bytes(const GNGeom& g) {
    const size_t fwd = (size_t)2 * g.B * g.nchunk * g.G, bwd = (size_t)2 * g.B * g.nchunk * g.C;
    return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

}  // namespace

extern "C" size_t vt_groupnorm_workspace_bytes(int32_t B, int64_t P, int32_t C, int32_t G) {
    GNGeom g;
    if (make_geom("vt_groupnorm_workspace_bytes", g, B, P, C, G, 1.f, 0) != VT_OK) return 0;
    return ws_bytes(g);
}

extern "C" int vt_groupnorm_fwd(const void* x_bf16, const float* gamma, const float* beta, float eps, int32_t B, int64_t P, int32_t C, int32_t G,
                                int32_t swish, void* y_bf16, float* mean, float* rstd, void* workspace, vtStream stream) {
    const char* who = "vt_groupnorm_fwd";
    VT_CHECK_ARG(x_bf16 && gamma && beta && y_bf16 && mean && rstd && workspace, "%s: x, gamma, beta, y, mean, rstd or workspace is null", who);
    VT_CHECK_ARG(aligned16(x_bf16) && aligned16(y_bf16) && aligned16(workspace), "%s: a tensor is not 16-byte aligned (x %p, y %p, workspace %p)", who, x_bf16,
                 y_bf16, workspace);
    GNGeom g;
    TRY(make_geom(who, g, B, P, C, G, eps, swish));
    float* part1 = (float*)workspace;
    float* part2 = part1 + (size_t)B * g.nchunk * G;
    const dim3 grid(g.nchunk, B);
    hipLaunchKernelGGL(gn_stats_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x_bf16, (const float*)nullptr, part1, g);
    VT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(gn_stats_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x_bf16, (const float*)part1, part2, g);
    VT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x_bf16, gamma, beta, (const float*)part1, (const float*)part2,
                       (bf16_t*)y_bf16, mean, rstd, g);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_groupnorm_bwd(const void* dz_bf16, const void* x_bf16, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                int32_t B, int64_t P, int32_t C, int32_t G, int32_t swish, void* dx_bf16, float* dgamma, float* dbeta, void* workspace,
                                vtStream stream) {
    const char* who = "vt_groupnorm_bwd";
    VT_CHECK_ARG(dz_bf16 && x_bf16 && gamma && beta && mean && rstd && dx_bf16 && dgamma && dbeta && workspace,
                 "%s: dz, x, gamma, beta, mean, rstd, dx, dgamma, dbeta or workspace is null", who);
    VT_CHECK_ARG(aligned16(dz_bf16) && aligned16(x_bf16) && aligned16(dx_bf16) && aligned16(workspace),
                 "%s: a tensor is not 16-byte aligned (dz %p, x %p, dx %p, workspace %p)", who, dz_bf16, x_bf16, dx_bf16, workspace);
    GNGeom g;
    TRY(make_geom(who, g, B, P, C, G, 1.f, swish));
    float* partb = (float*)workspace;
    const dim3 grid(g.nchunk, B);
    hipLaunchKernelGGL(gn_bwd_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dz_bf16, (const bf16_t*)x_bf16, gamma, beta, mean, rstd,
                       partb, g);
    VT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dz_bf16, (const bf16_t*)x_bf16, gamma, beta, mean, rstd,
                       (const float*)partb, (bf16_t*)dx_bf16, g);
    VT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)partb, B * g.nchunk, C, dgamma, dbeta);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
