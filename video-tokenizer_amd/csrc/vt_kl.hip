// Diagonal-Gaussian KL bottleneck ('skl', models/bottleneck.py:36-64 DiagonalGaussianDistribution, :347-375
// SummedKLDivergenceRegularizer) for gfx950: the part of Bottleneck.forward between in_linear and out_linear, and its backward.
//
// Forward, per row r of z (fp32, 2d columns interleaved: mean_c = z[r, 2c], logvar_c = clamp(z[r, 2c + 1], -30, 20)):
//   eps    = counter-hash Gaussian of (seed, device counter, element index r * d + c): Box-Muller on pairs of elements
//   sample = mean + exp(0.5 logvar) * eps           -> fp32 [M, d] and its bf16 copy, zero-padded to ldp columns (out_linear operand)
//   loss   = sum_{r,c} 0.5 (mean^2 + exp(logvar) - 1 - logvar) / batch
// The loss is summed in a fixed order: per-workgroup partials (shuffle tree, then the four waves in order) into the workspace, then
// one workgroup adds them in index order.  No float atomics: bit-identical run to run.
// Backward (g = dL/dsample, k = dL/dloss / batch):
//   dmean = g + g_mean + k mean,   dlogvar_raw = [-30 <= z_odd <= 20] (0.5 g eps std + 0.5 k (var - 1))
//   -> dz fp32 [M, 2d] and / or its bf16 copy zero-padded to ldp columns (in_linear dgrad / wgrad operand).
//
// HBM-bound row passes over a few MB.  Each lane owns 4 latent channels in the forward (two 16-byte z loads, 16-byte mean / sample /
// noise stores, an 8-byte bf16 store) and 2 in the backward (a 16-byte z load, 8-byte g / eps loads, a 16-byte dz store, an 8-byte
// bf16 store); lanes past the last channel write the zero pad of the bf16 row.
#include "vt_common.h"
#include "vt_kl_device.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

constexpr int kThreads = 256;
constexpr int kMaxParts = VT_KL_WORKSPACE_BYTES / 4;   // partial sums of the forward's loss (one per workgroup)

__device__ __forceinline__ bf16x4 zero_bf16x4() {
    const bf16_t z = f2bf(0.0f);
    return bf16x4{z, z, z, z};
}

// fixed-order sum over the workgroup (4 waves); result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
    if (threadIdx.x == 0) t = ((red[0] + red[1]) + red[2]) + red[3];
    return t;
}

__global__ __launch_bounds__(kThreads) void kl_fwd_kernel(const float* __restrict__ z, int64_t ldz, int64_t M, int d, int per_row,
                                                          unsigned seed_lo, unsigned seed_hi, const uint32_t* __restrict__ seed_ctr,
                                                          float* __restrict__ mean, float* __restrict__ sample, bf16_t* __restrict__ rzp,
                                                          int64_t ldp, float* __restrict__ noise, float* __restrict__ part) {
    __shared__ float red[kThreads / 64];
    if (seed_ctr) seed_lo += *seed_ctr;       // per-call counter in device memory (hipGraph replays), as vt_vq_forward_ctr
    const unsigned base = pcg_hash(seed_lo);
    const int64_t items = M * per_row;
    float acc = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
        const int64_t r = i / per_row;
        const int c = 4 * (int)(i - r * per_row);
        if (c < d) {
            const f32x4* zr = (const f32x4*)(z + r * ldz + 2 * c);
            const f32x4 a = ld_stream_any(zr), b = ld_stream_any(zr + 1);   // (m0, lv0, m1, lv1), (m2, lv2, m3, lv3)
            const unsigned pair = (unsigned)((r * d + c) >> 1);
            float e0, e1, e2, e3, s0, s1, s2, s3;
            vtkl::gauss2(base, seed_hi, pair, e0, e1);
            vtkl::gauss2(base, seed_hi, pair + 1, e2, e3);
            const f32x4 m = {a[0], a[2], b[0], b[2]};
            float kl = vtkl::forward1(a[0], a[1], e0, s0);
            kl += vtkl::forward1(a[2], a[3], e1, s1);
            kl += vtkl::forward1(b[0], b[1], e2, s2);
            kl += vtkl::forward1(b[2], b[3], e3, s3);
            acc += kl;
            const f32x4 e = {e0, e1, e2, e3}, s = {s0, s1, s2, s3};
            const int64_t o = r * d + c;
            if (mean) *(f32x4*)(mean + o) = m;
            if (sample) *(f32x4*)(sample + o) = s;
            if (noise) *(f32x4*)(noise + o) = e;
            if (rzp) {
                bf16x4 sb;
#pragma unroll
                for (int k = 0; k < 4; ++k) sb[k] = f2bf(s[k]);
                *(bf16x4*)(rzp + r * ldp + c) = sb;
            }
        } else {
            *(bf16x4*)(rzp + r * ldp + c) = zero_bf16x4();   // (c >= d only exists when rzp is given: per_row = ldp / 4)
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void kl_loss_kernel(const float* __restrict__ part, int nparts, float inv_batch, float* __restrict__ loss) {
    __shared__ float red[kThreads / 64];
    float v = 0.0f;
    for (int i = threadIdx.x; i < nparts; i += kThreads) v += part[i];
    const float t = block_sum(v, red);
    if (threadIdx.x == 0) loss[0] = t * inv_batch;
}

__global__ __launch_bounds__(kThreads) void kl_bwd_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ gmean,
                                                          const float* __restrict__ gkl, float inv_batch, const float* __restrict__ z, int64_t ldz,
                                                          const float* __restrict__ noise, int64_t M, int d, int per_row, float* __restrict__ dz,
                                                          bf16_t* __restrict__ dzp, int64_t ldp) {
    const float k = gkl ? gkl[0] * inv_batch : 0.0f;
    const int64_t items = M * per_row;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
        const int64_t r = i / per_row;
        const int q = (int)(i - r * per_row);
        const int c = 2 * q;                  // latent channels c, c + 1 = z columns 4q .. 4q + 3
        if (c < d) {
            const f32x4 zz = ld_stream_any((const f32x4*)(z + r * ldz + 2 * c));
            const f32x2_t e = *(const f32x2_t*)(noise + r * d + c);
            f32x2_t gg = {0.0f, 0.0f}, gm = {0.0f, 0.0f};
            if (g) gg = *(const f32x2_t*)(g + r * ldg + c);
            if (gmean) gm = *(const f32x2_t*)(gmean + r * d + c);
            float dm0, dl0, dm1, dl1;
            vtkl::backward1(zz[0], zz[1], e[0], gg[0], gm[0], k, dm0, dl0);
            vtkl::backward1(zz[2], zz[3], e[1], gg[1], gm[1], k, dm1, dl1);
            const f32x4 o = {dm0, dl0, dm1, dl1};
            if (dz) *(f32x4*)(dz + r * 2 * d + 4 * q) = o;
            if (dzp) {
                const bf16x4 ob = {f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
                *(bf16x4*)(dzp + r * ldp + 4 * q) = ob;
            }
        } else {
            *(bf16x4*)(dzp + r * ldp + 4 * q) = zero_bf16x4();
        }
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline int grid_for(int64_t items, int cap) {
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}

}  // namespace

extern "C" int vt_kl_forward(const float* z, int64_t ldz, int64_t M, int32_t d, int32_t batch, uint64_t seed, const uint32_t* seed_counter,
                             float* mean, float* sample, void* sample_pad_bf16, int64_t ldp, float* noise, float* loss_kl, void* workspace,
                             vtStream stream) {
    VT_CHECK_ARG(z && loss_kl && workspace, "vt_kl_forward: z, loss_kl and workspace are required");
    VT_CHECK_ARG(M > 0 && batch > 0 && M % batch == 0, "vt_kl_forward: M=%lld rows must be a positive multiple of batch=%d", (long long)M, batch);
    VT_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 256, "vt_kl_forward: d=%d unsupported (multiple of 4, <= 256)", d);
    VT_CHECK_ARG(ldz >= 2 * d && ldz % 4 == 0 && aligned(z, 16), "vt_kl_forward: z must be 16-byte aligned with ldz >= 2d, ldz %% 4 == 0");
    VT_CHECK_ARG(aligned(mean, 16) && aligned(sample, 16) && aligned(noise, 16) && aligned(workspace, 4),
                 "vt_kl_forward: mean / sample / noise must be 16-byte aligned");
    VT_CHECK_ARG(!sample_pad_bf16 || (ldp >= d && ldp % 4 == 0 && aligned(sample_pad_bf16, 8)),
                 "vt_kl_forward: the bf16 sample needs ldp >= d, ldp %% 4 == 0 and 8-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    const int per_row = sample_pad_bf16 ? (int)(ldp / 4) : d / 4;
    const int grid = grid_for(M * per_row, kMaxParts);
    hipLaunchKernelGGL(kl_fwd_kernel, dim3(grid), dim3(kThreads), 0, s, z, ldz, M, d, per_row, (unsigned)(seed & 0xffffffffu),
                       (unsigned)(seed >> 32), seed_counter, mean, sample, (bf16_t*)sample_pad_bf16, ldp, noise, (float*)workspace);
    hipLaunchKernelGGL(kl_loss_kernel, dim3(1), dim3(kThreads), 0, s, (const float*)workspace, grid, 1.0f / (float)batch, loss_kl);
    VT_CHECK_LAUNCH("vt_kl_forward");
    return VT_OK;
}

extern "C" int vt_kl_backward(const float* g_sample, int64_t ldg, const float* g_mean, const float* gkl, const float* z, int64_t ldz,
                              const float* noise, int64_t M, int32_t d, int32_t batch, float* dz, void* dz_pad_bf16, int64_t ldp, vtStream stream) {
    VT_CHECK_ARG(z && noise && (dz || dz_pad_bf16), "vt_kl_backward: z, noise and an output (dz or dz_pad_bf16) are required");
    VT_CHECK_ARG(M > 0 && batch > 0 && M % batch == 0, "vt_kl_backward: M=%lld rows must be a positive multiple of batch=%d", (long long)M, batch);
    VT_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 256, "vt_kl_backward: d=%d unsupported (multiple of 4, <= 256)", d);
    VT_CHECK_ARG(ldz >= 2 * d && ldz % 4 == 0 && aligned(z, 16), "vt_kl_backward: z must be 16-byte aligned with ldz >= 2d, ldz %% 4 == 0");
    VT_CHECK_ARG(!g_sample || (ldg >= d && ldg % 2 == 0 && aligned(g_sample, 8)), "vt_kl_backward: g_sample needs ldg >= d, ldg %% 2 == 0, 8-byte alignment");
    VT_CHECK_ARG(aligned(g_mean, 8) && aligned(noise, 16) && aligned(dz, 16) && aligned(gkl, 4), "vt_kl_backward: misaligned g_mean / noise / dz");
    VT_CHECK_ARG(!dz_pad_bf16 || (ldp >= 2 * d && ldp % 4 == 0 && aligned(dz_pad_bf16, 8)),
                 "vt_kl_backward: the bf16 dz needs ldp >= 2d, ldp %% 4 == 0 and 8-byte alignment");
    const int per_row = dz_pad_bf16 ? (int)(ldp / 4) : d / 2;
    const int grid = grid_for(M * per_row, 2048);
    hipLaunchKernelGGL(kl_bwd_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g_sample, ldg, g_mean, gkl, 1.0f / (float)batch, z, ldz,
                       noise, M, d, per_row, dz, (bf16_t*)dz_pad_bf16, ldp);
    VT_CHECK_LAUNCH("vt_kl_backward");
    return VT_OK;
}
