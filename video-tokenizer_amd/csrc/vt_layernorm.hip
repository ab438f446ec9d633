// LayerNorm forward/backward for gfx950 (fp32 statistics, bf16 output for the following MFMA GEMM).  HBM-bound: one wave (64 lanes)
// owns one row; each lane moves 16 B per access (8 B at the widths 128 and 384).
#include <type_traits>

#include "vt_common.h"

namespace {

// per-lane vector width of the LayerNorm kernels: a row is 64 lanes x VEC floats x V pieces
template <int VEC> struct LnVec;
template <> struct LnVec<4> { typedef f32x4 F; typedef bf16x4 H; };
template <> struct LnVec<2> { typedef __attribute__((ext_vector_type(2))) float F; typedef bf16x2 H; };

// ------------------------------------------------------------------------------------------------
// LayerNorm forward: y = (x - mean) * rstd * gamma + beta, y in bf16, stats saved in fp32
// ------------------------------------------------------------------------------------------------
template <int V, int VEC>  // dim = 64 * VEC * V: 256..1024 with 16-B accesses, 128 / 384 (the discriminator's width) with 8-B
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, RowMap xmap, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, int64_t rows,
                                                      bf16_t* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd) {
    typedef typename LnVec<VEC>::F F;
    typedef typename LnVec<VEC>::H Hh;
    constexpr int DIM = 64 * VEC * V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    F g[V], b[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        g[i] = *(const F*)(gamma + (i * 64 + lane) * VEC);
        b[i] = *(const F*)(beta + (i * 64 + lane) * VEC);
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const float* xr = x + xmap(row) * DIM;
        F v[V];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            v[i] = *(const F*)(xr + (i * 64 + lane) * VEC);
            if constexpr (VEC == 4) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            else s += v[i][0] + v[i][1];
        }
        const float mu = wave_sum(s) * (1.0f / DIM);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int r = 0; r < VEC; ++r) {
                const float d = v[i][r] - mu;
                q += d * d;
            }
        const float var = wave_sum(q) * (1.0f / DIM);
        const float rs = 1.0f / sqrtf(var + eps);
        bf16_t* yr = y + row * DIM;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            Hh o;
#pragma unroll
            for (int r = 0; r < VEC; ++r) o[r] = f2bf((v[i][r] - mu) * rs * g[i][r] + b[i][r]);
            *(Hh*)(yr + (i * 64 + lane) * VEC) = o;
        }
        if (lane == 0) {
            mean[row] = mu;
            rstd[row] = rs;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward (+ residual-stream add).  With xh = (x-mean)*rstd, a = dy*gamma:
//   dx = rstd * (a - mean(a) - xh * mean(a*xh));   out = dres + dx  (fp32, and a bf16 copy)
// Column partials per workgroup: dgamma = sum dy*xh, dbeta = sum dy, dxsum = sum out (the bias
// gradient of the Linear whose output this residual stream is).  partial layout [grid][3][DIM].
// ------------------------------------------------------------------------------------------------
template <int V, int VEC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x, RowMap xmap,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ dres, int64_t rows,
                                                      float* __restrict__ dx, bf16_t* __restrict__ dxb, float* __restrict__ partial) {
    typedef typename LnVec<VEC>::F F;
    typedef typename LnVec<VEC>::H Hh;
    constexpr int DIM = 64 * VEC * V;
    __shared__ float red[4][DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    F g[V], ag[V], ab[V], as[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        g[i] = *(const F*)(gamma + (i * 64 + lane) * VEC);
#pragma unroll
        for (int r = 0; r < VEC; ++r) ag[i][r] = ab[i][r] = as[i][r] = 0.f;
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t pr = xmap(row);
        const float mu = mean[row], rs = rstd[row];
        F xh[V], a[V], rv[V];
        float s1 = 0.f, s2 = 0.f;
        if (dres) {   // issued with the row's other loads: one more 3 KB per wave in flight while the two row sums are taken
#pragma unroll
            for (int i = 0; i < V; ++i) rv[i] = *(const F*)(dres + pr * DIM + (i * 64 + lane) * VEC);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const F xv = *(const F*)(x + pr * DIM + (i * 64 + lane) * VEC);
            const Hh dv = *(const Hh*)(dy + row * DIM + (i * 64 + lane) * VEC);
#pragma unroll
            for (int r = 0; r < VEC; ++r) {
                const float d = bf2f(dv[r]);
                xh[i][r] = (xv[r] - mu) * rs;
                a[i][r] = d * g[i][r];
                s1 += a[i][r];
                s2 += a[i][r] * xh[i][r];
                ag[i][r] += d * xh[i][r];
                ab[i][r] += d;
            }
        }
        const float m1 = wave_sum(s1) * (1.0f / DIM);
        const float m2 = wave_sum(s2) * (1.0f / DIM);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            F o;
#pragma unroll
            for (int r = 0; r < VEC; ++r) o[r] = rs * (a[i][r] - m1 - xh[i][r] * m2);
            if (dres) {
#pragma unroll
                for (int r = 0; r < VEC; ++r) o[r] += rv[i][r];
            }
#pragma unroll
            for (int r = 0; r < VEC; ++r) as[i][r] += o[r];
            *(F*)(dx + pr * DIM + (i * 64 + lane) * VEC) = o;
            if (dxb) {
                Hh ob;
#pragma unroll
                for (int r = 0; r < VEC; ++r) ob[r] = f2bf(o[r]);
                *(Hh*)(dxb + pr * DIM + (i * 64 + lane) * VEC) = ob;
            }
        }
    }
    // cross-wave reduction of the three column partials, one at a time through LDS
    float* out = partial + (int64_t)blockIdx.x * 3 * DIM;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < V; ++i) *(F*)(&red[wave][(i * 64 + lane) * VEC]) = (w == 0 ? ag[i] : (w == 1 ? ab[i] : as[i]));
        __syncthreads();
        for (int c = threadIdx.x; c < DIM; c += 256) out[w * DIM + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// the supported widths: X(dim, V, VEC) with dim = 64 * VEC * V
#define LN_WIDTHS(X) X(128, 1, 2) X(256, 1, 4) X(384, 3, 2) X(512, 2, 4) X(768, 3, 4) X(1024, 4, 4)

bool ln_width_ok(int dim) {
#define X(DIM, V, VEC) if (dim == DIM) return true;
    LN_WIDTHS(X)
#undef X
    return false;
}

// launch(std::integral_constant<int, V>, std::integral_constant<int, VEC>) for the table's entry of dim (dim has passed ln_width_ok)
template <typename Launch>
void at_width(int dim, Launch launch) {
    switch (dim) {
#define X(DIM, V, VEC) case DIM: launch(std::integral_constant<int, V>(), std::integral_constant<int, VEC>()); break;
        LN_WIDTHS(X)
#undef X
    }
}

}  // namespace

extern "C" int vt_layernorm_fwd(const float* x, vtRowMap xmap, const float* gamma, const float* beta, float eps, int64_t rows,
                                int32_t dim, void* y_bf16, float* mean, float* rstd, vtStream stream) {
    VT_CHECK_ARG(x && gamma && beta && y_bf16 && mean && rstd, "vt_layernorm_fwd: null pointer");
    VT_CHECK_ARG(rows > 0 && ln_width_ok(dim), "vt_layernorm_fwd: dim=%d must be 128, 256, 384, 512, 768 or 1024", dim);
    const int grid = (int)((rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048);
    at_width(dim, [&](auto v, auto vec) {
        hipLaunchKernelGGL((ln_fwd_kernel<decltype(v)::value, decltype(vec)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, to_map(xmap), gamma,
                           beta, eps, rows, (bf16_t*)y_bf16, mean, rstd);
    });
    VT_CHECK_LAUNCH("vt_layernorm_fwd");
    return VT_OK;
}

#define VT_LN_BWD_GRID 512
extern "C" size_t vt_layernorm_bwd_workspace_bytes(int32_t dim) { return (size_t)VT_LN_BWD_GRID * 3 * dim * sizeof(float); }

int vt_layernorm_bwd_partials(const void* dy_bf16, const float* x, vtRowMap xmap, const float* gamma, const float* mean, const float* rstd,
                              const float* dres, int64_t rows, int32_t dim, float* dx, void* dx_bf16, float* part, int* nslab, vtStream stream) {
    VT_CHECK_ARG(dy_bf16 && x && gamma && mean && rstd && dx && part, "vt_layernorm_bwd: null pointer");
    VT_CHECK_ARG(rows > 0 && ln_width_ok(dim), "vt_layernorm_bwd: dim=%d must be 128, 256, 384, 512, 768 or 1024", dim);
    const int grid = (int)((rows + 3) / 4 < VT_LN_BWD_GRID ? (rows + 3) / 4 : VT_LN_BWD_GRID);
    at_width(dim, [&](auto v, auto vec) {
        hipLaunchKernelGGL((ln_bwd_kernel<decltype(v)::value, decltype(vec)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy_bf16, x,
                           to_map(xmap), gamma, mean, rstd, dres, rows, dx, (bf16_t*)dx_bf16, part);
    });
    VT_CHECK_LAUNCH("vt_layernorm_bwd");
    *nslab = grid;
    return VT_OK;
}

extern "C" int vt_layernorm_bwd(const void* dy_bf16, const float* x, vtRowMap xmap, const float* gamma, const float* mean,
                                const float* rstd, const float* dres, int64_t rows, int32_t dim, float* dx, void* dx_bf16,
                                float* dgamma, float* dbeta, float* dxsum, void* workspace, vtStream stream) {
    VT_CHECK_ARG(dgamma && dbeta && workspace, "vt_layernorm_bwd: null pointer");
    int grid = 0;
    TRY(vt_layernorm_bwd_partials(dy_bf16, x, xmap, gamma, mean, rstd, dres, rows, dim, dx, dx_bf16, (float*)workspace, &grid, stream));
    return vt_reduce_partials("vt_layernorm_bwd/reduce", (const float*)workspace, grid, (int64_t)3 * dim, dim, dgamma, dbeta, dxsum, stream);
}
