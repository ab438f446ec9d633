// Fused epilogues of the NT GEMM, shared by the 128x128 and 192x192 tile kernels.  One call handles the four
// consecutive output columns n..n+3 of output row m that one lane owns after the swapped (B x A) MFMA.
// Interior tiles (n + 3 < N) take the vector path: 16-B loads of bias / residual / rowmod / aux, one 8- or
// 16-B store per output.  Only the last, ragged column group of a matrix takes the scalar path.
#pragma once
#include <type_traits>

#include "vt_common.h"

// every epilogue code, for the loops that prepare each kernel instantiation
constexpr int VT_EPI_ALL[] = {VT_EPI_BF16, VT_EPI_BF16_GELU, VT_EPI_F32, VT_EPI_BF16_DGELU, VT_EPI_BF16_GELU_GRAD, VT_EPI_BF16_MULAUX};

// gelu'(u) and gelu(u) of four bf16 pre-activations, each pair from one gelu_parts evaluation (VT_EPI_BF16_GELU_GRAD)
__device__ __forceinline__ void gelu_and_grad4(const bf16x4& u, bf16x4& g, bf16x4& dg) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float gf, df;
        gelu_erf_and_grad(bf2f(u[e]), gf, df);
        g[e] = f2bf(gf), dg[e] = f2bf(df);
    }
}
// bf16(h * aux) of four bf16 pairs (VT_EPI_BF16_MULAUX); the fp32 product of two bf16 values is exact
__device__ __forceinline__ bf16x4 mul_aux4(const bf16x4& h, const bf16x4& a) {
    return (bf16x4){f2bf(bf2f(h[0]) * bf2f(a[0])), f2bf(bf2f(h[1]) * bf2f(a[1])), f2bf(bf2f(h[2]) * bf2f(a[2])), f2bf(bf2f(h[3]) * bf2f(a[3]))};
}

// Calls f with the run-time epilogue `epi` as a compile-time constant (std::integral_constant<int, VT_EPI_*>) and returns what it returns.
template <typename F>
static inline int dispatch_epi(int epi, F&& f) {
    switch (epi) {
        case VT_EPI_BF16: return f(std::integral_constant<int, VT_EPI_BF16>{});
        case VT_EPI_BF16_GELU: return f(std::integral_constant<int, VT_EPI_BF16_GELU>{});
        case VT_EPI_F32: return f(std::integral_constant<int, VT_EPI_F32>{});
        case VT_EPI_BF16_DGELU: return f(std::integral_constant<int, VT_EPI_BF16_DGELU>{});
        case VT_EPI_BF16_GELU_GRAD: return f(std::integral_constant<int, VT_EPI_BF16_GELU_GRAD>{});
        case VT_EPI_BF16_MULAUX: return f(std::integral_constant<int, VT_EPI_BF16_MULAUX>{});
        default: vt_set_error("vt_gemm_nt: unknown epilogue %d", epi); return VT_ERR_INVALID;
    }
}

template <int EPI>
__device__ __forceinline__ void nt_epilogue(const vtGemmNT& p, const RowMap& omap, int m, int n, const f32x4& acc4) {
    const int64_t orow = (EPI == VT_EPI_F32) ? omap(m) : (int64_t)m;
    if (n + 3 < p.N) {
        f32x4 v = acc4;
        if (p.bias) v += *(const f32x4*)(p.bias + n);
        if constexpr (EPI == VT_EPI_BF16) {
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        } else if constexpr (EPI == VT_EPI_BF16_GELU) {
            // GELU of the bf16-rounded pre-activation, evaluated in fp32 (autocast order)
            const bf16x4 u = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) = u;
            *(bf16x4*)((bf16_t*)p.out2 + orow * p.ldo2 + n) =
                (bf16x4){f2bf(gelu_erf(bf2f(u[0]))), f2bf(gelu_erf(bf2f(u[1]))), f2bf(gelu_erf(bf2f(u[2]))), f2bf(gelu_erf(bf2f(u[3])))};
        } else if constexpr (EPI == VT_EPI_BF16_DGELU) {
            const bf16x4 uu = *(const bf16x4*)((const bf16_t*)p.aux + (int64_t)m * p.ldaux + n);
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) =
                (bf16x4){f2bf(v[0] * gelu_erf_grad(bf2f(uu[0]))), f2bf(v[1] * gelu_erf_grad(bf2f(uu[1]))),
                         f2bf(v[2] * gelu_erf_grad(bf2f(uu[2]))), f2bf(v[3] * gelu_erf_grad(bf2f(uu[3])))};
        } else if constexpr (EPI == VT_EPI_BF16_GELU_GRAD) {
            bf16x4 g, dg;
            gelu_and_grad4((bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}, g, dg);
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) = dg;
            *(bf16x4*)((bf16_t*)p.out2 + orow * p.ldo2 + n) = g;
        } else if constexpr (EPI == VT_EPI_BF16_MULAUX) {
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) =
                mul_aux4((bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}, *(const bf16x4*)((const bf16_t*)p.aux + (int64_t)m * p.ldaux + n));
        } else {  // VT_EPI_F32
            if (p.round_bf16) v = (f32x4){round_bf16(v[0]), round_bf16(v[1]), round_bf16(v[2]), round_bf16(v[3])};
            if (p.residual) v += *(const f32x4*)(p.residual + orow * p.ldr + n);   // (a streaming load of these 64-B line halves fetches every line twice)
            if (p.rowmod) v += *(const f32x4*)(p.rowmod + (int64_t)(m % p.rowmod_period) * p.N + n);
            if (p.out_scale != 0.f) v *= p.out_scale;
            *(f32x4*)((float*)p.out + orow * p.ldo + n) = v;   // 64-B pieces of a line per instruction: a streaming store would lose the L2's write combining (+45 %)
            if (p.out2) *(bf16x4*)((bf16_t*)p.out2 + orow * p.ldo2 + n) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        }
        return;
    }
    // ragged tail of the matrix (N % 4 != 0 only): scalar
    for (int r = 0; r < 4 && n + r < p.N; ++r) {
        float v = acc4[r] + (p.bias ? p.bias[n + r] : 0.f);
        if constexpr (EPI == VT_EPI_BF16) {
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = f2bf(v);
        } else if constexpr (EPI == VT_EPI_BF16_GELU) {
            const bf16_t u = f2bf(v);
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = u;
            ((bf16_t*)p.out2)[orow * p.ldo2 + n + r] = f2bf(gelu_erf(bf2f(u)));
        } else if constexpr (EPI == VT_EPI_BF16_DGELU) {
            const float u = bf2f(((const bf16_t*)p.aux)[(int64_t)m * p.ldaux + n + r]);
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = f2bf(v * gelu_erf_grad(u));
        } else if constexpr (EPI == VT_EPI_BF16_GELU_GRAD) {
            float gf, df;
            gelu_erf_and_grad(bf2f(f2bf(v)), gf, df);
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = f2bf(df);
            ((bf16_t*)p.out2)[orow * p.ldo2 + n + r] = f2bf(gf);
        } else if constexpr (EPI == VT_EPI_BF16_MULAUX) {
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = f2bf(bf2f(f2bf(v)) * bf2f(((const bf16_t*)p.aux)[(int64_t)m * p.ldaux + n + r]));
        } else {
            if (p.round_bf16) v = round_bf16(v);
            if (p.residual) v += p.residual[orow * p.ldr + n + r];
            if (p.rowmod) v += p.rowmod[(int64_t)(m % p.rowmod_period) * p.N + n + r];
            if (p.out_scale != 0.f) v *= p.out_scale;
            ((float*)p.out)[orow * p.ldo + n + r] = v;
            if (p.out2) ((bf16_t*)p.out2)[orow * p.ldo2 + n + r] = f2bf(v);
        }
    }
}

// Output of the TN kernels: a wave's NI x NJ accumulators start at (row0, col0) of C; after the swapped MFMA acc[i][j][r] =
// C[row0 + i*16 + (lane&15)][col0 + j*16 + (lane>>4)*4 + r].  Rows >= p_lim and columns >= q_lim are not stored; row_perm scatters the rows.
// `p` is taken BY VALUE: its fields are read once, into registers.  Through a reference into the kernel arguments they are re-read after
// every store that might alias them, and gemm_tn_kernel then stops hoisting its staging addresses out of the K loop (5 % slower, measured).
template <int NI, int NJ>
__device__ __forceinline__ void tn_store_acc(const vtGemmTN p, const f32x4 (&acc)[NI][NJ], int row0, int col0, int lane) {
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int pr = row0 + i * 16 + fr;
        if (pr >= p.p_lim) continue;
        const int64_t orow = p.row_perm ? (int64_t)p.row_perm[pr] : (int64_t)pr;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int qc = col0 + j * 16 + fq * 4;
            if (qc >= p.q_lim) continue;
            float* o = p.out + orow * p.ldo + qc;
            if (qc + 3 < p.q_lim && ((p.ldo & 3) == 0)) {
                *(f32x4*)o = acc[i][j];
            } else {
                for (int r = 0; r < 4 && qc + r < p.q_lim; ++r) o[r] = acc[i][j][r];
            }
        }
    }
}
