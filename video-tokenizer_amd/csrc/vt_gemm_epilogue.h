// Fused epilogues of the NT GEMM, shared by the 128x128 and 192x192 tile kernels.  One call handles the four
// consecutive output columns n..n+3 of output row m that one lane owns after the swapped (B x A) MFMA.
// Interior tiles (n + 3 < N) take the vector path: 16-B loads of bias / residual / rowmod / aux, one 8- or
// 16-B store per output.  Only the last, ragged column group of a matrix takes the scalar path.
#pragma once
#include <type_traits>

#include "vt_common.h"

// every epilogue code, for the loops that prepare each kernel instantiation
constexpr int VT_EPI_ALL[] = {VT_EPI_BF16, VT_EPI_BF16_GELU, VT_EPI_F32, VT_EPI_BF16_DGELU, VT_EPI_BF16_GELU_GRAD, VT_EPI_BF16_MULAUX};

template <int N>
using bf16xN = __bf16 __attribute__((ext_vector_type(N)));
__device__ __forceinline__ bf16x4 f2bf4(const f32x4& v) { return (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}; }

// THE per-element arithmetic of the bf16 epilogues: what leaves for h = bf16(acc + bias) -- and `aux`, where the epilogue has one --
// as `out`, and as `out2` under the two epilogues that write one.  Every path of every NT kernel (LDS read-backs, nt_epilogue's vector
// path and scalar tail, the arithmetic arms of the 192x192 kernel's table lookups) calls this, so their outputs agree bit for bit by
// construction.  Values only: every call site keeps its own loads and stores.  (The one exception is VT_EPI_BF16_DGELU in nt_epilogue.)
template <int EPI>
__device__ __forceinline__ void epi_value(bf16_t h, bf16_t aux, bf16_t& out, bf16_t& out2) {
    static_assert(EPI != VT_EPI_F32, "bf16 epilogues");
    if constexpr (EPI == VT_EPI_BF16) {
        out = h;
    } else if constexpr (EPI == VT_EPI_BF16_GELU) {          // GELU of the bf16-rounded pre-activation, evaluated in fp32 (autocast order)
        out = h, out2 = f2bf(gelu_erf(bf2f(h)));
    } else if constexpr (EPI == VT_EPI_BF16_GELU_GRAD) {     // both from one gelu_parts evaluation
        float gf, df;
        gelu_erf_and_grad(bf2f(h), gf, df);
        out = f2bf(df), out2 = f2bf(gf);
    } else if constexpr (EPI == VT_EPI_BF16_MULAUX) {        // the fp32 product of two bf16 values is exact
        out = f2bf(bf2f(h) * bf2f(aux));
    } else {                                                 // VT_EPI_BF16_DGELU: aux = the saved pre-activation
        out = f2bf(bf2f(h) * gelu_erf_grad(bf2f(aux)));
    }
}
template <int EPI, int N>
__device__ __forceinline__ void epi_values(const bf16xN<N>& h, const bf16xN<N>& aux, bf16xN<N>& out, bf16xN<N>& out2) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        bf16_t o, o2 = h[e];   // (o2 defaults to h where the epilogue has no out2: callers ignore it there)
        epi_value<EPI>(h[e], aux[e], o, o2);
        out[e] = o, out2[e] = o2;
    }
}
constexpr bool epi_has_out2(int epi) { return epi == VT_EPI_BF16_GELU || epi == VT_EPI_BF16_GELU_GRAD; }
constexpr bool epi_has_aux(int epi) { return epi == VT_EPI_BF16_DGELU || epi == VT_EPI_BF16_MULAUX; }

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
        if constexpr (EPI == VT_EPI_F32) {
            if (p.round_bf16) v = (f32x4){round_bf16(v[0]), round_bf16(v[1]), round_bf16(v[2]), round_bf16(v[3])};
            if (p.residual) v += *(const f32x4*)(p.residual + orow * p.ldr + n);   // (a streaming load of these 64-B line halves fetches every line twice)
            if (p.rowmod) v += *(const f32x4*)(p.rowmod + (int64_t)(m % p.rowmod_period) * p.N + n);
            if (p.out_scale != 0.f) v *= p.out_scale;
            *(f32x4*)((float*)p.out + orow * p.ldo + n) = v;   // 64-B pieces of a line per instruction: a streaming store would lose the L2's write combining (+45 %)
            if (p.out2) *(bf16x4*)((bf16_t*)p.out2 + orow * p.ldo2 + n) = f2bf4(v);
        } else if constexpr (EPI == VT_EPI_BF16_DGELU) {
            // NOT epi_values: this path multiplies the unrounded fp32 accumulator, the LDS read-backs the bf16-rounded h, so DGELU's bits depend on the path.  Kept as it is
            const bf16x4 uu = *(const bf16x4*)((const bf16_t*)p.aux + (int64_t)m * p.ldaux + n);
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) =
                (bf16x4){f2bf(v[0] * gelu_erf_grad(bf2f(uu[0]))), f2bf(v[1] * gelu_erf_grad(bf2f(uu[1]))),
                         f2bf(v[2] * gelu_erf_grad(bf2f(uu[2]))), f2bf(v[3] * gelu_erf_grad(bf2f(uu[3])))};
        } else {   // round first, then the shared arithmetic
            const bf16x4 h = f2bf4(v);
            bf16x4 aux = h, out, out2;   // (aux: read by VT_EPI_BF16_MULAUX only)
            if constexpr (epi_has_aux(EPI)) aux = *(const bf16x4*)((const bf16_t*)p.aux + (int64_t)m * p.ldaux + n);
            epi_values<EPI, 4>(h, aux, out, out2);
            *(bf16x4*)((bf16_t*)p.out + orow * p.ldo + n) = out;
            if constexpr (epi_has_out2(EPI)) *(bf16x4*)((bf16_t*)p.out2 + orow * p.ldo2 + n) = out2;
        }
        return;
    }
    // ragged tail of the matrix (N % 4 != 0 only): scalar
    for (int r = 0; r < 4 && n + r < p.N; ++r) {
        float v = acc4[r] + (p.bias ? p.bias[n + r] : 0.f);
        if constexpr (EPI == VT_EPI_F32) {
            if (p.round_bf16) v = round_bf16(v);
            if (p.residual) v += p.residual[orow * p.ldr + n + r];
            if (p.rowmod) v += p.rowmod[(int64_t)(m % p.rowmod_period) * p.N + n + r];
            if (p.out_scale != 0.f) v *= p.out_scale;
            ((float*)p.out)[orow * p.ldo + n + r] = v;
            if (p.out2) ((bf16_t*)p.out2)[orow * p.ldo2 + n + r] = f2bf(v);
        } else if constexpr (EPI == VT_EPI_BF16_DGELU) {   // the unrounded accumulator again, as above
            const float u = bf2f(((const bf16_t*)p.aux)[(int64_t)m * p.ldaux + n + r]);
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = f2bf(v * gelu_erf_grad(u));
        } else {
            const bf16_t h = f2bf(v);
            bf16_t aux = h, out, out2 = h;
            if constexpr (epi_has_aux(EPI)) aux = ((const bf16_t*)p.aux)[(int64_t)m * p.ldaux + n + r];
            epi_value<EPI>(h, aux, out, out2);
            ((bf16_t*)p.out)[orow * p.ldo + n + r] = out;
            if constexpr (epi_has_out2(EPI)) ((bf16_t*)p.out2)[orow * p.ldo2 + n + r] = out2;
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
