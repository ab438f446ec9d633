// Per-element arithmetic of the finite scalar quantizer (models/model_new/quantizer/fsq.py:62-131), shared by the stand-alone
// FSQ kernels (vt_fsq.hip) and the fused token gate of `autoencoder_stat` (vt_stat.hip), so that both give the same bits.
//
//   bounded   = tanh(z + shift) * half_l - offset        fsq.py:76-81
//   quantized = rint(bounded)  (straight-through)        fsq.py:47-50,83-88
//   codes     = quantized / (levels // 2)
//   indices   = int32( sum_c (codes_c * hw_c + hw_c) * basis_c )      fsq.py:90-92,103-107
//   dz        = dcodes / hw * half_l * (1 - tanh^2)       the straight-through gradient autograd derives
//
// All fp32 in the reference's operation order, never contracted into FMAs (every function body turns contraction off).
// tanh is evaluated in double and rounded: the correctly rounded fp32 tanh, the value oracle/fsq_oracle.c computes with libm.
#pragma once
#include "vt_common.h"

#include <cmath>

#define FSQ_MAX_D 16

struct FsqConsts {
    int d;
    int levels[FSQ_MAX_D];
    int basis[FSQ_MAX_D];
    float half_l[FSQ_MAX_D], offset[FSQ_MAX_D], shift[FSQ_MAX_D], half_width[FSQ_MAX_D];
};

// host side of fsq.py:62-73,78-80; identical to oracle/fsq_oracle.c:fsq_constants.  d must be in [1, FSQ_MAX_D].
static inline bool fsq_make_consts(const int32_t* levels, int d, FsqConsts& k) {
    int64_t b = 1;
    k.d = d;
    for (int c = 0; c < d; ++c) {
        if (levels[c] < 2) return false;
        k.levels[c] = levels[c];
        k.half_l[c] = (float)(levels[c] - 1) * (float)(1.0 + 1e-3) / 2.0f;
        k.offset[c] = (levels[c] % 2 == 0) ? 0.5f : 0.0f;
        k.shift[c] = (float)atanh((double)(k.offset[c] / k.half_l[c]));
        k.half_width[c] = (float)(levels[c] / 2);
        k.basis[c] = (int)b;
        b *= levels[c];
        if (b > (1 << 24)) return false;  // the reference sums level indices in fp32: exact only below 2^24
    }
    return true;
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__device__ __forceinline__ float fsq_tanh_rn(float x) { return (float)tanh((double)x); }

// code of channel c
__device__ __forceinline__ float fsq_code(float z, const FsqConsts& k, int c) {
#pragma clang fp contract(off)
    const float t = fsq_tanh_rn(z + k.shift[c]);
    const float bounded = t * k.half_l[c] - k.offset[c];
    return __fdiv_rn(rintf(bounded), k.half_width[c]);
}

// channel c's term of the index sum: an integer below 2^24, so the fp32 sum of the terms is exact in any order
__device__ __forceinline__ float fsq_index_term(float code, const FsqConsts& k, int c) {
#pragma clang fp contract(off)
    return (code * k.half_width[c] + k.half_width[c]) * (float)k.basis[c];
}

// straight-through gradient of channel c
__device__ __forceinline__ float fsq_grad(float z, float dcode, const FsqConsts& k, int c) {
#pragma clang fp contract(off)
    const float t = fsq_tanh_rn(z + k.shift[c]);
    const float g = __fdiv_rn(dcode, k.half_width[c]);
    return (g * k.half_l[c]) * (1.0f - t * t);
}
#endif
