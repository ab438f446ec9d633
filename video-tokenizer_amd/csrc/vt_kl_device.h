// Per-element arithmetic of the diagonal-Gaussian KL bottleneck ('skl', models/bottleneck.py:36-64, 347-375), shared by the
// forward and backward row passes of vt_kl.hip.  z holds (mean, logvar) pairs interleaved: z[2c] = mean_c, z[2c + 1] = logvar_c.
#pragma once
#include "vt_common.h"

namespace vtkl {

// torch.clamp(logvar, -30, 20)
__device__ __forceinline__ float clamp_logvar(float lv) { return fminf(fmaxf(lv, -30.0f), 20.0f); }
// the clamp passes the gradient where the raw value lies inside the bounds, bounds included (torch's clamp_backward)
__device__ __forceinline__ bool logvar_live(float lv) { return lv >= -30.0f && lv <= 20.0f; }

// Two standard normals of the Box-Muller transform for pair index `pair` (elements 2 pair and 2 pair + 1 of the flat [M, d]
// noise).  `base` = pcg_hash(per-call seed word); the pair index and the high seed word are hashed in turn, the second uniform
// comes from one more round.  u1 in (0, 1) (never 0: log(u1) is finite, |g| <= 5.9), u2 in [0, 1).
__device__ __forceinline__ void gauss2(unsigned base, unsigned seed_hi, unsigned pair, float& g0, float& g1) {
    const unsigned h1 = pcg_hash(pcg_hash(base + pair) + seed_hi);
    const unsigned h2 = pcg_hash(h1 + 0x9E3779B9u);
    const float u1 = ((float)(h1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    g0 = r * c;
    g1 = r * s;
}

// forward of one channel: sample = mean + std * eps (unfused, as torch rounds it), returns the channel's KL term
__device__ __forceinline__ float forward1(float mean, float lv_raw, float eps, float& sample) {
    const float lv = clamp_logvar(lv_raw);
    const float sd = expf(0.5f * lv);
    const float var = expf(lv);
    sample = __fadd_rn(mean, __fmul_rn(sd, eps));
    return 0.5f * (__fadd_rn(__fadd_rn(__fmul_rn(mean, mean), var), -1.0f) - lv);
}

// backward of one channel: g = dL/dsample, gm = dL/dmean, k = dL/dloss_kl / batch
__device__ __forceinline__ void backward1(float mean, float lv_raw, float eps, float g, float gm, float k, float& dmean, float& dlv) {
    const float lv = clamp_logvar(lv_raw);
    const float sd = expf(0.5f * lv);
    const float var = expf(lv);
    dmean = fmaf(k, mean, g + gm);
    dlv = logvar_live(lv_raw) ? 0.5f * (g * eps * sd) + 0.5f * k * (var - 1.0f) : 0.0f;
}

}  // namespace vtkl
