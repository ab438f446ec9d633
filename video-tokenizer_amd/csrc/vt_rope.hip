// Rotary position embedding on the packed attention operand of the plain block stack, for gfx950
// (models/model_new/base/simpletransformer.py:46-53 Attn.forward, base/rope.py:18-24 apply_rotary_emb).
//
// qkv is the bf16 [M, 3D] output of the qkv GEMM, columns [q | k | v], D = 64 H, M = B * L rows; row m has position m % L.
// The q and k column blocks are rotated IN PLACE; v is neither read nor written.  A head's 64 elements are 32 complex
// numbers (x[2j], x[2j+1]) (view_as_complex of [..., 32, 2]); pair j of every head of a row is multiplied by
// cos_tab[pos, j] + i sin_tab[pos, j] (conjugate = 0, forward) or by its conjugate (conjugate = 1: the backward of the
// rotation, applied to dq and dk).  Rounding as the reference under autocast(bf16): bf16 in, fp32 arithmetic, one
// rounding to bf16 (`apply_rotary_emb(...).type_as(x)` on the bf16 Linear output).
//
// HBM-bound element-wise pass.  A lane owns 16 bytes = 8 bf16 = 4 pairs, and reads the 4 matching cos and 4 sin factors as
// two 16-byte loads (the tables are L x 128 B each and stay in L2).  A workgroup is (lanes of a row) x (rows): the row and
// its position are computed once per thread and row, not per element.  Every lane reads and writes its own 16 bytes, so
// the in-place update needs no ordering; rows M .. of a padded workspace are not touched.  No trigonometry on the device.
#include "vt_common.h"

namespace {

constexpr int kMaxThreads = 256;

__global__ __launch_bounds__(kMaxThreads) void rope_rotate_kernel(bf16_t* __restrict__ qkv, int64_t ld, int M, int L, int per_row,
                                                                  const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                                  float sgn) {
    const int row_step = gridDim.x * blockDim.y;
    for (int r = blockIdx.x * blockDim.y + threadIdx.y; r < M; r += row_step) {
        const int pos = r % L;
        bf16_t* row = qkv + (int64_t)r * ld;
        const float* ct = cos_tab + (int64_t)pos * 32;
        const float* st = sin_tab + (int64_t)pos * 32;
        for (int c = threadIdx.x; c < per_row; c += blockDim.x) {          // c-th 16-byte piece of the row's [q | k] columns
            const int j = (c & 7) * 4;                                      // first of this lane's 4 pairs inside its head
            bf16x8* p = (bf16x8*)(row + c * 8);
            const bf16x8 x = *p;
            const f32x4 co = *(const f32x4*)(ct + j);
            const f32x4 si = *(const f32x4*)(st + j) * sgn;
            bf16x8 y;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = bf2f(x[2 * i]), b = bf2f(x[2 * i + 1]);
                y[2 * i] = f2bf(a * co[i] - b * si[i]);
                y[2 * i + 1] = f2bf(a * si[i] + b * co[i]);
            }
            *p = y;
        }
    }
}

}  // namespace

extern "C" int vt_rope_rotate(void* qkv, int64_t ld, int64_t M, int32_t L, int32_t H, const float* cos_tab, const float* sin_tab,
                              int32_t conjugate, vtStream stream) {
    VT_CHECK_ARG(qkv && cos_tab && sin_tab, "vt_rope_rotate: null pointer");
    VT_CHECK_ARG(M > 0 && M <= 0x7fffffff && L > 0 && H > 0 && H <= 1024, "vt_rope_rotate: M=%lld L=%d H=%d out of range (head_dim is 64: D = 64 H)",
                 (long long)M, L, H);
    VT_CHECK_ARG(ld >= (int64_t)128 * H && ld % 8 == 0, "vt_rope_rotate: row stride %lld must cover the q and k columns (2 x 64 x %d) and be a multiple of 8",
                 (long long)ld, H);
    VT_CHECK_ARG(conjugate == 0 || conjugate == 1, "vt_rope_rotate: conjugate must be 0 or 1");
    VT_CHECK_ARG(aligned16(qkv) && aligned16(cos_tab) && aligned16(sin_tab), "vt_rope_rotate: buffers must be 16-byte aligned");
    const int per_row = 16 * H;                                             // 16-byte pieces of [q | k] in a row
    const int tx = per_row < kMaxThreads ? per_row : kMaxThreads;           // a multiple of 16
    const int ty = kMaxThreads / tx;
    const int64_t groups = (M + ty - 1) / ty;
    const int gx = (int)(groups < 4096 ? groups : 4096);
    hipLaunchKernelGGL(rope_rotate_kernel, dim3(gx), dim3(tx, ty), 0, (hipStream_t)stream, (bf16_t*)qkv, ld, (int)M, L, per_row, cos_tab, sin_tab,
                       conjugate ? -1.0f : 1.0f);
    VT_CHECK_LAUNCH("vt_rope_rotate");
    return VT_OK;
}
