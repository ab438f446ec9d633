// The row pass of model_design's CrossAttention layer (models/model_design/base/transformer.py:92-141) for gfx950.  Its GEMMs are
// vt_gemm_nt / vt_gemm_tn_grouped, its attention vt_attention_cross_*, its gate vt_sigmoid_gate_cols_* (vt_gated.hip), its whole-row norms
// norm_q / norm_kv (:108-109, :123-124) vt_rmsnorm_any_* (vt_rmsnorm.hip); here is
//   head_rmsnorm  q_norm / k_norm (:18-27, :114-115, :134-135): RMSNorm over each 64-element head vector of a bf16 row
// HBM-bound single passes with 16-byte accesses.  Rounding as the reference under autocast(bf16): the head norm reads the bf16 Linear
// output and computes y = bf16(bf16(x * rstd) * w), rstd = rsqrt(mean(x^2) + eps) in fp32, w fp32.  The statistics and the backward step are
// vt_headvec.h's, shared with the fused q/k pass of vt_design.hip.
#include "vt_common.h"
#include "vt_headvec.h"

namespace {
constexpr int NBLK = 512;    // blocks of the backward = partial sums of dw: [NBLK, 64] fp32

__global__ __launch_bounds__(256) void head_rmsnorm_fwd_kernel(const bf16_t* __restrict__ x, int64_t x_rs, const float* __restrict__ w, float eps, int64_t M,
                                                                int H, bf16_t* __restrict__ y, int64_t y_rs) {
    const int lane = threadIdx.x & 7;
    const int64_t nvec = M * H;
    float wr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wr[i] = w[lane * 8 + i];
    for (int64_t vec = (int64_t)blockIdx.x * VPB + (threadIdx.x >> 3); vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int col = (int)(vec % H) * HD + lane * 8;
        const Vec8 xv = load8(x + row * x_rs + col);
        const float rstd = head_rstd(xv, eps);
        Vec8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.v[i] = round_bf16(xv.v[i] * rstd) * wr[i];
        store8(y + row * y_rs + col, r);
    }
}

// head_rmsnorm_bwd_step per head vector (fp32, one rounding at the store of dx; in dw the forward's rounding of x * rstd is not replayed, a step
// function inside a sum that is held to 1e-5).  dx may be dy's buffer: a lane reads its 16 bytes of dy before it writes the same 16 bytes of dx
// (no __restrict__ on the two).
// part: [NBLK, 64]
__global__ __launch_bounds__(256) void head_rmsnorm_bwd_kernel(const bf16_t* dy, int64_t dy_rs, const bf16_t* __restrict__ x, int64_t x_rs,
                                                                const float* __restrict__ w, float eps, int64_t M, int H, bf16_t* dx, int64_t dx_rs,
                                                                float* __restrict__ part) {
    __shared__ float red[VPB][HD];
    const int lane = threadIdx.x & 7, vslot = threadIdx.x >> 3;
    const int64_t nvec = M * H;
    float wr[8], aw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) aw[i] = 0.f, wr[i] = w[lane * 8 + i];
    for (int64_t vec = (int64_t)blockIdx.x * VPB + vslot; vec < nvec; vec += (int64_t)gridDim.x * VPB) {
        const int64_t row = vec / H;
        const int col = (int)(vec % H) * HD + lane * 8;
        const Vec8 xv = load8(x + row * x_rs + col);
        const Vec8 gy = load8(dy + row * dy_rs + col);
        store8(dx + row * dx_rs + col, head_rmsnorm_bwd_step(xv, gy, wr, head_rstd(xv, eps), aw));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[vslot][lane * 8 + i] = aw[i];
    __syncthreads();
    if (threadIdx.x < HD) {
        float t = 0.f;
#pragma unroll 8
        for (int v = 0; v < VPB; ++v) t += red[v][threadIdx.x];
        part[(int64_t)blockIdx.x * HD + threadIdx.x] = t;
    }
}

bool head_stride_ok(int64_t rs, int H) { return rs >= (int64_t)HD * H && rs % 8 == 0; }
}  // namespace

extern "C" int vt_head_rmsnorm_fwd(const void* x, int64_t x_rs, const float* w, float eps, int64_t M, int32_t H, void* y, int64_t y_rs, vtStream stream) {
    VT_CHECK_ARG(x && w && y, "vt_head_rmsnorm_fwd: null pointer");
    VT_CHECK_ARG(M > 0 && H > 0 && H <= 1024, "vt_head_rmsnorm_fwd: M=%lld H=%d out of range", (long long)M, H);
    VT_CHECK_ARG(head_stride_ok(x_rs, H) && head_stride_ok(y_rs, H), "vt_head_rmsnorm_fwd: row strides %lld, %lld must cover 64 x %d columns and be multiples of 8",
                 (long long)x_rs, (long long)y_rs, H);
    VT_CHECK_ARG(aligned16(x) && aligned16(y), "vt_head_rmsnorm_fwd: buffers must be 16-byte aligned");
    const int64_t nvec = M * H;
    const int gx = (int)((nvec + VPB - 1) / VPB < 2048 ? (nvec + VPB - 1) / VPB : 2048);
    hipLaunchKernelGGL(head_rmsnorm_fwd_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, x_rs, w, eps, M, H, (bf16_t*)y, y_rs);
    VT_CHECK_LAUNCH("vt_head_rmsnorm_fwd");
    return VT_OK;
}

extern "C" size_t vt_head_rmsnorm_bwd_workspace_bytes(void) { return (size_t)NBLK * HD * sizeof(float); }

extern "C" int vt_head_rmsnorm_bwd(const void* dy, int64_t dy_rs, const void* x, int64_t x_rs, const float* w, float eps, int64_t M, int32_t H, void* dx,
                                   int64_t dx_rs, float* dw, void* workspace, vtStream stream) {
    VT_CHECK_ARG(dy && x && w && dx && dw && workspace, "vt_head_rmsnorm_bwd: null pointer");
    VT_CHECK_ARG(M > 0 && H > 0 && H <= 1024, "vt_head_rmsnorm_bwd: M=%lld H=%d out of range", (long long)M, H);
    VT_CHECK_ARG(head_stride_ok(dy_rs, H) && head_stride_ok(x_rs, H) && head_stride_ok(dx_rs, H),
                 "vt_head_rmsnorm_bwd: row strides %lld, %lld, %lld must cover 64 x %d columns and be multiples of 8", (long long)dy_rs, (long long)x_rs,
                 (long long)dx_rs, H);
    {   // every lane reads its own 16 bytes of dy and x before it writes the same 16 bytes of dx: dx may be dy itself (same base, same
        // stride) and otherwise overlaps neither input
        const int64_t w = (int64_t)HD * H;
        auto lo = [](const void* p) { return (uintptr_t)p; };
        auto hi = [&](const void* p, int64_t rs) { return (uintptr_t)p + (uintptr_t)(((M - 1) * rs + w) * 2); };
        auto overlap = [&](const void* a, int64_t ars) { return lo(dx) < hi(a, ars) && lo(a) < hi(dx, dx_rs); };
        VT_CHECK_ARG(!overlap(x, x_rs), "vt_head_rmsnorm_bwd: dx overlaps x (dx may share dy's buffer, not x's)");
        VT_CHECK_ARG((dx == dy && dx_rs == dy_rs) || !overlap(dy, dy_rs), "vt_head_rmsnorm_bwd: dx overlaps dy without being dy itself (same pointer and row stride)");
    }
    VT_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(workspace), "vt_head_rmsnorm_bwd: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(head_rmsnorm_bwd_kernel, dim3(NBLK), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, dy_rs, (const bf16_t*)x, x_rs, w, eps, M, H,
                       (bf16_t*)dx, dx_rs, (float*)workspace);
    VT_CHECK_LAUNCH("vt_head_rmsnorm_bwd");
    return vt_reduce_waves("vt_head_rmsnorm_bwd(reduce)", (const float*)workspace, NBLK, HD, HD, dw, nullptr, nullptr, nullptr, stream);
}
