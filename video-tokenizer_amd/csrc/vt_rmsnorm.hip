// The whole-row RMSNorm entry points for gfx950: three families over the two kernel templates of vt_rmsnorm.h.
//   vt_rmsnorm_*          the AR consumer's norm (models/norm.py:6-17): fp32 rows in, bf16 out for the next GEMM; the llama-abs widths
//   vt_rmsnorm_any_*      the same at the widths of model_design as well (norm_q / norm_kv / the blocks' norms, transformer.py:18-27)
//   vt_rmsnorm_any_f32_*  final_norm of model_design's stack (:211, :216): fp32, unrounded output and an fp32 incoming gradient
// A family is its names, the widths it accepts, its type and whether it checks alignment (Family below); the checks, the width dispatch and
// the launches are written once.  HBM-bound single passes, one wave per row, 8 bytes per lane and access.
#include "vt_common.h"
#include "vt_rmsnorm.h"

#include <type_traits>

namespace {

// X(J, llama): a kernel exists for dim = 128 J; llama = the width is a llama-abs size, which every family accepts (the others: all but vt_rmsnorm_*)
#define RMS_WIDTHS(X) X(1, false) X(2, false) X(3, true) X(4, false) X(6, true) X(8, true) X(10, true) X(12, true) X(20, true)

struct Family {
    const char *fwd, *bwd;                  // the entry points' names, under which refusals and launch failures are reported
    const char *fwd_accepts, *bwd_accepts;  // what the refusal of a width adds about the accepted ones
    bool llama_only;                        // accepts the llama-abs widths only
    bool aligned;                           // asks for 16-byte aligned buffers
};
constexpr Family kLlama = {"vt_rmsnorm_fwd", "vt_rmsnorm_bwd", " (384, 768, 1024, 1280, 1536, 2560: the llama-abs sizes)", "", true, false};
constexpr Family kAny = {"vt_rmsnorm_any_fwd", "vt_rmsnorm_any_bwd", " (128, 256, 512 and the widths of vt_rmsnorm_fwd)", "", false, false};
constexpr Family kAnyF32 = {"vt_rmsnorm_any_f32_fwd", "vt_rmsnorm_any_f32_bwd", " (the widths of vt_rmsnorm_any_fwd)", " (the widths of vt_rmsnorm_any_fwd)", false, true};

bool width_ok(const Family& fam, int dim) {
#define X(J, LLAMA) if (dim == J * 128) return LLAMA || !fam.llama_only;
    RMS_WIDTHS(X)
#undef X
    return false;
}

// launch(std::integral_constant<int, J>) for J = dim / 128 (dim has passed width_ok)
template <typename Launch>
void at_width(int dim, Launch launch) {
    switch (dim / 128) {
#define X(J, LLAMA) case J: launch(std::integral_constant<int, J>()); break;
        RMS_WIDTHS(X)
#undef X
    }
}

template <typename T>
int forward(const Family& fam, const float* x, const float* w, float eps, int64_t rows, int32_t dim, T* y, float* rstd, vtStream stream) {
    VT_CHECK_ARG(x && w && y && rows > 0, "%s: null pointer", fam.fwd);
    VT_CHECK_ARG(width_ok(fam, dim), "%s: width %d unsupported%s", fam.fwd, dim, fam.fwd_accepts);
    VT_CHECK_ARG(!fam.aligned || (aligned16(x) && aligned16(w) && aligned16(y)), "%s: buffers must be 16-byte aligned", fam.fwd);
    const int grid = (int)((rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048);
    at_width(dim, [&](auto j) {
        hipLaunchKernelGGL((rmsnorm_fwd_kernel<decltype(j)::value, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, eps, rows, y, rstd);
    });
    VT_CHECK_LAUNCH(fam.fwd);
    return VT_OK;
}

size_t workspace_bytes(int32_t dim) { return (size_t)RMS_BLOCKS * dim * sizeof(float); }

// dres and dxb are the bf16 families' (the fp32 kernels do not look at them)
template <typename T>
int backward(const Family& fam, const T* dy, const float* x, const float* w, const float* rstd, const float* dres, int64_t rows, int32_t dim, float* dx,
             bf16_t* dxb, float* dw, void* workspace, vtStream stream) {
    VT_CHECK_ARG(dy && x && w && rstd && (dx || dxb) && dw && workspace && rows > 0, "%s: null pointer", fam.bwd);
    VT_CHECK_ARG(width_ok(fam, dim), "%s: width %d unsupported%s", fam.bwd, dim, fam.bwd_accepts);
    VT_CHECK_ARG(!fam.aligned || (aligned16(dy) && aligned16(x) && aligned16(w) && aligned16(dx) && aligned16(workspace)), "%s: buffers must be 16-byte aligned",
                 fam.bwd);
    float* part = (float*)workspace;
    at_width(dim, [&](auto j) {
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<decltype(j)::value, T>), dim3(RMS_BLOCKS), dim3(256), 0, (hipStream_t)stream, dy, x, w, rstd, dres, rows, dx, dxb,
                           part);
    });
    VT_CHECK_LAUNCH(fam.bwd);
    return vt_sum_slabs(part, RMS_BLOCKS, (int64_t)dim, dim, dw, stream);
}

}  // namespace

extern "C" int vt_rmsnorm_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, void* y_bf16, float* rstd, vtStream stream) {
    return forward(kLlama, x, w, eps, rows, dim, (bf16_t*)y_bf16, rstd, stream);
}
extern "C" size_t vt_rmsnorm_bwd_workspace_bytes(int32_t dim) { return workspace_bytes(dim); }
extern "C" int vt_rmsnorm_bwd(const void* dy_bf16, const float* x, const float* w, const float* rstd, const float* dres, int64_t rows, int32_t dim,
                              float* dx, void* dx_bf16, float* dw, void* workspace, vtStream stream) {
    return backward(kLlama, (const bf16_t*)dy_bf16, x, w, rstd, dres, rows, dim, dx, (bf16_t*)dx_bf16, dw, workspace, stream);
}

extern "C" int vt_rmsnorm_any_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, void* y_bf16, float* rstd, vtStream stream) {
    return forward(kAny, x, w, eps, rows, dim, (bf16_t*)y_bf16, rstd, stream);
}
extern "C" size_t vt_rmsnorm_any_bwd_workspace_bytes(int32_t dim) { return workspace_bytes(dim); }
extern "C" int vt_rmsnorm_any_bwd(const void* dy_bf16, const float* x, const float* w, const float* rstd, const float* dres, int64_t rows, int32_t dim,
                                  float* dx, void* dx_bf16, float* dw, void* workspace, vtStream stream) {
    return backward(kAny, (const bf16_t*)dy_bf16, x, w, rstd, dres, rows, dim, dx, (bf16_t*)dx_bf16, dw, workspace, stream);
}

extern "C" int vt_rmsnorm_any_f32_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, float* y, float* rstd, vtStream stream) {
    return forward(kAnyF32, x, w, eps, rows, dim, y, rstd, stream);
}
extern "C" size_t vt_rmsnorm_any_f32_bwd_workspace_bytes(int32_t dim) { return workspace_bytes(dim); }
extern "C" int vt_rmsnorm_any_f32_bwd(const float* dy, const float* x, const float* w, const float* rstd, int64_t rows, int32_t dim, float* dx, float* dw,
                                      void* workspace, vtStream stream) {
    return backward(kAnyF32, dy, x, w, rstd, nullptr, rows, dim, dx, nullptr, dw, workspace, stream);
}
