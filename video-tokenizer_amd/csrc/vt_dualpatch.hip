// Two-segment (T,H,W) patchify / unpatchify for gfx950: the ends of the reference's `autoencoder_dualpatch`
// (models/model_dualpatch/base/blocks.py:99-112, 234-257), which cuts a clip along time into frames [0, T0) with a (pt0, ph, pw) patch and
// frames [T0, T) with a (pt1, ph, pw) patch, each with a row matrix of its own.
//
// patchify  : video fp32 [B,C,T,H,W] -> rows0 bf16 [B*(T0/pt0)*(H/ph)*(W/pw), C*pt0*ph*pw] and rows1 bf16 [B*((T-T0)/pt1)*(H/ph)*(W/pw),
//             C*pt1*ph*pw]; column order (c, dt, dy, dx) == the flattening of a Conv3d weight, token order (t, h, w) t-major per clip, both as
//             in vt_patch.hip, whose rounding this shares (one f2bf per pixel).  Also used on d(pred_frames) in backward.
// unpatchify: the inverse on two fp32 row matrices; every element of video is written exactly once.
// One launch each, no slice copy of the video and no concatenation behind it.  Threads are laid out over the VIDEO index space as in
// vt_patch.hip: a lane moves 8 consecutive pixels of one image row (fully coalesced on the video side), its t selects the segment, and the
// row side moves 16-B (bf16) / 32-B (fp32) pieces.  The grid covers the lanes exactly (no cap, no stride loop); plain vector loads and
// stores, no atomics, no LDS.  H != W and ph != pw are fine.
#include "vt_common.h"

namespace {

struct Segment {
    int t_begin, pt, Th, Kp;  // first frame, temporal patch, temporal token count, row width C*pt*ph*pw
};

struct DualGeom {
    int C, T, H, W, ph, pw, Hh, Ww;  // Hh x Ww: the spatial token grid
    Segment seg[2];
    int64_t total;                   // lanes: B*C*T*H*(W/8)
};

// the lane's 8 pixels: their offset in the video, their segment and their offset in that segment's row matrix
__device__ __forceinline__ void locate(const DualGeom& g, int64_t idx, int64_t& video_off, int& s, int64_t& row_off) {
    const int w8 = g.W >> 3;
    const int x = (int)(idx % w8) * 8;
    int64_t r = idx / w8;
    const int y = (int)(r % g.H);
    r /= g.H;
    const int t = (int)(r % g.T);
    r /= g.T;
    const int c = (int)(r % g.C);
    const int64_t b = r / g.C;
    video_off = idx * 8;
    s = t >= g.seg[1].t_begin;
    const int t_begin = s ? g.seg[1].t_begin : 0, pt = s ? g.seg[1].pt : g.seg[0].pt;
    const int Th = s ? g.seg[1].Th : g.seg[0].Th, Kp = s ? g.seg[1].Kp : g.seg[0].Kp;
    const int ts = t - t_begin;
    const int tt = ts / pt, dt = ts % pt, hh = y / g.ph, dy = y % g.ph, ww = x / g.pw, dx = x % g.pw;
    const int64_t tok = ((b * Th + tt) * g.Hh + hh) * g.Ww + ww;
    const int col = ((c * pt + dt) * g.ph + dy) * g.pw + dx;
    row_off = tok * Kp + col;
}

__global__ __launch_bounds__(256) void patchify_dual_kernel(const float* __restrict__ v, DualGeom g, bf16_t* __restrict__ rows0,
                                                            bf16_t* __restrict__ rows1) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    int64_t voff, roff;
    int s;
    locate(g, idx, voff, s, roff);
    const f32x4 a0 = *(const f32x4*)(v + voff), a1 = *(const f32x4*)(v + voff + 4);
    const bf16x8 o = {f2bf(a0[0]), f2bf(a0[1]), f2bf(a0[2]), f2bf(a0[3]), f2bf(a1[0]), f2bf(a1[1]), f2bf(a1[2]), f2bf(a1[3])};
    *(bf16x8*)((s ? rows1 : rows0) + roff) = o;
}

__global__ __launch_bounds__(256) void unpatchify_dual_kernel(const float* __restrict__ rows0, const float* __restrict__ rows1, DualGeom g,
                                                              float* __restrict__ v) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    int64_t voff, roff;
    int s;
    locate(g, idx, voff, s, roff);
    const float* src = (s ? rows1 : rows0) + roff;
    *(f32x4*)(v + voff) = *(const f32x4*)src;
    *(f32x4*)(v + voff + 4) = *(const f32x4*)(src + 4);
}

// host validation shared by the two entry points: VT_OK and a filled geometry and grid, or VT_ERR_INVALID with vt_last_error set
int make_geom(const char* who, DualGeom& g, unsigned& grid, const void* video, const void* rows0, const void* rows1, int B, int C, int T, int H,
              int W, int T0, int pt0, int pt1, int ph, int pw) {
    VT_CHECK_ARG(video != nullptr && rows0 != nullptr && rows1 != nullptr, "%s: video, rows0 or rows1 is null", who);
    VT_CHECK_ARG(aligned16(video), "%s: video (%p) is not 16-byte aligned", who, video);
    VT_CHECK_ARG(aligned16(rows0), "%s: rows0 (%p) is not 16-byte aligned", who, rows0);
    VT_CHECK_ARG(aligned16(rows1), "%s: rows1 (%p) is not 16-byte aligned", who, rows1);
    VT_CHECK_ARG(B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "%s: bad size B=%d C=%d T=%d H=%d W=%d", who, B, C, T, H, W);
    VT_CHECK_ARG(pt0 > 0 && pt1 > 0 && ph > 0 && pw > 0, "%s: bad patch pt0=%d pt1=%d ph=%d pw=%d", who, pt0, pt1, ph, pw);
    VT_CHECK_ARG(T0 > 0 && T0 < T, "%s: T0=%d outside 1..%d (both segments of T=%d frames must be non-empty)", who, T0, T - 1, T);
    VT_CHECK_ARG(T0 % pt0 == 0, "%s: T0=%d is no multiple of pt0=%d", who, T0, pt0);
    VT_CHECK_ARG((T - T0) % pt1 == 0, "%s: T-T0=%d is no multiple of pt1=%d", who, T - T0, pt1);
    VT_CHECK_ARG(H % ph == 0, "%s: H=%d is no multiple of ph=%d", who, H, ph);
    VT_CHECK_ARG(W % pw == 0, "%s: W=%d is no multiple of pw=%d", who, W, pw);
    VT_CHECK_ARG(pw % 8 == 0, "%s: pw=%d must be a multiple of 8", who, pw);
    const int64_t kp0 = (int64_t)C * pt0 * ph * pw, kp1 = (int64_t)C * pt1 * ph * pw;
    VT_CHECK_ARG(kp0 <= 0x7fffffff && kp1 <= 0x7fffffff, "%s: patch of C=%d pt0=%d pt1=%d ph=%d pw=%d too large", who, C, pt0, pt1, ph, pw);
    const int64_t total = (int64_t)B * C * T * H * (W / 8), blocks = (total + 255) / 256;
    VT_CHECK_ARG(blocks <= 0x7fffffff, "%s: B=%d C=%d T=%d H=%d W=%d is too large for one launch", who, B, C, T, H, W);
    g.C = C, g.T = T, g.H = H, g.W = W, g.ph = ph, g.pw = pw, g.Hh = H / ph, g.Ww = W / pw;
    g.seg[0] = Segment{0, pt0, T0 / pt0, (int)kp0};
    g.seg[1] = Segment{T0, pt1, (T - T0) / pt1, (int)kp1};
    g.total = total;
    grid = (unsigned)blocks;
    return VT_OK;
}

}  // namespace

extern "C" int vt_patchify_dual(const float* video, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0, int32_t pt0, int32_t pt1,
                                int32_t ph, int32_t pw, void* rows0_bf16, void* rows1_bf16, vtStream stream) {
    DualGeom g;
    unsigned grid;
    TRY(make_geom("vt_patchify_dual", g, grid, video, rows0_bf16, rows1_bf16, B, C, T, H, W, T0, pt0, pt1, ph, pw));
    hipLaunchKernelGGL(patchify_dual_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, video, g, (bf16_t*)rows0_bf16, (bf16_t*)rows1_bf16);
    VT_CHECK_LAUNCH("vt_patchify_dual");
    return VT_OK;
}

extern "C" int vt_unpatchify_dual(const float* rows0, const float* rows1, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0,
                                  int32_t pt0, int32_t pt1, int32_t ph, int32_t pw, float* video, vtStream stream) {
    DualGeom g;
    unsigned grid;
    TRY(make_geom("vt_unpatchify_dual", g, grid, video, rows0, rows1, B, C, T, H, W, T0, pt0, pt1, ph, pw));
    hipLaunchKernelGGL(unpatchify_dual_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows0, rows1, g, video);
    VT_CHECK_LAUNCH("vt_unpatchify_dual");
    return VT_OK;
}
