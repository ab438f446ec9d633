// (T,H,W) patchify / unpatchify for gfx950, over one or two temporal segments -- HBM-bound, 16-32 B per lane per access.
//
// patchify  : video fp32 [B,C,T,H,W]  ->  patch rows bf16 [B*Nv, Kp], Kp = C*pt*ph*pw, column order
//             (c, dt, dy, dx) == the flattening of the Conv3d weight [D,C,pt,p,p] (models/embed.py:82),
//             token order (t,h,w) t-major (embed.py:112).  Also used on d(pred_frames) in backward.
// unpatchify: rows fp32 [B*Nv, Kp] in the SAME (c,dt,dy,dx) column order -> video fp32 [B,C,T,H,W]; every element of video is written
//             exactly once.  The reference's head emits columns in (dt,dy,dx,c) order (channel last,
//             models/larp_tokenizer.py:452-453); the head weight rows are permuted once at pack time
//             so both directions share this coalesced layout.
// The _dual pair are the ends of the reference's `autoencoder_dualpatch` (models/model_dualpatch/base/blocks.py:99-112, 234-257), which cuts a
// clip along time into frames [0, T0) with a (pt0, ph, pw) patch and frames [T0, T) with a (pt1, ph, pw) patch, each with a row matrix of its
// own: rows0 [B*(T0/pt0)*(H/ph)*(W/pw), C*pt0*ph*pw] and rows1 [B*((T-T0)/pt1)*(H/ph)*(W/pw), C*pt1*ph*pw].  One launch each, no slice copy
// of the video and no concatenation behind it; H != W and ph != pw are fine.  vt_patchify / vt_unpatchify are the one-segment case with
// H = W = S and ph = pw = p: the same kernel template, the same validation.
// The lane layout, the patch map and the move are those of vt_patch_map.h; a lane's t selects its segment.  The grid covers the lanes
// exactly (no cap, no stride loop); plain vector loads and stores, no atomics, no LDS.
#include "vt_patch_map.h"

namespace {

struct Segment {
    int t_begin, pt, Th, Kp;  // first frame, temporal patch, temporal token count, row width C*pt*ph*pw
};

template <int NSEG>
struct PatchGeom {
    int C, T, H, W, ph, pw, Hh, Ww;  // Hh x Ww: the spatial token grid
    Segment seg[NSEG];
    int64_t total;                   // lanes: B*C*T*H*(W/8)
};

// the segment is picked by select, never by indexing (the geometry stays in scalar registers); with one segment the select compiles away
template <int NSEG, bool TO_ROWS>
__global__ __launch_bounds__(256) void patch_segments_kernel(float* __restrict__ video, PatchGeom<NSEG> g, void* __restrict__ rows0,
                                                             void* __restrict__ rows1) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const PatchUnit u = patch_unit(idx, g.T, g.H, g.W);
    const int c = (int)(u.plane % g.C);
    const int64_t b = u.plane / g.C;
    const bool s = NSEG == 2 && u.t >= g.seg[NSEG - 1].t_begin;
    const int t_begin = s ? g.seg[NSEG - 1].t_begin : 0, pt = s ? g.seg[NSEG - 1].pt : g.seg[0].pt;
    const int Th = s ? g.seg[NSEG - 1].Th : g.seg[0].Th, Kp = s ? g.seg[NSEG - 1].Kp : g.seg[0].Kp;
    const int64_t off = patch_offset(c, u.t - t_begin, u.y, u.x, pt, Kp, g.ph, g.pw, g.Hh, g.Ww, b * Th * g.Hh * g.Ww);
    patch_move<TO_ROWS>(video + idx * 8, s ? rows1 : rows0, off);
}

// host validation shared by the four entry points: VT_OK and a filled geometry and grid, or VT_ERR_INVALID with vt_last_error set.  The
// one-segment callers pass T0 = T, pt1 = pt0 and no rows1; their S and p are reported as H = W and ph = pw.
template <int NSEG>
int make_geom(const char* who, PatchGeom<NSEG>& g, unsigned& grid, const void* video, const void* rows0, const void* rows1, int B, int C, int T,
              int H, int W, int T0, int pt0, int pt1, int ph, int pw) {
    constexpr bool dual = NSEG == 2;
    VT_CHECK_ARG(video != nullptr && rows0 != nullptr && (rows1 != nullptr || !dual), dual ? "%s: video, rows0 or rows1 is null" : "%s: video or rows is null", who);
    VT_CHECK_ARG(aligned16(video), "%s: video (%p) is not 16-byte aligned", who, video);
    VT_CHECK_ARG(aligned16(rows0), dual ? "%s: rows0 (%p) is not 16-byte aligned" : "%s: rows (%p) is not 16-byte aligned", who, rows0);
    VT_CHECK_ARG(aligned16(rows1), "%s: rows1 (%p) is not 16-byte aligned", who, rows1);
    VT_CHECK_ARG(B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "%s: bad size B=%d C=%d T=%d H=%d W=%d", who, B, C, T, H, W);
    VT_CHECK_ARG(pt0 > 0 && pt1 > 0 && ph > 0 && pw > 0, "%s: bad patch pt0=%d pt1=%d ph=%d pw=%d", who, pt0, pt1, ph, pw);
    VT_CHECK_ARG(!dual || (T0 > 0 && T0 < T), "%s: T0=%d outside 1..%d (both segments of T=%d frames must be non-empty)", who, T0, T - 1, T);
    VT_CHECK_ARG(T0 % pt0 == 0, dual ? "%s: T0=%d is no multiple of pt0=%d" : "%s: T=%d is no multiple of pt=%d", who, T0, pt0);
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
    if constexpr (dual) g.seg[1] = Segment{T0, pt1, (T - T0) / pt1, (int)kp1};
    g.total = total;
    grid = (unsigned)blocks;
    return VT_OK;
}

// validate, then one launch; rows1 == nullptr and T0 == T for one segment
template <int NSEG, bool TO_ROWS>
int launch(const char* who, const void* video, const void* rows0, const void* rows1, int B, int C, int T, int H, int W, int T0, int pt0, int pt1,
           int ph, int pw, vtStream stream) {
    PatchGeom<NSEG> g;
    unsigned grid;
    TRY(make_geom(who, g, grid, video, rows0, rows1, B, C, T, H, W, T0, pt0, pt1, ph, pw));
    hipLaunchKernelGGL((patch_segments_kernel<NSEG, TO_ROWS>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (float*)video, g, (void*)rows0, (void*)rows1);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // namespace

extern "C" int vt_patchify(const float* video, int32_t B, int32_t C, int32_t T, int32_t S, int32_t pt, int32_t p, void* rows_bf16,
                           vtStream stream) {
    return launch<1, true>("vt_patchify", video, rows_bf16, nullptr, B, C, T, S, S, T, pt, pt, p, p, stream);
}

extern "C" int vt_unpatchify(const float* rows, int32_t B, int32_t C, int32_t T, int32_t S, int32_t pt, int32_t p, float* video,
                             vtStream stream) {
    return launch<1, false>("vt_unpatchify", video, rows, nullptr, B, C, T, S, S, T, pt, pt, p, p, stream);
}

extern "C" int vt_patchify_dual(const float* video, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0, int32_t pt0, int32_t pt1,
                                int32_t ph, int32_t pw, void* rows0_bf16, void* rows1_bf16, vtStream stream) {
    return launch<2, true>("vt_patchify_dual", video, rows0_bf16, rows1_bf16, B, C, T, H, W, T0, pt0, pt1, ph, pw, stream);
}

extern "C" int vt_unpatchify_dual(const float* rows0, const float* rows1, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0,
                                  int32_t pt0, int32_t pt1, int32_t ph, int32_t pw, float* video, vtStream stream) {
    return launch<2, false>("vt_unpatchify_dual", video, rows0, rows1, B, C, T, H, W, T0, pt0, pt1, ph, pw, stream);
}
