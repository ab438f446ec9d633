// The patch ends' one source: how 8 consecutive pixels of one image row of a video map into a patch-row matrix, and how they move.  Shared by
// vt_patch.hip (vt_patchify / vt_unpatchify and their two-segment _dual siblings) and the clips half of vt_packed.hip (vt_patchify_clips /
// vt_unpatchify_clips), so that the three families agree bit for bit by construction: the column order (c, dt, dy, dx) == the flattening of a
// Conv3d weight [D, C, pt, ph, pw], the token order (t, h, w) t-major, and the one f2bf per pixel are written here and nowhere else.
// Threads are laid out over the VIDEO index space, so the video side is fully coalesced (unit idx = pixels 8 idx .. 8 idx + 7 of a contiguous
// block); the patch-row side moves 16-B (bf16) / 32-B (fp32) pieces, 2+ lanes per contiguous run.  pw % 8 == 0 keeps a unit inside one patch row.
#pragma once
#include "vt_common.h"

namespace {

// unit idx of a contiguous fp32 [*, C, T, H, W] block: image row y of frame t of plane = outer * C + c, pixels x .. x + 7; its video offset is
// idx * 8.  (The plane is left whole: a caller with one clip per block has outer == 0 and spares the division by C.)
struct PatchUnit {
    int64_t plane;
    int t, y, x;
};
__device__ __forceinline__ PatchUnit patch_unit(int64_t idx, int T, int H, int W) {
    const int w8 = W >> 3;
    PatchUnit u;
    u.x = (int)(idx % w8) * 8;
    idx /= w8;
    u.y = (int)(idx % H);
    idx /= H;
    u.t = (int)(idx % T);
    u.plane = idx / T;
    return u;
}

// element offset tok * Kp + col of pixel (c, ts, y, x) in the row matrix of its segment: ts = t - the segment's first frame, (pt, Kp) the segment's
// temporal patch and row width C * pt * ph * pw, Hh x Ww the spatial token grid, row0 the first row of the clip's segment
__device__ __forceinline__ int64_t patch_offset(int c, int ts, int y, int x, int pt, int Kp, int ph, int pw, int Hh, int Ww, int64_t row0) {
    const int tt = ts / pt, dt = ts % pt, hh = y / ph, dy = y % ph, ww = x / pw, dx = x % pw;
    const int64_t tok = row0 + ((int64_t)tt * Hh + hh) * Ww + ww;
    const int col = ((c * pt + dt) * ph + dy) * pw + dx;
    return tok * Kp + col;
}

// the only place where a pixel of a patch end is rounded or copied.  TO_ROWS: 8 fp32 pixels at video8 -> bf16 rows + off (one f2bf each, one
// 16-B store); otherwise fp32 rows + off -> the 8 pixels at video8
template <bool TO_ROWS>
__device__ __forceinline__ void patch_move(float* video8, void* rows, int64_t off) {
    if constexpr (TO_ROWS) {
        const f32x4 a0 = *(const f32x4*)video8, a1 = *(const f32x4*)(video8 + 4);
        const bf16x8 o = {f2bf(a0[0]), f2bf(a0[1]), f2bf(a0[2]), f2bf(a0[3]), f2bf(a1[0]), f2bf(a1[1]), f2bf(a1[2]), f2bf(a1[3])};
        *(bf16x8*)((bf16_t*)rows + off) = o;
    } else {
        const float* src = (const float*)rows + off;
        const f32x4 a0 = *(const f32x4*)src, a1 = *(const f32x4*)(src + 4);
        *(f32x4*)video8 = a0;
        *(f32x4*)(video8 + 4) = a1;
    }
}

}  // namespace
