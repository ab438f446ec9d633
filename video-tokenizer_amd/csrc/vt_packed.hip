// Data movement of the packed `titok` model (models/model_titok/base/blocks.py:82-222) for gfx950 -- HBM-bound copies, 16 B per lane
// and access where the layout allows.
//
// A batch of this family has no period: every clip has its own (T, H, W), every sequence of the packed residual stream is
// [lead rows | tail rows] with its own two counts (the encoder's [latent tokens | patch rows], the decoder's [codes | mask tokens]).
// The periodic vtRowMap cannot say that, so the kernels here take TABLES: validated host arrays that travel BY VALUE in the kernel
// arguments, like SeqTable of vt_attention.hip.  No kernel reads a boundary or a pointer from device memory, every launch can be captured
// in a graph, every table has at most VT_VARLEN_MAX_SEQ entries and the largest argument block (ClipTable) is 1.8 KB.  Every index into a
// table is wave-uniform (a workgroup works on one clip, a wave on one row at a time), so the tables are read with scalar loads.
// No atomics anywhere: every result has the same bits on every run.
//
// patchify_clips  : n clips, each its own contiguous fp32 [C, T_b, H_b, W_b] -> bf16 rows [sum G_b, Kp], G_b = (T_b/pt)(H_b/p)(W_b/p),
//                   Kp = C*pt*p*p; column order (c, dt, dy, dx) and token order (t, h, w) of vt_patchify, = the rearrange of blocks.py:128;
//                   clip b starts at row sum_{a<b} G_a.  One launch for all clips.
// unpatchify_clips: the inverse on fp32 rows, into n separate fp32 clips (blocks.py:214-220).
// packed_scatter  : dst fp32 [M, D]; the chosen segment (lead or tail) of every sequence takes the rows of a compact src in order, the
//                   other segment takes vec[D] (or zeros): blocks.py:132-135 and :197-200, and the backward of the gather.
// packed_gather   : the chosen segment's rows of a packed [M, D] -> compact (blocks.py:140-142, :207-209).
// packed_segment_colsum: out[D] = sum over the chosen segment's rows of all sequences (the gradient of mask_token), in a fixed order.
#include "vt_patch_map.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// clips
// ---------------------------------------------------------------------------------------------------------------------------------
struct ClipTable {
    int n, C, pt, p, Kp;
    int T[VT_VARLEN_MAX_SEQ], H[VT_VARLEN_MAX_SEQ], W[VT_VARLEN_MAX_SEQ];
    int row0[VT_VARLEN_MAX_SEQ + 1];   // patch rows before clip b
    int blk0[VT_VARLEN_MAX_SEQ + 1];   // workgroups before clip b: ceil(units_b / 256), a unit = 8 consecutive pixels of one image row
    void* ptr[VT_VARLEN_MAX_SEQ];
};

// blk[lo] <= gb < blk[lo + 1], by a scalar bisection (gb is wave-uniform)
__device__ __forceinline__ int find_entry(const int* __restrict__ start, int n, int gb) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= gb) lo = mid;
        else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// A workgroup works on one clip (found by bisection, so every table index is wave-uniform); behind that the lane layout, the patch map and the
// move are those of vt_patch_map.h, with the clip as the whole contiguous block (its plane is the channel).
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void clips_kernel(const ClipTable tab, void* __restrict__ rows_) {
    const int b = find_entry(tab.blk0, tab.n, blockIdx.x);
    const int T = tab.T[b], H = tab.H[b], W = tab.W[b];
    const int64_t units = (int64_t)tab.C * T * H * (W >> 3);
    const int64_t idx = (int64_t)(blockIdx.x - tab.blk0[b]) * 256 + threadIdx.x;
    if (idx >= units) return;
    const PatchUnit u = patch_unit(idx, T, H, W);
    const int64_t off = patch_offset((int)u.plane, u.t, u.y, u.x, tab.pt, tab.Kp, tab.p, tab.p, H / tab.p, W / tab.p, tab.row0[b]);
    patch_move<TO_ROWS>((float*)tab.ptr[b] + idx * 8, rows_, off);
}

int clip_table(const char* who, const vtClip* clips, int n, int C, int pt, int p, int64_t rows_total, ClipTable* tab) {
    VT_CHECK_ARG(clips != nullptr, "%s: the clip table is null", who);
    VT_CHECK_ARG(n >= 1 && n <= VT_VARLEN_MAX_SEQ, "%s: n=%d outside 1..%d clips per launch", who, n, VT_VARLEN_MAX_SEQ);
    VT_CHECK_ARG(C > 0 && pt > 0 && p > 0, "%s: bad geometry C=%d pt=%d p=%d", who, C, pt, p);
    VT_CHECK_ARG(p % 8 == 0, "%s: p=%d must be a multiple of 8", who, p);
    VT_CHECK_ARG((int64_t)C * pt * p * p <= 0x7fffffff, "%s: patch of C=%d pt=%d p=%d too large", who, C, pt, p);
    tab->n = n, tab->C = C, tab->pt = pt, tab->p = p, tab->Kp = C * pt * p * p;
    int64_t rows = 0, blocks = 0;
    for (int b = 0; b < n; ++b) {
        const vtClip& c = clips[b];
        VT_CHECK_ARG(c.data != nullptr, "%s: clip %d has a null pointer", who, b);
        VT_CHECK_ARG(aligned16(c.data), "%s: clip %d (%p) is not 16-byte aligned", who, b, c.data);
        VT_CHECK_ARG(c.T > 0 && c.H > 0 && c.W > 0, "%s: clip %d has a bad size T=%d H=%d W=%d", who, b, c.T, c.H, c.W);
        VT_CHECK_ARG(c.T % pt == 0, "%s: clip %d: T=%d is no multiple of pt=%d", who, b, c.T, pt);
        VT_CHECK_ARG(c.H % p == 0, "%s: clip %d: H=%d is no multiple of p=%d", who, b, c.H, p);
        VT_CHECK_ARG(c.W % p == 0, "%s: clip %d: W=%d is no multiple of p=%d", who, b, c.W, p);
        const int64_t units = (int64_t)C * c.T * c.H * (c.W / 8);
        tab->T[b] = c.T, tab->H[b] = c.H, tab->W[b] = c.W, tab->ptr[b] = c.data;
        tab->row0[b] = (int)rows, tab->blk0[b] = (int)blocks;
        rows += (int64_t)(c.T / pt) * (c.H / p) * (c.W / p);
        blocks += (units + 255) / 256;
        VT_CHECK_ARG(rows <= 0x7fffffff && blocks <= 0x7fffffff, "%s: clips 0..%d are too large for one launch", who, b);
    }
    for (int b = n; b < VT_VARLEN_MAX_SEQ; ++b) tab->T[b] = tab->H[b] = tab->W[b] = 8, tab->ptr[b] = nullptr;
    for (int b = n; b <= VT_VARLEN_MAX_SEQ; ++b) tab->row0[b] = (int)rows, tab->blk0[b] = (int)blocks;
    VT_CHECK_ARG(rows == rows_total, "%s: rows=%lld must equal the clips' %lld patches", who, (long long)rows_total, (long long)rows);
    return VT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// packed rows
// ---------------------------------------------------------------------------------------------------------------------------------
struct PackTable {
    int n, tail;                       // sequences; tail = 1: the chosen segment is the tail
    int cu[VT_VARLEN_MAX_SEQ + 1];     // first packed row of sequence b; cu[n] = M
    int lead[VT_VARLEN_MAX_SEQ];       // rows of the lead segment of sequence b
    int seg0[VT_VARLEN_MAX_SEQ + 1];   // rows of the chosen segment before sequence b; seg0[n] = the compact row count
};

// one wave per row at a time (the row and everything read from the table are wave-uniform), lanes over the row's 16-byte pieces
__global__ __launch_bounds__(256) void packed_scatter_kernel(const PackTable tab, const float* __restrict__ src, const float* __restrict__ vec,
                                                             float* __restrict__ dst, int M, int D) {
    const int lane = threadIdx.x & 63, pieces = D >> 2;
    for (int m = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); m < M; m += gridDim.x * 4) {
        const int b = find_entry(tab.cu, tab.n, m);
        const int r = m - tab.cu[b], lead = tab.lead[b];
        const bool in_tail = r >= lead;
        f32x4* o = (f32x4*)(dst + (int64_t)m * D);
        if (in_tail == (tab.tail != 0)) {
            const f32x4* s = (const f32x4*)(src + (int64_t)(tab.seg0[b] + (in_tail ? r - lead : r)) * D);
            for (int i = lane; i < pieces; i += 64) o[i] = s[i];
        } else if (vec) {
            for (int i = lane; i < pieces; i += 64) o[i] = ((const f32x4*)vec)[i];
        } else {
            for (int i = lane; i < pieces; i += 64) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

__device__ __forceinline__ int64_t packed_row_of(const PackTable& tab, int j) {
    const int b = find_entry(tab.seg0, tab.n, j);
    return (int64_t)tab.cu[b] + (tab.tail ? tab.lead[b] : 0) + (j - tab.seg0[b]);
}

__global__ __launch_bounds__(256) void packed_gather_kernel(const PackTable tab, const float* __restrict__ packed, float* __restrict__ out, int D) {
    const int lane = threadIdx.x & 63, pieces = D >> 2, R = tab.seg0[tab.n];
    for (int j = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); j < R; j += gridDim.x * 4) {
        const f32x4* s = (const f32x4*)(packed + packed_row_of(tab, j) * D);
        f32x4* o = (f32x4*)(out + (int64_t)j * D);
        for (int i = lane; i < pieces; i += 64) o[i] = s[i];
    }
}

// slab blockIdx.y adds its rows_per_slab consecutive rows of the chosen segment (in compact order) into part[slab][D]; a thread owns 4 columns
__global__ __launch_bounds__(256) void packed_colsum_kernel(const PackTable tab, const float* __restrict__ packed, float* __restrict__ part, int D,
                                                            int rows_per_slab) {
    const int piece = blockIdx.x * 256 + threadIdx.x;
    const int R = tab.seg0[tab.n];
    const int j0 = blockIdx.y * rows_per_slab, j1 = j0 + rows_per_slab < R ? j0 + rows_per_slab : R;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (piece < (D >> 2)) {
        for (int j = j0; j < j1; ++j) acc += *((const f32x4*)(packed + packed_row_of(tab, j) * D) + piece);
        *((f32x4*)(part + (int64_t)blockIdx.y * D) + piece) = acc;
    }
}

__global__ __launch_bounds__(256) void packed_colsum_final_kernel(const float* __restrict__ part, int slabs, int D, float* __restrict__ out) {
    const int piece = blockIdx.x * 256 + threadIdx.x;
    if (piece >= (D >> 2)) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < slabs; ++s) acc += *((const f32x4*)(part + (int64_t)s * D) + piece);
    *((f32x4*)out + piece) = acc;
}

int pack_table(const char* who, const int32_t* cu, const int32_t* lead, int n, int M, int D, int which, PackTable* tab) {
    VT_CHECK_ARG(cu != nullptr && lead != nullptr, "%s: cu_seqlens_host or lead_host is null", who);
    VT_CHECK_ARG(n >= 1 && n <= VT_VARLEN_MAX_SEQ, "%s: n_seq=%d outside 1..%d sequences per launch", who, n, VT_VARLEN_MAX_SEQ);
    VT_CHECK_ARG(M > 0 && D > 0, "%s: bad shape M=%d D=%d", who, M, D);
    VT_CHECK_ARG(D % 4 == 0, "%s: D=%d must be a multiple of 4", who, D);
    VT_CHECK_ARG(which == VT_PACKED_LEAD || which == VT_PACKED_TAIL, "%s: which=%d is neither VT_PACKED_LEAD nor VT_PACKED_TAIL", who, which);
    VT_CHECK_ARG(cu[0] == 0, "%s: cu_seqlens[0]=%d must be 0", who, cu[0]);
    for (int b = 0; b < n; ++b) {
        VT_CHECK_ARG(cu[b + 1] > cu[b], "%s: cu_seqlens must increase strictly: cu[%d]=%d, cu[%d]=%d", who, b, cu[b], b + 1, cu[b + 1]);
        VT_CHECK_ARG(lead[b] >= 1 && lead[b] < cu[b + 1] - cu[b], "%s: lead[%d]=%d outside 1..%d (both segments of a %d-row sequence must be non-empty)",
                     who, b, lead[b], cu[b + 1] - cu[b] - 1, cu[b + 1] - cu[b]);
    }
    VT_CHECK_ARG(cu[n] == M, "%s: cu_seqlens[%d]=%d must equal M=%d", who, n, cu[n], M);
    tab->n = n, tab->tail = which == VT_PACKED_TAIL;
    int seg = 0;
    for (int b = 0; b <= VT_VARLEN_MAX_SEQ; ++b) {
        tab->cu[b] = b <= n ? cu[b] : M;
        tab->seg0[b] = seg;
        if (b < VT_VARLEN_MAX_SEQ) tab->lead[b] = b < n ? lead[b] : 0;
        if (b < n) seg += tab->tail ? cu[b + 1] - cu[b] - lead[b] : lead[b];
    }
    return VT_OK;
}

int row_grid(int rows) { return rows / 4 + 1 < 4096 ? rows / 4 + 1 : 4096; }

#define VT_PACKED_COLSUM_SLABS 256

}  // namespace

extern "C" int vt_patchify_clips(const vtClip* clips_host, int32_t n, int32_t C, int32_t pt, int32_t p, void* rows_bf16, int64_t rows,
                                 vtStream stream) {
    const char* who = "vt_patchify_clips";
    ClipTable tab;
    VT_CHECK_ARG(rows_bf16 != nullptr, "%s: rows is null", who);
    VT_CHECK_ARG(aligned16(rows_bf16), "%s: rows (%p) is not 16-byte aligned", who, rows_bf16);
    TRY(clip_table(who, clips_host, n, C, pt, p, rows, &tab));
    hipLaunchKernelGGL(clips_kernel<true>, dim3(tab.blk0[n]), dim3(256), 0, (hipStream_t)stream, tab, rows_bf16);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_unpatchify_clips(const float* rows_f32, int64_t rows, const vtClip* clips_host, int32_t n, int32_t C, int32_t pt, int32_t p,
                                   vtStream stream) {
    const char* who = "vt_unpatchify_clips";
    ClipTable tab;
    VT_CHECK_ARG(rows_f32 != nullptr, "%s: rows is null", who);
    VT_CHECK_ARG(aligned16(rows_f32), "%s: rows (%p) is not 16-byte aligned", who, (const void*)rows_f32);
    TRY(clip_table(who, clips_host, n, C, pt, p, rows, &tab));
    hipLaunchKernelGGL(clips_kernel<false>, dim3(tab.blk0[n]), dim3(256), 0, (hipStream_t)stream, tab, (void*)rows_f32);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_packed_scatter(const float* src, const float* vec, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq,
                                 int32_t M, int32_t D, int32_t which, float* dst, vtStream stream) {
    const char* who = "vt_packed_scatter";
    PackTable tab;
    VT_CHECK_ARG(src != nullptr && dst != nullptr, "%s: src or dst is null", who);
    VT_CHECK_ARG(aligned16(src) && aligned16(dst) && aligned16(vec), "%s: src, vec and dst must be 16-byte aligned", who);
    TRY(pack_table(who, cu_seqlens_host, lead_host, n_seq, M, D, which, &tab));
    hipLaunchKernelGGL(packed_scatter_kernel, dim3(row_grid(M)), dim3(256), 0, (hipStream_t)stream, tab, src, vec, dst, M, D);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_packed_gather(const float* packed, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq, int32_t M, int32_t D,
                                int32_t which, float* out, vtStream stream) {
    const char* who = "vt_packed_gather";
    PackTable tab;
    VT_CHECK_ARG(packed != nullptr && out != nullptr, "%s: packed or out is null", who);
    VT_CHECK_ARG(aligned16(packed) && aligned16(out), "%s: packed and out must be 16-byte aligned", who);
    TRY(pack_table(who, cu_seqlens_host, lead_host, n_seq, M, D, which, &tab));
    hipLaunchKernelGGL(packed_gather_kernel, dim3(row_grid(tab.seg0[n_seq])), dim3(256), 0, (hipStream_t)stream, tab, packed, out, D);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" size_t vt_packed_segment_colsum_workspace_bytes(int32_t D) {
    return D > 0 ? (size_t)VT_PACKED_COLSUM_SLABS * D * sizeof(float) : 0;
}

extern "C" int vt_packed_segment_colsum(const float* packed, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq, int32_t M,
                                        int32_t D, int32_t which, float* out, void* workspace, vtStream stream) {
    const char* who = "vt_packed_segment_colsum";
    PackTable tab;
    VT_CHECK_ARG(packed != nullptr && out != nullptr && workspace != nullptr, "%s: packed, out or workspace is null", who);
    VT_CHECK_ARG(aligned16(packed) && aligned16(out) && aligned16(workspace), "%s: packed, out and workspace must be 16-byte aligned", who);
    TRY(pack_table(who, cu_seqlens_host, lead_host, n_seq, M, D, which, &tab));
    const int R = tab.seg0[n_seq];
    const int rps = (R + VT_PACKED_COLSUM_SLABS - 1) / VT_PACKED_COLSUM_SLABS < 4 ? 4 : (R + VT_PACKED_COLSUM_SLABS - 1) / VT_PACKED_COLSUM_SLABS;
    const int slabs = (R + rps - 1) / rps;      // <= VT_PACKED_COLSUM_SLABS, every slab has a row
    const int gx = (D / 4 + 255) / 256;
    hipLaunchKernelGGL(packed_colsum_kernel, dim3(gx, slabs), dim3(256), 0, (hipStream_t)stream, tab, packed, (float*)workspace, D, rps);
    hipLaunchKernelGGL(packed_colsum_final_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, slabs, D, out);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
