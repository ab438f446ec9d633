// Weight packing for gfx950: fp32 master W[N,K] -> bf16 Wb[N, ldd] and/or its transpose bf16 WT[K, lddT], through an LDS tile.
// row_perm (optional): packed row r takes source row row_perm[r].  Up to VT_PACK_MAX_GROUP weights per launch (after an optimizer step
// every bf16 operand copy of the model is refreshed: ~100 matrices, launch-latency-bound one by one).
#include "vt_common.h"

namespace {

struct PackGroup {
    vtPackJob job[VT_PACK_MAX_GROUP];
    int tile_start[VT_PACK_MAX_GROUP + 1];
    int n;
};

// the job of workgroup blockIdx.x and the corner (n0, k0) of its edge x edge tile
__device__ __forceinline__ const vtPackJob& locate(const PackGroup& g, int edge, int& n0, int& k0) {
    int j = 0;
    while (j + 1 < g.n && (int)blockIdx.x >= g.tile_start[j + 1]) ++j;
    const vtPackJob& q = g.job[j];
    const int local = blockIdx.x - g.tile_start[j];
    const int tiles_k = (q.K + edge - 1) / edge;
    n0 = (local / tiles_k) * edge, k0 = (local % tiles_k) * edge;
    return q;
}

// One tile by 256 threads, each moving VEC consecutive elements per access.  VEC = 1: 32x32 tiles, any extents and bases.  VEC = 4: 64x64
// tiles, 16 bytes in / 8 bytes out per thread: a row of the tile is a whole 256-B (fp32 read) or 128-B (bf16 write) line in both the
// row-major and the transposed copy (the 32x32 tile writes 64-B half lines and ran at 2.3 TB/s of the 8 B/element it moves); needs K, N,
// ldd, lddT multiples of 4 and 16-/8-byte aligned bases (every tokenizer weight).
template <int VEC>
__device__ __forceinline__ void pack_tile(const PackGroup& g) {
    typedef __attribute__((ext_vector_type(VEC))) float F;
    typedef __attribute__((ext_vector_type(VEC))) bf16_t H;
    constexpr int EDGE = VEC == 1 ? 32 : 64, TX = EDGE / VEC, TY = 256 / TX;   // threads across x down: 32 x 8 or 16 x 16
    __shared__ float tile[EDGE][EDGE + 1];
    int n0, k0;
    const vtPackJob& q = locate(g, EDGE, n0, k0);
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    bf16_t* wb = (bf16_t*)q.wb;
    bf16_t* wt = (bf16_t*)q.wt;
#pragma unroll
    for (int i = 0; i < EDGE / TY; ++i) {
        const int n = n0 + ty + i * TY, k = k0 + tx * VEC;
        F v = 0.f;
        if (n < q.N && k < q.K) {
            const int sn = q.row_perm ? q.row_perm[n] : n;
            v = *(const F*)(q.w + (int64_t)sn * q.K + k);
            if (wb) {
                H o;
#pragma unroll
                for (int r = 0; r < VEC; ++r) o[r] = f2bf(v[r]);
                *(H*)(wb + (int64_t)n * q.ldd + k) = o;
            }
        }
#pragma unroll
        for (int r = 0; r < VEC; ++r) tile[ty + i * TY][tx * VEC + r] = v[r];
    }
    if (!wt) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EDGE / TY; ++i) {
        const int k = k0 + ty + i * TY, n = n0 + tx * VEC;
        if (n < q.N && k < q.K) {
            H o;
#pragma unroll
            for (int r = 0; r < VEC; ++r) o[r] = f2bf(tile[tx * VEC + r][ty + i * TY]);
            *(H*)(wt + (int64_t)k * q.lddT + n) = o;
        }
    }
}

__global__ __launch_bounds__(256) void pack_weight_group_kernel(const PackGroup g) { pack_tile<1>(g); }
__global__ __launch_bounds__(256) void pack_weight_group64_kernel(const PackGroup g) { pack_tile<4>(g); }

// one launch for jobs[0..n), n <= VT_PACK_MAX_GROUP, already validated: the 64x64 kernel if every job allows it, else the 32x32 one.
// `who`: the entry point's name, under which a launch failure is reported
int pack_group(const char* who, const vtPackJob* jobs, int n, vtStream stream) {
    PackGroup g;
    g.n = n;
    bool wide = true;
    for (int i = 0; i < n; ++i) {
        const vtPackJob& q = jobs[i];
        wide = wide && q.K % 4 == 0 && q.N % 4 == 0 && q.ldd % 4 == 0 && q.lddT % 4 == 0 && ((uintptr_t)q.w & 15) == 0 &&
               ((uintptr_t)q.wb & 7) == 0 && ((uintptr_t)q.wt & 7) == 0;
    }
    const int edge = wide ? 64 : 32;
    g.tile_start[0] = 0;
    for (int i = 0; i < n; ++i) {
        const vtPackJob& q = jobs[i];
        g.job[i] = q;
        g.tile_start[i + 1] = g.tile_start[i] + ((q.N + edge - 1) / edge) * ((q.K + edge - 1) / edge);
    }
    if (wide) hipLaunchKernelGGL(pack_weight_group64_kernel, dim3(g.tile_start[n]), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(pack_weight_group_kernel, dim3(g.tile_start[n]), dim3(256), 0, (hipStream_t)stream, g);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // namespace

extern "C" int vt_pack_weight(const float* w, int32_t N, int32_t K, const int32_t* row_perm, void* wb, int64_t ldd, void* wt,
                              int64_t lddT, vtStream stream) {
    VT_CHECK_ARG(w && (wb || wt) && N > 0 && K > 0, "vt_pack_weight: bad arguments");
    VT_CHECK_ARG((!wb || ldd >= K) && (!wt || lddT >= N), "vt_pack_weight: leading dimension too small");
    const vtPackJob job = {w, N, K, row_perm, wb, ldd, wt, lddT};
    return pack_group("vt_pack_weight", &job, 1, stream);
}

extern "C" int vt_pack_weights_grouped(const vtPackJob* jobs, int32_t n, vtStream stream) {
    VT_CHECK_ARG(jobs && n > 0, "vt_pack_weights_grouped: bad arguments");
    for (int base = 0; base < n; base += VT_PACK_MAX_GROUP) {
        const int m = n - base < VT_PACK_MAX_GROUP ? n - base : VT_PACK_MAX_GROUP;
        for (int i = base; i < base + m; ++i) {
            const vtPackJob& q = jobs[i];
            VT_CHECK_ARG(q.w && (q.wb || q.wt) && q.N > 0 && q.K > 0, "vt_pack_weights_grouped[%d]: bad arguments", i);
            VT_CHECK_ARG((!q.wb || q.ldd >= q.K) && (!q.wt || q.lddT >= q.N), "vt_pack_weights_grouped[%d]: leading dimension too small", i);
        }
        TRY(pack_group("vt_pack_weights_grouped", jobs + base, m, stream));
    }
    return VT_OK;
}
