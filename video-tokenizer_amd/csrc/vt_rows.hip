// HBM-bound row utilities for gfx950: the fixed-order reducers of per-slab partial sums, column sums (bias gradients), batch sums
// (query-embedding gradients), fp32->bf16 row casts, zeroing, sequence assembly and the scaled copy of gradient rows.  Each lane moves
// 16 B per access.
#include "vt_common.h"

namespace {

// The column reduction of every partial-sum reducer here: o[w][c] = sum_s partial[s * slab_stride + w * width + c] for column
// c = blockIdx.x * 32 + tx and output w = blockIdx.y.  Lane ty of `lanes` adds slabs ty, ty + lanes, ... in order; the partial sums go
// through the LDS tile; thread row 0 adds the `lanes` of them in index order.  Fixed summation order => deterministic, and one text for
// the stand-alone and the grouped kernel => the same bits from both.
__device__ __forceinline__ void reduce_columns(float (*red)[33], const float* __restrict__ partial, int nslab, int64_t slab_stride, int width, int lanes,
                                               float* const* o) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    const int w = blockIdx.y;
    float s = 0.f;
    if (c < width && ty < lanes) {
        const float* p = partial + (int64_t)w * width + c;
#pragma unroll 4
        for (int i = ty; i < nslab; i += lanes) s += p[(int64_t)i * slab_stride];
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < width) {
        float t = 0.f;
        for (int k = 0; k < lanes; ++k) t += red[k][tx];
        o[w][c] = t;
    }
}

// workgroup = 32 columns x NL slab lanes
struct ReduceOuts {
    float* o[3];
};
template <int NL>  // slab lanes per column: 8 (256 threads) or 32 (1024 threads, for the 512-slab LayerNorm partials)
__global__ __launch_bounds__(32 * NL) void reduce_partials_kernel(const float* __restrict__ partial, int nslab, int64_t slab_stride, int width,
                                                                   ReduceOuts outs) {
    __shared__ float red[NL][33];
    reduce_columns(red, partial, nslab, slab_stride, width, NL, outs.o);
}

// several reductions in one launch (blockIdx.z = item), each with the lanes of the stand-alone launch it stands for
struct ReduceGroup {
    vtReduceItem it[VT_REDUCE_MAX_GROUP];
};
__global__ __launch_bounds__(1024) void reduce_grouped_kernel(const ReduceGroup g) {
    __shared__ float red[32][33];
    const vtReduceItem& q = g.it[blockIdx.z];
    if ((int)blockIdx.y >= q.nout || blockIdx.x * 32 >= q.width) return;      // uniform per workgroup
    reduce_columns(red, q.partial, q.nslab, q.slab_stride, q.width, q.lanes, q.o);
}

// the reducer of the head-vector row passes (vt_reduce_waves, vt_common.h): one wave per output element t, lane l adds partials l, l + 64, ...
// in order, then the fixed butterfly of wave_sum; element t belongs to destination t / 64
__global__ __launch_bounds__(256) void reduce_waves_kernel(const float* __restrict__ part, int nblk, int64_t row_stride, int nout, float* d0, float* d1,
                                                            float* d2, float* d3) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= nout) return;      // uniform per wave
    float s = 0.f;
    for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * row_stride + t];
    s = wave_sum(s);
    float* dst = (t >> 6) == 0 ? d0 : (t >> 6) == 1 ? d1 : (t >> 6) == 2 ? d2 : d3;
    if (dst && lane == 0) dst[t & 63] = s;
}

// ------------------------------------------------------------------------------------------------
// column sums of a [rows, width] matrix (bf16 or fp32, optional row map) -> partial[slab][width]
// workgroup = 4 waves over one 512-column chunk; lane owns 8 consecutive columns
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ src, int64_t ld, RowMap map, int64_t rows, int width,
                                                      int rows_per_slab, float* __restrict__ partial) {
    __shared__ float red[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 512 + lane * 8;
    const int slab = blockIdx.y;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t r_begin = (int64_t)slab * rows_per_slab;
    const int64_t r_end = r_begin + rows_per_slab < rows ? r_begin + rows_per_slab : rows;
    if (c0 < width) {
        // four rows of a wave are requested before the first is added (one load in flight per wave left the kernel at 1.6-2.4 TB/s); the
        // additions keep their order, so the sums are the bits they were
        constexpr int UN = 4;
        int64_t r = r_begin + wave;
        for (; r + 4 * (UN - 1) < r_end; r += 4 * UN) {
            if constexpr (sizeof(T) == 2) {
                bf16x8 v[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) v[u] = *(const bf16x8*)(src + map(r + 4 * u) * ld + c0);
#pragma unroll
                for (int u = 0; u < UN; ++u)
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] += bf2f(v[u][k]);
            } else {
                f32x4 v0[UN], v1[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const T* p = src + map(r + 4 * u) * ld + c0;
                    v0[u] = *(const f32x4*)p, v1[u] = *(const f32x4*)(p + 4);
                }
#pragma unroll
                for (int u = 0; u < UN; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) { acc[k] += v0[u][k]; acc[4 + k] += v1[u][k]; }
            }
        }
        for (; r < r_end; r += 4) {
            const T* p = src + map(r) * ld + c0;
            if constexpr (sizeof(T) == 2) {
                const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] += bf2f(v[k]);
            } else {
                const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) { acc[k] += v0[k]; acc[4 + k] += v1[k]; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane * 8 + k] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256) {
        const int gc = blockIdx.x * 512 + c;
        if (gc < width) partial[(int64_t)slab * width + gc] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// zero rows map(r), r < rows, of an fp32 [*, dim] matrix and of its bf16 twin
__global__ void zero_rows_kernel(float* __restrict__ a, bf16_t* __restrict__ b, RowMap map, int64_t rows, int dim) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over rows * dim / 4
    const int d4 = dim >> 2;
    if (idx >= rows * d4) return;
    const int64_t pr = map(idx / d4);
    const int c = (idx % d4) * 4;
    if (a) *(f32x4*)(a + pr * dim + c) = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (b) *(bf16x4*)(b + pr * dim + c) = (bf16x4){f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
}

// out[j, :] = sum_b src[map(b * n + j), :]   (fp32)
__global__ void batch_sum_kernel(const float* __restrict__ src, RowMap map, int batch, int n, int dim, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over n * dim / 4
    const int d4 = dim >> 2;
    if (idx >= (int64_t)n * d4) return;
    const int j = idx / d4, c = (idx % d4) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < batch; ++b) {
        const f32x4 v = *(const f32x4*)(src + map((int64_t)b * n + j) * dim + c);
        s += v;
    }
    *(f32x4*)(out + (int64_t)j * dim + c) = s;
}

// dst[r, :] = bf16(src[map(r), :])
__global__ void cast_rows_kernel(const float* __restrict__ src, RowMap map, int64_t rows, int dim, bf16_t* __restrict__ dst, int64_t ldd) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over rows * dim / 4
    const int d4 = dim >> 2;
    if (idx >= rows * d4) return;
    const int64_t r = idx / d4;
    const int c = (idx % d4) * 4;
    const f32x4 v = *(const f32x4*)(src + map(r) * dim + c);
    *(bf16x4*)(dst + r * ldd + c) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}

// dst[b*seq + off + j, :] = (src ? src[(b*n + j), :] : 0) + (table ? table[j, :] : 0) + (vec ? vec[:] : 0)
__global__ void assemble_rows_kernel(float* __restrict__ dst, int64_t seq, int64_t off, int batch, int n, int dim,
                                     const float* __restrict__ src, const float* __restrict__ table, const float* __restrict__ vec) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int d4 = dim >> 2;
    if (idx >= (int64_t)batch * n * d4) return;
    const int c = (idx % d4) * 4;
    const int64_t r = idx / d4;
    const int j = r % n;
    const int64_t b = r / n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (src) v += *(const f32x4*)(src + r * dim + c);
    if (table) v += *(const f32x4*)(table + (int64_t)j * dim + c);
    if (vec) v += *(const f32x4*)(vec + c);
    *(f32x4*)(dst + (b * seq + off + j) * dim + c) = v;
}

// dst (fp32) and / or dstb (bf16) = scale * src, over n4 groups of 4 elements: the scaled copy of gradient rows
__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ src, float scale, int64_t n4, float* __restrict__ dst, bf16_t* __restrict__ dstb) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 v = ((const f32x4*)src)[i];
        v *= scale;
        if (dst) ((f32x4*)dst)[i] = v;
        if (dstb) ((bf16x4*)dstb)[i] = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    }
}

}  // namespace

int vt_reduce_partials(const char* who, const float* partial, int nslab, int64_t slab_stride, int width, float* o0, float* o1, float* o2, vtStream stream) {
    const ReduceOuts ro = {{o0, o1, o2}};
    const dim3 grid((width + 31) / 32, o2 ? 3 : o1 ? 2 : 1);
    if (nslab >= 128) hipLaunchKernelGGL(reduce_partials_kernel<32>, grid, dim3(1024), 0, (hipStream_t)stream, partial, nslab, slab_stride, width, ro);
    else hipLaunchKernelGGL(reduce_partials_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, partial, nslab, slab_stride, width, ro);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_reduce_waves(const char* who, const float* part, int nblk, int64_t row_stride, int nout, float* d0, float* d1, float* d2, float* d3, vtStream stream) {
    hipLaunchKernelGGL(reduce_waves_kernel, dim3((nout + 3) / 4), dim3(256), 0, (hipStream_t)stream, part, nblk, row_stride, nout, d0, d1, d2, d3);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_reduce_grouped(const vtReduceItem* items, int n, vtStream stream) {
    VT_CHECK_ARG(items && n > 0 && n <= VT_REDUCE_MAX_GROUP, "vt_reduce_grouped: 1..%d items", VT_REDUCE_MAX_GROUP);
    ReduceGroup g;
    int wmax = 0, nout = 0;
    for (int i = 0; i < n; ++i) {
        g.it[i] = items[i];
        VT_CHECK_ARG(items[i].partial && items[i].nout >= 1 && items[i].nout <= 3 && (items[i].lanes == 8 || items[i].lanes == 32), "vt_reduce_grouped: bad item %d", i);
        wmax = items[i].width > wmax ? items[i].width : wmax;
        nout = items[i].nout > nout ? items[i].nout : nout;
    }
    hipLaunchKernelGGL(reduce_grouped_kernel, dim3((wmax + 31) / 32, nout, n), dim3(1024), 0, (hipStream_t)stream, g);
    VT_CHECK_LAUNCH("vt_reduce_grouped");
    return VT_OK;
}

#define VT_COLSUM_SLABS 64
extern "C" size_t vt_colsum_workspace_bytes(int32_t width) { return (size_t)VT_COLSUM_SLABS * width * sizeof(float); }

extern "C" int vt_colsum(const void* src, int32_t src_is_bf16, int64_t ld, vtRowMap map, int64_t rows, int32_t width, float* out,
                         void* workspace, vtStream stream) {
    VT_CHECK_ARG(src && out && workspace, "vt_colsum: null pointer");
    VT_CHECK_ARG(rows > 0 && width > 0 && width % 8 == 0 && ld % 8 == 0, "vt_colsum: width/ld must be multiples of 8");
    int slabs = (int)((rows + 63) / 64);
    if (slabs > VT_COLSUM_SLABS) slabs = VT_COLSUM_SLABS;
    const int rps = (int)((rows + slabs - 1) / slabs);
    const dim3 grid((width + 511) / 512, slabs);
    hipStream_t s = (hipStream_t)stream;
    if (src_is_bf16)
        hipLaunchKernelGGL(colsum_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)src, ld, to_map(map), rows, width, rps, (float*)workspace);
    else
        hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, s, (const float*)src, ld, to_map(map), rows, width, rps, (float*)workspace);
    return vt_reduce_partials("vt_colsum", (const float*)workspace, slabs, (int64_t)width, width, out, nullptr, nullptr, stream);
}

extern "C" int vt_zero_rows(float* a, void* b_bf16, vtRowMap map, int64_t rows, int32_t dim, vtStream stream) {
    VT_CHECK_ARG((a || b_bf16) && rows > 0 && dim % 4 == 0, "vt_zero_rows: bad arguments");
    const int64_t total = rows * (dim / 4);
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, (bf16_t*)b_bf16, to_map(map), rows, dim);
    VT_CHECK_LAUNCH("vt_zero_rows");
    return VT_OK;
}

// out[c] = sum_s slabs[s * slab_stride + c]  (fixed order; e.g. split-M partial weight gradients)
extern "C" int vt_sum_slabs(const float* slabs, int32_t nslab, int64_t slab_stride, int32_t width, float* out, vtStream stream) {
    VT_CHECK_ARG(slabs && out && nslab > 0 && width > 0, "vt_sum_slabs: bad arguments");
    return vt_reduce_partials("vt_sum_slabs", slabs, nslab, slab_stride, width, out, nullptr, nullptr, stream);
}

extern "C" int vt_batch_sum(const float* src, vtRowMap map, int32_t batch, int32_t n, int32_t dim, float* out, vtStream stream) {
    VT_CHECK_ARG(src && out && batch > 0 && n > 0 && dim % 4 == 0, "vt_batch_sum: bad arguments");
    const int64_t total = (int64_t)n * (dim / 4);
    hipLaunchKernelGGL(batch_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, to_map(map), batch, n, dim, out);
    VT_CHECK_LAUNCH("vt_batch_sum");
    return VT_OK;
}

extern "C" int vt_cast_rows(const float* src, vtRowMap map, int64_t rows, int32_t dim, void* dst_bf16, int64_t ldd, vtStream stream) {
    VT_CHECK_ARG(src && dst_bf16 && rows > 0 && dim % 4 == 0 && ldd % 4 == 0 && ldd >= dim, "vt_cast_rows: bad arguments");
    const int64_t total = rows * (dim / 4);
    hipLaunchKernelGGL(cast_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, to_map(map), rows, dim, (bf16_t*)dst_bf16, ldd);
    VT_CHECK_LAUNCH("vt_cast_rows");
    return VT_OK;
}

extern "C" int vt_assemble_rows(float* dst, int64_t seq, int64_t off, int32_t batch, int32_t n, int32_t dim, const float* src,
                                const float* table, const float* vec, vtStream stream) {
    VT_CHECK_ARG(dst && batch > 0 && n > 0 && dim % 4 == 0 && off >= 0 && off + n <= seq, "vt_assemble_rows: bad arguments");
    const int64_t total = (int64_t)batch * n * (dim / 4);
    hipLaunchKernelGGL(assemble_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, seq, off, batch, n, dim, src, table, vec);
    VT_CHECK_LAUNCH("vt_assemble_rows");
    return VT_OK;
}

extern "C" int vt_scale_rows(const float* src, float scale, int64_t rows, int32_t dim, float* dst_f32, void* dst_bf16, vtStream stream) {
    VT_CHECK_ARG(src && (dst_f32 || dst_bf16) && rows > 0 && dim > 0 && dim % 4 == 0, "vt_scale_rows: bad arguments (dim %% 4 == 0)");
    VT_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst_f32) & 15) == 0 && ((uintptr_t)dst_bf16 & 7) == 0, "vt_scale_rows: unaligned pointer");
    const int64_t n4 = rows * dim / 4;
    const int grid = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, scale, n4, dst_f32, (bf16_t*)dst_bf16);
    VT_CHECK_LAUNCH("vt_scale_rows");
    return VT_OK;
}
