// 3x3x3 convolution, padding 1, for gfx950: the three products of the 3D ResNet ends of the reference's `autoencoder_cnnvit`
// (models/model_cnnvit/base/cnnvit.py: ResnetBlock3D, Downsample3D, Upsample3D, conv_in / conv_out), plus the data movement around them
// (nearest-neighbour upsampling and the fp32 video <-> bf16 channels-last layout pair).
//
// Activations are bf16 channels-last [B, T, H, W, C] (the memory of a torch [B, C, T, H, W] tensor in channels_last_3d), C a multiple of 16.
//
// forward / dgrad : ONE implicit-GEMM kernel on v_mfma_f32_16x16x32_bf16.  A workgroup (4 waves) owns TT x TH x 16 output positions and 16*NF
//     output channels.  Per 32-channel slab of the source it stages the halo brick of the tile in LDS once (zeros outside the clip: padding is
//     zeros, and a brick never reaches into the next row, frame or clip because it is filled by (t, h, w) coordinate, not by flat offset) and
//     walks the 27 taps over it; the packed weights of three taps (one (kt, kh) row) are staged beside it.  The operand roles are swapped as in
//     the GEMMs (A = weights, B = positions), so a lane ends up with 4 consecutive output channels of one position: 8-byte stores.
//     A tap reads source index  idx = o * a + k - 1  per axis and uses it when idx % d == 0, at idx / d:
//         forward, stride s : a = s, d = 1              dgrad, stride s : a = 1, d = s, on the flipped and transposed weight pack
//     so the strided input gradient is the same kernel with a tap mask: wave-uniform in t and h (the MFMA is skipped), per lane in w (the
//     lane's operand is zero).  fp32 accumulation over all 27 * K products in a fixed order; no atomics.
// wgrad : dW[co][ci][tap] = sum over output positions of dy[pos][co] * x[src(pos, tap)][ci].  A workgroup owns a 32 x 32 channel tile and a
//     contiguous run of position tiles (1 x TH x 16); both operands are read transposed out of their channels-last LDS images
//     (ds_read_b64_tr_b16), the 27 taps are 27 accumulators of the wave's 16 x 16 channel pair.  Runs write fp32 partials to the workspace and a
//     second kernel adds them in run order: no atomics, the same bits every call.
#include "vt_common.h"

namespace {

constexpr int SLAB = 32;          // source channels per LDS brick (one MFMA k-step)
constexpr int ROWB = SLAB * 2;    // bytes of one brick position

struct ConvGeom {
    int B, Ts, Hs, Ws, To, Ho, Wo;   // source (read through the brick) and output extents
    int K, N, nslab, nfrag;          // source / output channels, K slabs of 32, N fragments of 16
    int at, ah, aw, dt, dh, dw;      // idx = o * a + k - 1, used when idx % d == 0 at idx / d
    int bt, bh, bw;                  // brick extents (positions)
    int tilesT, tilesH, tilesW, tilesN;
};

__device__ __forceinline__ int brick_origin(int o0, int a, int d) { return (o0 * a - 1 + d - 1) / d; }   // ceil((o0 * a - 1) / d); only d = 1 sees -1
__device__ __forceinline__ unsigned brick_off(int pos, int chunk) { return (unsigned)pos * ROWB + ((chunk ^ ((pos >> 2) & 3)) << 4); }

template <int TT, int TH, int NF>
__global__ __launch_bounds__(256) void conv3d_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
                                                     const bf16_t* __restrict__ res, bf16_t* __restrict__ out, const ConvGeom g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = TT * TH / 4;
    const int npos = g.bt * g.bh * g.bw;
    char* brick = smem;
    char* wl = smem + (size_t)npos * ROWB;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;

    int r = blockIdx.x;
    const int nt = r % g.tilesN; r /= g.tilesN;
    const int wt = r % g.tilesW; r /= g.tilesW;
    const int ht = r % g.tilesH; r /= g.tilesH;
    const int tt = r % g.tilesT;
    const int b = r / g.tilesT;
    const int o0t = tt * TT, o0h = ht * TH, o0w = wt * 16;
    const int org_t = brick_origin(o0t, g.at, g.dt), org_h = brick_origin(o0h, g.ah, g.dh), org_w = brick_origin(o0w, g.aw, g.dw);

    // this lane's position along w: per kw, the brick column or -1 when the tap is masked
    int bwi[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
        const int idx = (o0w + li) * g.aw + kw - 1;
        bwi[kw] = (o0w + li < g.Wo && idx % g.dw == 0) ? idx / g.dw - org_w : -1;
    }

    f32x4 acc[MF][NF];
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int slab = 0; slab < g.nslab; ++slab) {
        __syncthreads();   // the previous slab's readers are done with the brick
        for (int idx = tid; idx < npos * 4; idx += 256) {
            const int pos = idx >> 2, ch = idx & 3;
            const int wi = pos % g.bw;
            const int q = pos / g.bw;
            const int hi = q % g.bh, ti = q / g.bh;
            const int st = org_t + ti, sh = org_h + hi, sw = org_w + wi, c = slab * SLAB + ch * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (st >= 0 && st < g.Ts && sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws && c < g.K)
                v = *(const bf16x8*)(x + ((((int64_t)b * g.Ts + st) * g.Hs + sh) * g.Ws + sw) * g.K + c);
            *(bf16x8*)(brick + brick_off(pos, ch)) = v;
        }
        for (int kth = 0; kth < 9; ++kth) {
            const int kt = kth / 3, kh = kth % 3;
            __syncthreads();   // brick visible; the previous row's weight readers are done
            {
                const bf16_t* src = wp + (((int64_t)slab * 27 + kth * 3) * g.nfrag + nt * NF) * 512;
                for (int idx = tid; idx < 3 * NF * 64; idx += 256) {
                    const int kw = idx / (NF * 64), rem = idx % (NF * 64);
                    *(bf16x8*)(wl + (size_t)idx * 16) = *(const bf16x8*)(src + (int64_t)kw * g.nfrag * 512 + rem * 8);
                }
            }
            __syncthreads();
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                bf16x8 wf[NF];
#pragma unroll
                for (int n = 0; n < NF; ++n) wf[n] = *(const bf16x8*)(wl + ((kw * NF + n) * 64 + lane) * 16);
#pragma unroll
                for (int m = 0; m < MF; ++m) {
                    const int f = wave * MF + m, ft = f / TH, fh = f % TH;
                    const int it = (o0t + ft) * g.at + kt - 1, ih = (o0h + fh) * g.ah + kh - 1;
                    if (o0t + ft >= g.To || o0h + fh >= g.Ho || it % g.dt != 0 || ih % g.dh != 0) continue;   // wave-uniform
                    const int pos = ((it / g.dt - org_t) * g.bh + (ih / g.dh - org_h)) * g.bw + bwi[kw];
                    bf16x8 xf = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (bwi[kw] >= 0) xf = *(const bf16x8*)(brick + brick_off(pos, lg));
#pragma unroll
                    for (int n = 0; n < NF; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], xf, acc[m][n], 0, 0, 0);
                }
            }
        }
    }

    // epilogue: lane = position li of the fragment's row, output channels 4 * lg .. + 3 of each N fragment
    const int ow = o0w + li;
#pragma unroll
    for (int m = 0; m < MF; ++m) {
        const int f = wave * MF + m, ot = o0t + f / TH, oh = o0h + f % TH;
        if (ot >= g.To || oh >= g.Ho || ow >= g.Wo) continue;
        const int64_t row = (((int64_t)b * g.To + ot) * g.Ho + oh) * g.Wo + ow;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const int co = (nt * NF + n) * 16 + lg * 4;
            f32x4 v = acc[m][n];
            if (bias) {
                const f32x4 bv = *(const f32x4*)(bias + co);
                v += bv;
            }
            bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
            if (res) {
                const bf16x4 rv = *(const bf16x4*)(res + row * g.N + co);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = f2bf(bf2f(o[j]) + bf2f(rv[j]));
            }
            *(bf16x4*)(out + row * g.N + co) = o;
        }
    }
}

// fp32 [Cout, Cin, 27] -> the operand image of conv3d_kernel: [K slab][tap][N fragment][lane][8], element = the A operand of the MFMA
// (row n = 16 * frag + (lane & 15), k = 32 * slab + 8 * (lane >> 4) + j); zeros where n or k is past the parameter's own extent.
// for_dgrad: n runs over Cin, k over Cout, and the taps are mirrored (tap 26 - t).
__global__ __launch_bounds__(256) void conv3d_pack_kernel(const float* __restrict__ w, int Cout, int Cin, int nfrag, int64_t total, int for_dgrad,
                                                          bf16_t* __restrict__ packed) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one lane's 8 elements
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    int64_t r = idx >> 6;
    const int frag = (int)(r % nfrag); r /= nfrag;
    const int tap = (int)(r % 27);
    const int slab = (int)(r / 27);
    const int n = frag * 16 + (lane & 15), k0 = slab * SLAB + 8 * (lane >> 4);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        const int co = for_dgrad ? k : n, ci = for_dgrad ? n : k, t = for_dgrad ? 26 - tap : tap;
        o[j] = (co < Cout && ci < Cin) ? f2bf(w[((int64_t)co * Cin + ci) * 27 + t]) : f2bf(0.f);
    }
    *(bf16x8*)(packed + idx * 8) = o;
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------
struct WGeom {
    int B, T, H, W, To, Ho, Wo, Cin, Cout, st, sh, sw;
    int bh, bw;                    // brick extents in h and w (3 planes in t)
    int tilesH, tilesW;
    int64_t npt, per;              // position tiles, tiles per run
    int tilesCo, tilesCi, cout_lim, cin_lim;
};

// one 16 x 32 operand of the 16x16x32 MFMA read transposed out of a channels-last image: lane (g = l >> 4, i = l & 15) gets
// image[row(8g + 0..7)][col + i]; the caller gives the byte address of rows 8g + q and 8g + q + 4 (q = i >> 2)
__device__ __forceinline__ bf16x8 frag_tr(const char* row_lo, const char* row_hi, int col, int lane) {
    const int pp = lane & 3;
    return cat4(lds_read_tr16(row_lo + (col + 4 * pp) * 2), lds_read_tr16(row_hi + (col + 4 * pp) * 2));
}

template <int TH>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part,
                                                           const WGeom g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NPOS = TH * 16;
    char* dyl = smem;                       // [NPOS][32 co]
    char* brick = smem + NPOS * ROWB;       // [3][bh][bw][32 ci]
    const int nbrick = 3 * g.bh * g.bw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4, q = li >> 2;
    const int wco = wave >> 1, wci = wave & 1;

    int r = blockIdx.x;
    const int cit = r % g.tilesCi; r /= g.tilesCi;
    const int cot = r % g.tilesCo;
    const int run = r / g.tilesCo;
    const int co0 = cot * 32, ci0 = cit * 32;

    f32x4 acc[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int64_t p_begin = run * g.per, p_end = p_begin + g.per < g.npt ? p_begin + g.per : g.npt;
    for (int64_t pt = p_begin; pt < p_end; ++pt) {
        int64_t rr = pt;
        const int wt = (int)(rr % g.tilesW); rr /= g.tilesW;
        const int ht = (int)(rr % g.tilesH); rr /= g.tilesH;
        const int ot = (int)(rr % g.To);
        const int b = (int)(rr / g.To);
        const int o0h = ht * TH, o0w = wt * 16;
        const int org_t = ot * g.st - 1, org_h = o0h * g.sh - 1, org_w = o0w * g.sw - 1;
        __syncthreads();   // the previous tile's readers are done
        for (int idx = tid; idx < NPOS * 4; idx += 256) {
            const int pos = idx >> 2, ch = idx & 3;
            const int oh = o0h + (pos >> 4), ow = o0w + (pos & 15), c = co0 + ch * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (oh < g.Ho && ow < g.Wo && c < g.Cout)
                v = *(const bf16x8*)(dy + ((((int64_t)b * g.To + ot) * g.Ho + oh) * g.Wo + ow) * g.Cout + c);
            *(bf16x8*)(dyl + pos * ROWB + ch * 16) = v;
        }
        for (int idx = tid; idx < nbrick * 4; idx += 256) {
            const int pos = idx >> 2, ch = idx & 3;
            const int wi = pos % g.bw;
            const int qq = pos / g.bw;
            const int hi = qq % g.bh, ti = qq / g.bh;
            const int st = org_t + ti, sh = org_h + hi, sw = org_w + wi, c = ci0 + ch * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (st >= 0 && st < g.T && sh >= 0 && sh < g.H && sw >= 0 && sw < g.W && c < g.Cin)
                v = *(const bf16x8*)(x + ((((int64_t)b * g.T + st) * g.H + sh) * g.W + sw) * g.Cin + c);
            *(bf16x8*)(brick + pos * ROWB + ch * 16) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < TH / 2; ++ks) {
            // the k-step's 32 positions: rows 2ks and 2ks + 1 of the tile; this lane addresses positions 8 lg + q and + 4
            const int p_lo = ks * 32 + 8 * lg + q, p_hi = p_lo + 4;
            const bf16x8 dyf = frag_tr(dyl + p_lo * ROWB, dyl + p_hi * ROWB, wco * 16, lane);
            const int h_lo = (p_lo >> 4) * g.sh, w_lo = (p_lo & 15) * g.sw, h_hi = (p_hi >> 4) * g.sh, w_hi = (p_hi & 15) * g.sw;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int b_lo = ((kt * g.bh) + h_lo + kh) * g.bw + w_lo + kw, b_hi = ((kt * g.bh) + h_hi + kh) * g.bw + w_hi + kw;
                        const bf16x8 xf = frag_tr(brick + b_lo * ROWB, brick + b_hi * ROWB, wci * 16, lane);
                        acc[(kt * 3 + kh) * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dyf, xf, acc[(kt * 3 + kh) * 3 + kw], 0, 0, 0);
                    }
        }
    }
    // D[row = co 4 lg + reg][col = ci li]
    const int ci = ci0 + wci * 16 + li;
    float* dst = part + (int64_t)run * g.cout_lim * g.cin_lim * 27;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int co = co0 + wco * 16 + lg * 4 + reg;
        if (co < g.cout_lim && ci < g.cin_lim) {
#pragma unroll
            for (int t = 0; t < 27; ++t) dst[((int64_t)co * g.cin_lim + ci) * 27 + t] = acc[t][reg];
        }
    }
}

__global__ __launch_bounds__(256) void conv3d_wgrad_merge_kernel(const float* __restrict__ part, int nrun, int64_t n, float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = part[e];
    for (int r = 1; r < nrun; ++r) s += part[(int64_t)r * n + e];
    dw[e] = s;
}

// ---- nearest-neighbour upsampling and the layout pair ---------------------------------------------------------------------------------------
struct UpGeom {
    int B, T, H, W, C8, ft, fh, fw;   // source extents, channels / 8, factors
    int64_t total;
};

__global__ __launch_bounds__(256) void upsample_fwd_kernel(const bf16x8* __restrict__ x, bf16x8* __restrict__ out, const UpGeom g) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one 16-byte piece of the OUTPUT
    if (idx >= g.total) return;
    const int c = (int)(idx % g.C8);
    int64_t r = idx / g.C8;
    const int w = (int)(r % (g.W * g.fw)); r /= g.W * g.fw;
    const int h = (int)(r % (g.H * g.fh)); r /= g.H * g.fh;
    const int t = (int)(r % (g.T * g.ft));
    const int64_t b = r / (g.T * g.ft);
    out[idx] = x[(((b * g.T + t / g.ft) * g.H + h / g.fh) * g.W + w / g.fw) * g.C8 + c];
}

__global__ __launch_bounds__(256) void upsample_bwd_kernel(const bf16x8* __restrict__ dout, bf16x8* __restrict__ dx, const UpGeom g) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one 16-byte piece of the SOURCE
    if (idx >= g.total) return;
    const int c = (int)(idx % g.C8);
    int64_t r = idx / g.C8;
    const int w = (int)(r % g.W); r /= g.W;
    const int h = (int)(r % g.H); r /= g.H;
    const int t = (int)(r % g.T);
    const int64_t b = r / g.T;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int dt = 0; dt < g.ft; ++dt)
        for (int dh = 0; dh < g.fh; ++dh)
            for (int dw = 0; dw < g.fw; ++dw) {
                const bf16x8 v = dout[(((b * g.T * g.ft + t * g.ft + dt) * (g.H * g.fh) + h * g.fh + dh) * (int64_t)(g.W * g.fw) + w * g.fw + dw) * g.C8 + c];
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += bf2f(v[j]);
            }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(s[j]);
    dx[idx] = o;
}

// fp32 [B, C, T, H, W] -> bf16 [B, T, H, W, Cp] (channels C .. Cp - 1 zero) and back; a thread per position
__global__ __launch_bounds__(256) void video_to_cl_kernel(const float* __restrict__ v, int C, int Cp, int64_t thw, int64_t total, bf16_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t b = idx / thw, p = idx % thw;
    for (int c0 = 0; c0 < Cp; c0 += 8) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = c0 + j < C ? f2bf(v[(b * C + c0 + j) * thw + p]) : f2bf(0.f);
        *(bf16x8*)(out + idx * Cp + c0) = o;
    }
}

__global__ __launch_bounds__(256) void cl_to_video_kernel(const bf16_t* __restrict__ x, int C, int Cp, int64_t thw, int64_t total, float* __restrict__ v) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t b = idx / thw, p = idx % thw;
    for (int c0 = 0; c0 < C; c0 += 8) {
        const bf16x8 in = *(const bf16x8*)(x + idx * Cp + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < C) v[(b * C + c0 + j) * thw + p] = bf2f(in[j]);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
bool stride_ok(int st, int sh, int sw) { return (st == 1 && sh == 1 && sw == 1) || (st == 1 && sh == 2 && sw == 2) || (st == 2 && sh == 2 && sw == 2); }
int out_extent(int n, int s) { return (n - 1) / s + 1; }

// what the three products ask of a problem; T, H, W are the INPUT extents of the convolution
int check_problem(const char* who, int B, int T, int H, int W, int Cin, int Cout, int st, int sh, int sw) {
    VT_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "%s: bad size B=%d T=%d H=%d W=%d", who, B, T, H, W);
    VT_CHECK_ARG(Cin > 0 && Cin % 16 == 0 && Cin <= 1024, "%s: Cin=%d must be a multiple of 16 in 16..1024", who, Cin);
    VT_CHECK_ARG(Cout > 0 && Cout % 16 == 0 && Cout <= 1024, "%s: Cout=%d must be a multiple of 16 in 16..1024", who, Cout);
    VT_CHECK_ARG(stride_ok(st, sh, sw), "%s: stride (%d,%d,%d) is none of (1,1,1), (1,2,2), (2,2,2)", who, st, sh, sw);
    return VT_OK;
}

template <int TT, int TH, int NF>
int launch_conv(const char* who, const ConvGeom& g0, const void* x, const void* wp, const float* bias, const void* res, void* out, vtStream stream) {
    ConvGeom g = g0;
    auto ext = [](int n, int a, int d) { return d == 1 ? (n - 1) * a + 3 : n / 2 + 2; };
    g.bt = ext(TT, g.at, g.dt), g.bh = ext(TH, g.ah, g.dh), g.bw = ext(16, g.aw, g.dw);
    g.tilesT = (g.To + TT - 1) / TT, g.tilesH = (g.Ho + TH - 1) / TH, g.tilesW = (g.Wo + 15) / 16, g.tilesN = g.N / (16 * NF);
    const size_t lds = (size_t)g.bt * g.bh * g.bw * ROWB + 3 * NF * 1024;
    VT_CHECK_ARG(lds <= 65536, "%s: tile needs %zu bytes of LDS", who, lds);
    const int64_t blocks = (int64_t)g.B * g.tilesT * g.tilesH * g.tilesW * g.tilesN;
    VT_CHECK_ARG(blocks <= 0x7fffffff, "%s: B=%d To=%d Ho=%d Wo=%d N=%d is too large for one launch", who, g.B, g.To, g.Ho, g.Wo, g.N);
    hipLaunchKernelGGL((conv3d_kernel<TT, TH, NF>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)wp, bias,
                       (const bf16_t*)res, (bf16_t*)out, g);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

template <int TT, int TH>
int launch_conv_nf(const char* who, const ConvGeom& g, const void* x, const void* wp, const float* bias, const void* res, void* out, vtStream stream) {
    if (g.N % 64 == 0) return launch_conv<TT, TH, 4>(who, g, x, wp, bias, res, out, stream);
    if (g.N % 32 == 0) return launch_conv<TT, TH, 2>(who, g, x, wp, bias, res, out, stream);
    return launch_conv<TT, TH, 1>(who, g, x, wp, bias, res, out, stream);
}

int run_conv(const char* who, ConvGeom& g, const void* x, const void* wp, const float* bias, const void* res, void* out, vtStream stream) {
    g.nslab = (g.K + SLAB - 1) / SLAB, g.nfrag = g.N / 16;
    // a strided forward reads a brick of (n - 1) * s + 3 positions per axis: a small tile keeps it in LDS
    if (g.at == 1 && g.ah == 1 && g.aw == 1) return launch_conv_nf<2, 8>(who, g, x, wp, bias, res, out, stream);
    return launch_conv_nf<2, 2>(who, g, x, wp, bias, res, out, stream);
}

struct WPlan {
    WGeom g;
    int nrun;
    int th;
    size_t lds;
};

void plan_wgrad(WPlan& p, int B, int T, int H, int W, int Cin, int Cout, int st, int sh, int sw, int cout_lim, int cin_lim) {
    WGeom& g = p.g;
    g.B = B, g.T = T, g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.st = st, g.sh = sh, g.sw = sw;
    g.To = out_extent(T, st), g.Ho = out_extent(H, sh), g.Wo = out_extent(W, sw);
    p.th = (sh == 1 && sw == 1) ? 8 : 2;
    g.bh = (p.th - 1) * sh + 3, g.bw = 15 * sw + 3;
    g.tilesH = (g.Ho + p.th - 1) / p.th, g.tilesW = (g.Wo + 15) / 16;
    g.npt = (int64_t)B * g.To * g.tilesH * g.tilesW;
    g.tilesCo = (Cout + 31) / 32, g.tilesCi = (Cin + 31) / 32;
    g.cout_lim = cout_lim, g.cin_lim = cin_lim;
    // runs: enough workgroups to fill the chip twice, as a function of the shape alone
    const int64_t ct = (int64_t)g.tilesCo * g.tilesCi;
    int64_t want = 512 / ct;
    if (want < 1) want = 1;
    if (want > g.npt) want = g.npt;
    g.per = (g.npt + want - 1) / want;
    p.nrun = (int)((g.npt + g.per - 1) / g.per);
    p.lds = (size_t)p.th * 16 * ROWB + (size_t)3 * g.bh * g.bw * ROWB;
}

int up_geom(const char* who, UpGeom& g, const void* a, const void* b, int B, int T, int H, int W, int C, int ft, int fh, int fw, bool by_output) {
    VT_CHECK_ARG(a != nullptr && b != nullptr, "%s: a tensor is null", who);
    VT_CHECK_ARG(aligned16(a) && aligned16(b), "%s: a tensor (%p, %p) is not 16-byte aligned", who, a, b);
    VT_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "%s: bad size B=%d T=%d H=%d W=%d", who, B, T, H, W);
    VT_CHECK_ARG(C > 0 && C % 16 == 0 && C <= 1024, "%s: C=%d must be a multiple of 16 in 16..1024", who, C);
    VT_CHECK_ARG((ft == 1 || ft == 2) && fh == 2 && fw == 2, "%s: scale (%d,%d,%d) is neither (2,2,2) nor (1,2,2)", who, ft, fh, fw);
    g.B = B, g.T = T, g.H = H, g.W = W, g.C8 = C / 8, g.ft = ft, g.fh = fh, g.fw = fw;
    g.total = (int64_t)B * T * H * W * g.C8 * (by_output ? ft * fh * fw : 1);
    VT_CHECK_ARG((g.total + 255) / 256 <= 0x7fffffff, "%s: B=%d T=%d H=%d W=%d C=%d is too large for one launch", who, B, T, H, W, C);
    return VT_OK;
}

int layout_check(const char* who, const void* video, const void* cl, int B, int C, int T, int H, int W, int Cp, int64_t& thw, int64_t& total) {
    VT_CHECK_ARG(video != nullptr && cl != nullptr, "%s: video or the channels-last tensor is null", who);
    VT_CHECK_ARG(aligned16(cl), "%s: the channels-last tensor (%p) is not 16-byte aligned", who, cl);
    VT_CHECK_ARG(B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "%s: bad size B=%d C=%d T=%d H=%d W=%d", who, B, C, T, H, W);
    VT_CHECK_ARG(Cp >= C && Cp % 16 == 0 && Cp <= 1024, "%s: Cpad=%d must be a multiple of 16, >= C=%d and <= 1024", who, Cp, C);
    thw = (int64_t)T * H * W, total = thw * B;
    VT_CHECK_ARG((total + 255) / 256 <= 0x7fffffff, "%s: B=%d T=%d H=%d W=%d is too large for one launch", who, B, T, H, W);
    return VT_OK;
}

}  // namespace

extern "C" size_t vt_conv3d_packed_elems(int32_t n_abi, int32_t k_abi) {
    if (n_abi <= 0 || k_abi <= 0) return 0;
    return (size_t)27 * ((size_t)(n_abi + 15) / 16 * 16) * ((size_t)(k_abi + SLAB - 1) / SLAB * SLAB);
}

extern "C" int vt_conv3d_pack_weight(const float* w, int32_t Cout, int32_t Cin, int32_t cout_abi, int32_t cin_abi, int32_t for_dgrad, void* packed_bf16,
                                     vtStream stream) {
    const char* who = "vt_conv3d_pack_weight";
    VT_CHECK_ARG(w != nullptr && packed_bf16 != nullptr, "%s: w or packed is null", who);
    VT_CHECK_ARG(aligned16(packed_bf16), "%s: packed (%p) is not 16-byte aligned", who, packed_bf16);
    VT_CHECK_ARG(Cout > 0 && Cin > 0, "%s: bad size Cout=%d Cin=%d", who, Cout, Cin);
    VT_CHECK_ARG(cout_abi >= Cout && cout_abi % 16 == 0 && cout_abi <= 1024, "%s: cout_abi=%d must be a multiple of 16, >= Cout=%d and <= 1024", who, cout_abi, Cout);
    VT_CHECK_ARG(cin_abi >= Cin && cin_abi % 16 == 0 && cin_abi <= 1024, "%s: cin_abi=%d must be a multiple of 16, >= Cin=%d and <= 1024", who, cin_abi, Cin);
    VT_CHECK_ARG(for_dgrad == 0 || for_dgrad == 1, "%s: for_dgrad=%d is neither 0 nor 1", who, for_dgrad);
    const int n = for_dgrad ? cin_abi : cout_abi, k = for_dgrad ? cout_abi : cin_abi;
    const int nfrag = n / 16, nslab = (k + SLAB - 1) / SLAB;
    const int64_t total = (int64_t)nslab * 27 * nfrag * 64;
    hipLaunchKernelGGL(conv3d_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, nfrag, total, for_dgrad,
                       (bf16_t*)packed_bf16);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_conv3d_fwd(const void* x_bf16, const void* w_packed, const float* bias, const void* residual_bf16, int32_t B, int32_t T, int32_t H,
                             int32_t W, int32_t Cin, int32_t Cout, int32_t st, int32_t sh, int32_t sw, void* out_bf16, vtStream stream) {
    const char* who = "vt_conv3d_fwd";
    VT_CHECK_ARG(x_bf16 != nullptr && w_packed != nullptr && bias != nullptr && out_bf16 != nullptr, "%s: x, w_packed, bias or out is null", who);
    VT_CHECK_ARG(aligned16(x_bf16) && aligned16(w_packed) && aligned16(bias) && aligned16(out_bf16) && aligned16(residual_bf16),
                 "%s: a tensor is not 16-byte aligned (x %p, w %p, bias %p, residual %p, out %p)", who, x_bf16, w_packed, (const void*)bias, residual_bf16,
                 out_bf16);
    TRY(check_problem(who, B, T, H, W, Cin, Cout, st, sh, sw));
    ConvGeom g{};
    g.B = B, g.Ts = T, g.Hs = H, g.Ws = W, g.To = out_extent(T, st), g.Ho = out_extent(H, sh), g.Wo = out_extent(W, sw);
    g.K = Cin, g.N = Cout, g.at = st, g.ah = sh, g.aw = sw, g.dt = g.dh = g.dw = 1;
    return run_conv(who, g, x_bf16, w_packed, bias, residual_bf16, out_bf16, stream);
}

extern "C" int vt_conv3d_dgrad(const void* dy_bf16, const void* w_packed_dgrad, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                               int32_t st, int32_t sh, int32_t sw, void* dx_bf16, vtStream stream) {
    const char* who = "vt_conv3d_dgrad";
    VT_CHECK_ARG(dy_bf16 != nullptr && w_packed_dgrad != nullptr && dx_bf16 != nullptr, "%s: dy, w_packed_dgrad or dx is null", who);
    VT_CHECK_ARG(aligned16(dy_bf16) && aligned16(w_packed_dgrad) && aligned16(dx_bf16), "%s: a tensor is not 16-byte aligned (dy %p, w %p, dx %p)", who,
                 dy_bf16, w_packed_dgrad, dx_bf16);
    TRY(check_problem(who, B, T, H, W, Cin, Cout, st, sh, sw));
    ConvGeom g{};
    g.B = B, g.Ts = out_extent(T, st), g.Hs = out_extent(H, sh), g.Ws = out_extent(W, sw), g.To = T, g.Ho = H, g.Wo = W;
    g.K = Cout, g.N = Cin, g.at = g.ah = g.aw = 1, g.dt = st, g.dh = sh, g.dw = sw;
    return run_conv(who, g, dy_bf16, w_packed_dgrad, nullptr, nullptr, dx_bf16, stream);
}

extern "C" size_t vt_conv3d_wgrad_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t st, int32_t sh,
                                                  int32_t sw, int32_t cout_lim, int32_t cin_lim) {
    if (check_problem("vt_conv3d_wgrad_workspace_bytes", B, T, H, W, Cin, Cout, st, sh, sw) != VT_OK) return 0;
    if (cout_lim <= 0 || cout_lim > Cout || cin_lim <= 0 || cin_lim > Cin) return 0;
    WPlan p;
    plan_wgrad(p, B, T, H, W, Cin, Cout, st, sh, sw, cout_lim, cin_lim);
    return (size_t)p.nrun * cout_lim * cin_lim * 27 * sizeof(float);
}

extern "C" int vt_conv3d_wgrad(const void* x_bf16, const void* dy_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t st,
                               int32_t sh, int32_t sw, int32_t cout_lim, int32_t cin_lim, float* dw, void* workspace, vtStream stream) {
    const char* who = "vt_conv3d_wgrad";
    VT_CHECK_ARG(x_bf16 != nullptr && dy_bf16 != nullptr && dw != nullptr && workspace != nullptr, "%s: x, dy, dw or workspace is null", who);
    VT_CHECK_ARG(aligned16(x_bf16) && aligned16(dy_bf16) && aligned16(workspace), "%s: a tensor is not 16-byte aligned (x %p, dy %p, workspace %p)", who,
                 x_bf16, dy_bf16, workspace);
    TRY(check_problem(who, B, T, H, W, Cin, Cout, st, sh, sw));
    VT_CHECK_ARG(cout_lim > 0 && cout_lim <= Cout, "%s: cout_lim=%d outside 1..Cout=%d", who, cout_lim, Cout);
    VT_CHECK_ARG(cin_lim > 0 && cin_lim <= Cin, "%s: cin_lim=%d outside 1..Cin=%d", who, cin_lim, Cin);
    WPlan p;
    plan_wgrad(p, B, T, H, W, Cin, Cout, st, sh, sw, cout_lim, cin_lim);
    VT_CHECK_ARG(p.lds <= 65536, "%s: tile needs %zu bytes of LDS", who, p.lds);
    const int64_t blocks = (int64_t)p.nrun * p.g.tilesCo * p.g.tilesCi;
    VT_CHECK_ARG(blocks <= 0x7fffffff, "%s: too many workgroups (%lld)", who, (long long)blocks);
    if (p.th == 8)
        hipLaunchKernelGGL(conv3d_wgrad_kernel<8>, dim3((unsigned)blocks), dim3(256), p.lds, (hipStream_t)stream, (const bf16_t*)x_bf16, (const bf16_t*)dy_bf16,
                           (float*)workspace, p.g);
    else
        hipLaunchKernelGGL(conv3d_wgrad_kernel<2>, dim3((unsigned)blocks), dim3(256), p.lds, (hipStream_t)stream, (const bf16_t*)x_bf16, (const bf16_t*)dy_bf16,
                           (float*)workspace, p.g);
    VT_CHECK_LAUNCH(who);
    const int64_t n = (int64_t)cout_lim * cin_lim * 27;
    hipLaunchKernelGGL(conv3d_wgrad_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, p.nrun, n, dw);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_upsample_nearest_fwd(const void* x_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t ft, int32_t fh, int32_t fw,
                                       void* out_bf16, vtStream stream) {
    UpGeom g;
    TRY(up_geom("vt_upsample_nearest_fwd", g, x_bf16, out_bf16, B, T, H, W, C, ft, fh, fw, true));
    hipLaunchKernelGGL(upsample_fwd_kernel, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16x8*)x_bf16, (bf16x8*)out_bf16, g);
    VT_CHECK_LAUNCH("vt_upsample_nearest_fwd");
    return VT_OK;
}

extern "C" int vt_upsample_nearest_bwd(const void* dout_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t ft, int32_t fh, int32_t fw,
                                       void* dx_bf16, vtStream stream) {
    UpGeom g;
    TRY(up_geom("vt_upsample_nearest_bwd", g, dout_bf16, dx_bf16, B, T, H, W, C, ft, fh, fw, false));
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16x8*)dout_bf16, (bf16x8*)dx_bf16, g);
    VT_CHECK_LAUNCH("vt_upsample_nearest_bwd");
    return VT_OK;
}

extern "C" int vt_video_to_channels_last(const float* video, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t Cpad, void* out_bf16,
                                         vtStream stream) {
    int64_t thw, total;
    TRY(layout_check("vt_video_to_channels_last", video, out_bf16, B, C, T, H, W, Cpad, thw, total));
    hipLaunchKernelGGL(video_to_cl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, video, C, Cpad, thw, total, (bf16_t*)out_bf16);
    VT_CHECK_LAUNCH("vt_video_to_channels_last");
    return VT_OK;
}

extern "C" int vt_channels_last_to_video(const void* x_bf16, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t Cpad, float* video,
                                         vtStream stream) {
    int64_t thw, total;
    TRY(layout_check("vt_channels_last_to_video", video, x_bf16, B, C, T, H, W, Cpad, thw, total));
    hipLaunchKernelGGL(cl_to_video_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x_bf16, C, Cpad, thw, total, video);
    VT_CHECK_LAUNCH("vt_channels_last_to_video");
    return VT_OK;
}
