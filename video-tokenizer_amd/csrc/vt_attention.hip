// Fused multi-head attention (no mask, head_dim 64 or 32) for gfx950: forward with online softmax and the
// two recompute backward kernels.  Replaces timm Attention's F.scaled_dot_product_attention inside
// timm Block (constructed at /root/reference/models/transformer.py:52-59) and its autograd.
//
// Layouts: qkv bf16 [B, L, 3, H, 64] (the qkv Linear's output, reshape (B,N,3,H,hd)); o / dO bf16
// [B, L, H, 64]; lse2 fp32 [B, H, L] = log2-domain log-sum-exp of the scaled scores; delta fp32 [B,H,L].
// CROSS instantiations (vt_attention_cross_*; CrossAttention of models/model_design/base/transformer.py:92-141): q, k and v are
// three pointers with a row stride each, Lq query rows and Lk key rows per batch; o / dO [B, Lq, H, 64], lse2 / delta [B, H, Lq].
// The same kernels and tile code: a packed launch is the special case q = qkv, k = q + D, v = k + D, every stride 3D, Lq = Lk,
// which the packed instantiations know at compile time (one stride register, one set of staging offsets) and CROSS ones do not.
// Variable-length launches (vt_attention_varlen_*; Attn of models/model_titok/base/transformer.py:32-62, flash_attn_varlen_func): n sequences
// packed one behind the other in [M, ...] operands, Hq query heads over Hkv KV heads, lse2 / delta [Hq, M].  Again the same kernels and tile
// code behind a third address computation (varlen_head_ptrs): a sequence is a batch of one that starts at any row.
//
// Common skeleton (one workgroup = 4 waves, each wave owns 32 "stationary" rows held in registers as
// MFMA B operands; 64-row "streaming" tiles are staged global -> LDS with 16-B global_load_lds,
// double-buffered, one barrier per tile):
//   score-like products  X[stream_row][own_row] = Tile . Own^T      : A = tile rows by ds_read_b128
//   accumulate products  Acc^T[d][own_row]    += Tile^T . X         : A = tile columns by
//                        ds_read_b64_tr_b16; B = the fp32 accumulator X converted to bf16 IN REGISTERS
//                        (a 32x32 accumulator has its column on the lane and its rows in the 16
//                        registers, so registers 8s..8s+7 are the B fragment of k-step s; the k order
//                        inside a step is row 16s + 8(j>>2) + 4*half + (j&3), which the transposed read
//                        of the other operand follows).
// Because the own row (query in fwd/dQ, key in dK/dV) sits on the lane, softmax statistics are
// lane-local: no cross-lane reduction except one exchange between the two lane halves.
//
// LDS tile image: [64 rows][HD bf16].  head_dim 64: 128-B rows of eight 16-B chunks, physical chunk =
// logical ^ f(row), f(row) = (((row>>1)&1)<<2) | ((row>>2)&3); head_dim 32 (the GAN discriminator's heads,
// /root/reference/models/loss.py:119-204 with cfgs/larp_tokenizer.yaml:130-131): 64-B rows of four chunks,
// f(row) = (row>>2)&3.  Both are conflict-free for BOTH the b128 row reads of a 32x32x16 A operand and the
// transposed b64 reads (derivation in DESIGN.md).  The image is written lane-linearly by the LDS-DMA, so the
// XOR goes on the per-lane source address.
#include "vt_common.h"
#include <stdlib.h>

#include <type_traits>

#include "vt_attn_tile.h"

namespace {

// One workgroup's (batch, head, row-block) and the first Q / K / V row of that head.  1-D grid, XCD-aware: the nblk row-blocks of one
// (batch, head) get consecutive ids inside ONE XCD's chunk, so the tiles they all stream (K/V in fwd and dQ, Q/dO in dK/dV) are
// fetched into that XCD's L2 once instead of once per XCD.  Returned BY VALUE: the fields are scalars the kernels keep in SGPRs.
// (id, count): the workgroup's index among the `count` workgroups that share its mapping -- blockIdx.x of gridDim.x in a launch of one
// kind of workgroup, the index within its role in the two-role backward launch (attn_bwd_kernel).
// The operands of a launch (kernel arguments).  Packed: q = qkv [B, L, 3, H, HD] and Lq = L are read, the other fields are not.
struct AttnOps {
    const bf16_t *q, *k, *v;
    int64_t q_rs, k_rs, v_rs;        // row strides (elements)
    int Lq, Lk;                      // rows per batch of q and of k / v
};
// Where the gradients go.  Packed: dq = dqkv, laid out as qkv.
struct AttnGrads {
    bf16_t *dq, *dk, *dv;
    int64_t dq_rs, dk_rs, dv_rs;
};
struct HeadPtrs {
    int blk;
    int Lq, Lk;
    int hq, hkv;                     // head columns of q / dq / o and of k / v / dk / dv (the same head unless the launch is grouped)
    int group;                       // query heads hq .. hq + group - 1 share the KV head: the dK/dV workgroup sweeps them all (1 unless grouped)
    int64_t qrow, krow;              // first row of the workgroup's batch (sequence) in q / dq and in k / v / dk / dv
    int64_t q_rs, k_rs, v_rs, ors;   // row strides (elements) of q, k, v and of o / dO [B, Lq, H, HD]
    int64_t orow;                    // first row of the batch (sequence) in o / dO, which hold the kept queries only
    int64_t st_off, st_hs;           // index of (first query row, head hq) in lse2 / delta, and the distance between two heads there
    const bf16_t *qb, *kb, *vb;
};
template <int HD, bool CROSS>
__device__ __forceinline__ HeadPtrs head_ptrs(const AttnOps& a, int H, int nblk, int q_begin, int id, int count) {
    HeadPtrs p;
    const int sid = xcd_remap(id, count);
    const int bh = sid / nblk;
    p.blk = sid - bh * nblk;
    const int b = bh / H, h = bh % H;
    p.hq = p.hkv = h;
    p.group = 1;
    p.ors = (int64_t)H * HD;
    p.Lq = a.Lq;
    p.qrow = (int64_t)b * p.Lq;
    p.orow = (int64_t)b * (p.Lq - q_begin);
    p.st_off = ((int64_t)b * H + h) * p.Lq;
    p.st_hs = p.Lq;
    if constexpr (CROSS) {
        p.Lk = a.Lk;
        p.krow = (int64_t)b * p.Lk;
        p.q_rs = a.q_rs, p.k_rs = a.k_rs, p.v_rs = a.v_rs;
        p.qb = a.q + p.qrow * p.q_rs + (int64_t)h * HD;
        p.kb = a.k + p.krow * p.k_rs + (int64_t)h * HD;
        p.vb = a.v + p.krow * p.v_rs + (int64_t)h * HD;
    } else {
        p.Lk = p.Lq;
        p.krow = p.qrow;
        p.q_rs = p.k_rs = p.v_rs = (int64_t)3 * H * HD;
        p.qb = a.q + p.qrow * p.q_rs + (int64_t)h * HD;
        p.kb = p.qb + p.ors;
        p.vb = p.kb + p.ors;
    }
    return p;
}

// Packed variable-length launches (vt_attention_varlen_*): n sequences of cu[b+1] - cu[b] rows each, one behind the other in the
// same [M, ...] operands; Hq query heads over Hkv KV heads.  The boundaries and the prefix of 128-row blocks per sequence are KERNEL
// ARGUMENTS (the host validated them; nothing is read from device memory that a caller could leave stale), so the grid is exactly
// blk[n] * heads workgroups and each finds its (head, sequence, block) by a scalar bisection of blk[].
struct SeqTable {
    int n, total;                    // sequences; total = blk[n]
    int cu[VT_VARLEN_MAX_SEQ + 1];   // first row of sequence b; cu[n] = M
    int blk[VT_VARLEN_MAX_SEQ + 1];  // 128-row blocks before sequence b
};
// KV = false: the forward and dQ, one workgroup per (query head, sequence, 128 queries); KV = true: dK/dV, one per (KV head, sequence,
// 128 keys), hq = the first query head of its group.  A sequence is a "batch" of one whose rows start at cu[b]: the tile code clamps
// loads to its last row and masks stores past it exactly as at the end of a dense batch.  Everything the bisection yields is
// wave-uniform and goes through readfirstlane, because the full-tile stagers take the row base as a scalar ("s") operand.
template <int HD, bool KV>
__device__ __forceinline__ HeadPtrs varlen_head_ptrs(const AttnOps& a, const SeqTable& tab, int Hq, int Hkv, int M) {
    HeadPtrs p;
    const int sid = xcd_remap(blockIdx.x, gridDim.x);
    const int h = sid / tab.total;
    const int gb = sid - h * tab.total;
    int lo = 0, hi = tab.n;          // blk[lo] <= gb < blk[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.blk[mid] <= gb) lo = mid;
        else hi = mid;
    }
    const int b = __builtin_amdgcn_readfirstlane(lo);
    const int row0 = __builtin_amdgcn_readfirstlane(tab.cu[b]);
    const int L = __builtin_amdgcn_readfirstlane(tab.cu[b + 1] - row0);
    p.blk = __builtin_amdgcn_readfirstlane(gb - tab.blk[b]);
    p.group = Hq / Hkv;
    p.hq = __builtin_amdgcn_readfirstlane(KV ? h * p.group : h);
    p.hkv = __builtin_amdgcn_readfirstlane(KV ? h : h / p.group);
    p.Lq = p.Lk = L;
    p.qrow = p.krow = row0;
    p.ors = (int64_t)Hq * HD;
    p.q_rs = a.q_rs, p.k_rs = a.k_rs, p.v_rs = a.v_rs;
    p.orow = row0;
    p.st_off = (int64_t)p.hq * M + row0;     // lse2 / delta [Hq, M]
    p.st_hs = M;
    p.qb = a.q + (int64_t)row0 * p.q_rs + (int64_t)p.hq * HD;
    p.kb = a.k + (int64_t)row0 * p.k_rs + (int64_t)p.hkv * HD;
    p.vb = a.v + (int64_t)row0 * p.v_rs + (int64_t)p.hkv * HD;
    return p;
}
// first gradient row of the workgroup's (batch, head) in dq / dk / dv
template <int HD, bool CROSS>
__device__ __forceinline__ AttnGrads grad_ptrs(const AttnGrads& g, const HeadPtrs& hp) {
    AttnGrads r;
    if constexpr (CROSS) {
        r.dq_rs = g.dq_rs, r.dk_rs = g.dk_rs, r.dv_rs = g.dv_rs;
        r.dq = g.dq + hp.qrow * r.dq_rs + (int64_t)hp.hq * HD;
        r.dk = g.dk + hp.krow * r.dk_rs + (int64_t)hp.hkv * HD;
        r.dv = g.dv + hp.krow * r.dv_rs + (int64_t)hp.hkv * HD;
    } else {
        r.dq_rs = r.dk_rs = r.dv_rs = hp.q_rs;
        r.dq = g.dq + hp.qrow * hp.q_rs + (int64_t)hp.hq * HD;
        r.dk = r.dq + hp.ors;
        r.dv = r.dk + hp.ors;
    }
    return r;
}

// K and V tile t into LDS buffer `buf` ([buffer 0: K | V][buffer 1: K | V]) for the forward and dQ sweeps.  koff / voff: the lane
// offsets of stage_offsets for the K and the V stride (packed: one array, V's tile is K's moved by one operand width).
template <int HD, bool CROSS>
__device__ __forceinline__ void stage_kv(const HeadPtrs hp, const unsigned (&koff)[AG<HD>::CH / 4], const unsigned (&voff)[AG<HD>::CH / 4], int t, int buf,
                                         int nfull, unsigned sbase, int tid, int wave) {
    constexpr int TILE = AG<HD>::TILE;
    const unsigned lds = sbase + buf * 2 * TILE;
    if (t < nfull) {              // a full tile: scalar base + invariant lane offsets
        const bf16_t* kt = hp.kb + (int64_t)t * 64 * hp.k_rs;
        stage64_full<HD>(kt, koff, lds, wave);
        if constexpr (CROSS) stage64_full<HD>(hp.vb + (int64_t)t * 64 * hp.v_rs, voff, lds + TILE, wave);
        else stage64_full<HD>(kt + hp.ors, koff, lds + TILE, wave);
    } else {                      // the ragged last tile: clamped rows
        stage64<HD>(hp.kb, hp.k_rs, t * 64, hp.Lk, lds, tid, wave);
        stage64<HD>(hp.vb, hp.v_rs, t * 64, hp.Lk, lds + TILE, tid, wave);
    }
}

// The double-buffered sweep of all three kernels over the streamed tiles t0 .. nt-1 (the first nfull of them full 64-row tiles, at most
// one ragged tile behind them).  The caller has staged tile t0 into buffer 0 and published it; here tile t sits in buffer (t - t0) & 1,
// tile t + 1 is staged while t computes, and one dma_drain + barrier per tile publishes it.  body(ragged, buf, t) is one tile's math.
//   plain : hot loop over full tiles only; the ragged last tile (L % 64 != 0) runs once, after the loop, so its masking code never
//           shares registers with the steady state.  Two tiles per trip so that the LDS buffer of a tile body is a compile-time
//           constant (an instruction immediate, not an add).
//   CAUSAL: every tile goes through body(ragged = true), which itself picks plain / masked / skipped per wave.
template <bool B>
struct BoolTag { static constexpr bool value = B; };
template <bool CAUSAL, class Stage, class Body>
__device__ __forceinline__ void sweep_tiles(int t0, int nt, int nfull, Stage&& stage, Body&& body) {
    if constexpr (CAUSAL) {
        for (int t = t0; t < nt; ++t) {
            const int cur = (t - t0) & 1;
            if (t + 1 < nt) stage(t + 1, cur ^ 1);
            body(BoolTag<true>{}, cur, t);
            dma_drain();
            __syncthreads();
        }
    } else {
        for (int t = t0; t < nfull; t += 2) {
            if (t + 1 < nt) stage(t + 1, 1);
            body(BoolTag<false>{}, 0, t);
            dma_drain();
            __syncthreads();
            if (t + 1 < nfull) {
                if (t + 2 < nt) stage(t + 2, 0);
                body(BoolTag<false>{}, 1, t + 1);
                dma_drain();
                __syncthreads();
            }
        }
        if (nfull < nt) body(BoolTag<true>{}, (nfull - t0) & 1, nfull);
    }
}

// one 64-key tile of the forward: S^T = K.Q^T, online softmax (log2 domain; max taken on the raw scores since
// the scale is positive), O^T += V^T.P^T.  TAIL masks keys >= L (last tile of a ragged sequence only).
// Round 4: fragments from precomputed lane offsets + immediates (TileAddr), and the softmax arithmetic two elements per
// instruction (v_pk_fma_f32 for s * c - m, v_pk_add_f32 for the row sum): 11.6 -> ~7 vector instructions per MFMA.
template <int HD, bool TAIL>
__device__ __forceinline__ void fwd_tile(unsigned kl, unsigned vl, const TileAddr<HD>& ad, const bf16x8 (&qf)[HD / 16], f32x16 (&oacc)[HD / 32],
                                         float& m, float& lsum, int key0, int L, float c, int half) {
    f32x16 sacc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 16; ++s)
            sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag_a<HD>(kl, ad, kt * 32, s), qf[s], sacc[kt], 0, 0, 0);
    }
    float mx = -__builtin_inff();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (TAIL && (key0 + kt * 32 + reg_row(r, half) >= L)) sacc[kt][r] = -__builtin_inff();
            mx = fmaxf(mx, sacc[kt][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    // Lazy rescaling: `m` is the reference point of the exponentials, not necessarily the running maximum.  It moves (and
    // O, l are rescaled) only when some row's maximum has outgrown it by more than 2^8; until then p <= 256 instead of
    // <= 1, harmless in fp32 sums and in bf16 P (relative precision), and lse = m + log2(l) stays exact.  After the first
    // tiles the wave-uniform branch is almost never taken, which removes 16 packed multiplies + an exp per tile.
    const float want = mx * c;
    if (__builtin_amdgcn_ballot_w64(want > m + 8.0f) != 0ull) {
        const float mn = fmaxf(m, want);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // m = -inf on the first tile: alpha = 0, O and l are 0 anyway
        m = mn;
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
    }
    const f32x2 c2 = {c, c}, nm2 = {-m, -m};
    f32x2 ps2 = {0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const f32x2 sv = {sacc[kt][r], sacc[kt][r + 1]};
            const f32x2 t = __builtin_elementwise_fma(sv, c2, nm2);
            const f32x2 pv = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
            ps2 += pv;
            sacc[kt][r] = pv[0];
            sacc[kt][r + 1] = pv[1];
        }
    lsum += ps2[0] + ps2[1];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            const bf16x8 pf = pack8(sacc[kt], sp);
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag_a<HD>(vl, ad, kt * 32, sp, dt), pf, oacc[dt], 0, 0, 0);
        }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// CAUSAL (the AR consumer, models/larp_ar.py:186-190 `is_causal=True`): query q attends keys 0..q.  A workgroup stops at the last
// tile its 128 queries can see; per wave a tile is plain (every key <= every query of the wave), masked (fwd_tile<TAIL> with
// the per-lane limit q + 1 in place of L) or skipped.
// The three kernel bodies ask `heads()` for the workgroup's HeadPtrs: the dense and cross kernels answer with head_ptrs, the packed
// variable-length ones with varlen_head_ptrs (CROSS = true: separate strides); the tile code below does not know which.
template <int HD, bool CAUSAL, bool CROSS, class Heads>
__device__ __forceinline__ void attn_fwd_body(Heads&& heads, bf16_t* __restrict__ o, float* __restrict__ lse2, float scale_log2e, int q_begin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const HeadPtrs hp = heads();
    const int Lq = hp.Lq, Lk = hp.Lk;
    // queries q_begin .. Lq-1 only (q_begin > 0: the last block of a stack, whose other output rows nobody reads); their
    // outputs go to a COMPACT o [B, Lq - q_begin, H, HD]; keys are always all Lk rows; lse2 keeps the full [B, H, Lq] index
    const int q0 = q_begin + hp.blk * 128 + wave * 32;

    constexpr int TILE = AG<HD>::TILE, KS = AG<HD>::KS, DT = AG<HD>::DT;
    bf16x8 qf[KS];
    load_own<KS>(hp.qb, hp.q_rs, q0, Lq, lane, qf);

    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m = -__builtin_inff(), lsum = 0.f;

    const int nt = (Lk + 63) / 64, nfull = (Lk & 63) ? nt - 1 : nt;
    const unsigned sbase = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const TileAddr<HD> ad = tile_addr<HD>(lane, sbase);
    unsigned koff[AG<HD>::CH / 4], voff[CROSS ? AG<HD>::CH / 4 : 1];
    stage_offsets<HD>(hp.k_rs, tid, koff);
    if constexpr (CROSS) stage_offsets<HD>(hp.v_rs, tid, voff);
    auto stage = [&](int t, int buf) __attribute__((always_inline)) {
        if constexpr (CROSS) stage_kv<HD, true>(hp, koff, voff, t, buf, nfull, sbase, tid, wave);
        else stage_kv<HD, false>(hp, koff, koff, t, buf, nfull, sbase, tid, wave);
    };
    stage(0, 0);
    pin_loaded(qf);
    dma_drain();
    __syncthreads();

    const int q_end = min(Lq, q_begin + hp.blk * 128 + 128);          // one past the workgroup's last query
    const int nt_c = CAUSAL ? min(nt, (q_end + 63) / 64) : nt;        // CAUSAL: tiles any of its queries can see
    const int nvis = min(nfull, (q0 + 1) / 64);                       // CAUSAL: tiles with every key <= the wave's first query
    const int lim = min(Lk, q0 + (lane & 31) + 1);                    // CAUSAL: this lane's query sees keys < lim
    sweep_tiles<CAUSAL>(0, nt_c, nfull, stage, [&](auto ragged, int buf, int t) __attribute__((always_inline)) {
        const unsigned kl = buf * 2 * TILE;
        if constexpr (!CAUSAL) fwd_tile<HD, decltype(ragged)::value>(kl, kl + TILE, ad, qf, oacc, m, lsum, t * 64, Lk, scale_log2e, half);
        else if (t < nvis) fwd_tile<HD, false>(kl, kl + TILE, ad, qf, oacc, m, lsum, t * 64, Lk, scale_log2e, half);
        else if (t * 64 <= q0 + 31) fwd_tile<HD, true>(kl, kl + TILE, ad, qf, oacc, m, lsum, t * 64, lim, scale_log2e, half);
    });
    const float ltot = lsum + __shfl_xor(lsum, 32);
    const int q = q0 + (lane & 31);
    const bool ok = q < Lq;
    store_own<DT>(oacc, 1.0f / ltot, o + hp.orow * hp.ors + (int64_t)hp.hq * HD, hp.ors, q - q_begin, ok, half);
    if (ok && half == 0) lse2[hp.st_off + q] = m + __builtin_amdgcn_logf(ltot);  // v_log_f32 = log2
}
template <int HD, bool CAUSAL = false, bool CROSS = false>
__global__ __launch_bounds__(256, CAUSAL ? 3 : 4) void attn_fwd_kernel(const AttnOps ops, bf16_t* __restrict__ o, float* __restrict__ lse2,
                                                           int H, int nblk, float scale_log2e, int q_begin) {
    attn_fwd_body<HD, CAUSAL, CROSS>([&]() __attribute__((always_inline)) { return head_ptrs<HD, CROSS>(ops, H, nblk, q_begin, blockIdx.x, gridDim.x); }, o, lse2, scale_log2e, q_begin);
}
__global__ __launch_bounds__(256, 4) void attn_varlen_fwd_kernel(const AttnOps ops, const SeqTable tab, bf16_t* __restrict__ o,
                                                                 float* __restrict__ lse2, int Hq, int Hkv, int M, float scale_log2e) {
    attn_fwd_body<64, false, true>([&]() __attribute__((always_inline)) { return varlen_head_ptrs<64, false>(ops, tab, Hq, Hkv, M); }, o, lse2, scale_log2e, 0);
}

template <int HD, bool TAIL>
__device__ __forceinline__ void dq_tile(unsigned kl, unsigned vl, const TileAddr<HD>& ad, const bf16x8 (&qf)[HD / 16], const bf16x8 (&dof)[HD / 16],
                                        f32x16 (&dq)[HD / 32], float my_lse, float my_delta, int key0, int L, float c, int half) {
    const f32x2 c2 = {c, c}, nl2 = {-my_lse, -my_lse}, nd2 = {-my_delta, -my_delta};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        f32x16 sacc, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = dp[r] = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 16; ++s) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag_a<HD>(kl, ad, kt * 32, s), qf[s], sacc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag_a<HD>(vl, ad, kt * 32, s), dof[s], dp, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; r += 2) {   // two elements per instruction: v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32
            const f32x2 t = __builtin_elementwise_fma((f32x2){sacc[r], sacc[r + 1]}, c2, nl2);
            f32x2 p = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
            if (TAIL) {
                if (key0 + kt * 32 + reg_row(r, half) >= L) p[0] = 0.f;
                if (key0 + kt * 32 + reg_row(r + 1, half) >= L) p[1] = 0.f;
            }
            const f32x2 ds = p * ((f32x2){dp[r], dp[r + 1]} + nd2);  // dS (unscaled)
            sacc[r] = ds[0];
            sacc[r + 1] = ds[1];
        }
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            const bf16x8 dsf = pack8(sacc, sp);
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
                dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag_a<HD>(kl, ad, kt * 32, sp, dt), dsf, dq[dt], 0, 0, 0);
        }
    }
}

// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d] of a lane's own row from its load_own fragments of O and dO.  ONE expression for both of its
// users (the dQ body and attn_delta_kernel), the 8 * KS products of a lane in this order and then the exchange between the lane halves, so
// that delta has the same bits whichever of them wrote it.
template <int KS>
__device__ __forceinline__ float delta_own(const bf16x8 (&of)[KS], const bf16x8 (&dof)[KS]) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) d += bf2f(of[s][j]) * bf2f(dof[s][j]);
    d += __shfl_xor(d, 32);   // the two lane halves hold the two halves of every 16-wide k-step
    return d;
}

// ------------------------------------------------------------------------------------------------
// dQ: own rows = queries; streams K (row reads + transposed reads) and V (row reads).  OWN_DELTA (the causal and the variable-length
// launches): also produces delta for its own rows (both operands are one 16-B load per k-step away) and leaves it in `delta` for the
// dK/dV kernel, which is launched behind this one.  Otherwise (the dQ role of attn_bwd_kernel) `delta` was filled by attn_delta_kernel
// and is only read here, and `o` is not.
// ------------------------------------------------------------------------------------------------
template <int HD, bool CAUSAL, bool CROSS, bool OWN_DELTA, class Heads>
__device__ __forceinline__ void attn_bwd_dq_body(Heads&& heads, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dO,
                                                 const float* __restrict__ lse2, std::conditional_t<OWN_DELTA, float, const float>* __restrict__ delta,
                                                 const AttnGrads grads, float scale, float scale_log2e, int q_begin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const HeadPtrs hp = heads();
    const int Lq = hp.Lq, Lk = hp.Lk;
    const int q0 = q_begin + hp.blk * 128 + wave * 32;   // kept queries only; o / dO are compact [B, Lq - q_begin, H, HD]
    const int Lo = Lq - q_begin;
    const int q = q0 + (lane & 31);
    const int qc = q < Lq ? q : Lq - 1;

    constexpr int TILE = AG<HD>::TILE, KS = AG<HD>::KS, DT = AG<HD>::DT;
    bf16x8 qf[KS], dof[KS];
    load_own<KS>(hp.qb, hp.q_rs, q0, Lq, lane, qf);
    load_own<KS>(dO + hp.orow * hp.ors + (int64_t)hp.hq * HD, hp.ors, q0 - q_begin, Lo, lane, dof);
    const float my_lse = lse2[hp.st_off + qc];
    float my_delta;
    if constexpr (OWN_DELTA) {
        bf16x8 of[KS];
        load_own<KS>(o + hp.orow * hp.ors + (int64_t)hp.hq * HD, hp.ors, q0 - q_begin, Lo, lane, of);
        my_delta = delta_own<KS>(of, dof);
        if (q < Lq && half == 0) delta[hp.st_off + q] = my_delta;
    } else {
        my_delta = delta[hp.st_off + qc];
    }

    f32x16 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;

    const int nt = (Lk + 63) / 64, nfull = (Lk & 63) ? nt - 1 : nt;
    const unsigned sbase = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const TileAddr<HD> ad = tile_addr<HD>(lane, sbase);
    unsigned koff[AG<HD>::CH / 4], voff[CROSS ? AG<HD>::CH / 4 : 1];
    stage_offsets<HD>(hp.k_rs, tid, koff);
    if constexpr (CROSS) stage_offsets<HD>(hp.v_rs, tid, voff);
    auto stage = [&](int t, int buf) __attribute__((always_inline)) {
        if constexpr (CROSS) stage_kv<HD, true>(hp, koff, voff, t, buf, nfull, sbase, tid, wave);
        else stage_kv<HD, false>(hp, koff, koff, t, buf, nfull, sbase, tid, wave);
    };
    stage(0, 0);
    pin_loaded(qf);
    pin_loaded(dof);
    float lse_pin = my_lse;
    pin_loaded(lse_pin);
    pin_loaded(my_delta);
    dma_drain();
    __syncthreads();

    const int q_end = min(Lq, q_begin + hp.blk * 128 + 128);          // CAUSAL: see attn_fwd_kernel
    const int nt_c = CAUSAL ? min(nt, (q_end + 63) / 64) : nt;
    const int nvis = min(nfull, (q0 + 1) / 64);
    const int lim = min(Lk, q0 + (lane & 31) + 1);
    sweep_tiles<CAUSAL>(0, nt_c, nfull, stage, [&](auto ragged, int buf, int t) __attribute__((always_inline)) {
        const unsigned kl = buf * 2 * TILE;
        if constexpr (!CAUSAL) dq_tile<HD, decltype(ragged)::value>(kl, kl + TILE, ad, qf, dof, dq, lse_pin, my_delta, t * 64, Lk, scale_log2e, half);
        else if (t < nvis) dq_tile<HD, false>(kl, kl + TILE, ad, qf, dof, dq, lse_pin, my_delta, t * 64, Lk, scale_log2e, half);
        else if (t * 64 <= q0 + 31) dq_tile<HD, true>(kl, kl + TILE, ad, qf, dof, dq, lse_pin, my_delta, t * 64, lim, scale_log2e, half);
    });
    const AttnGrads g = grad_ptrs<HD, CROSS>(grads, hp);
    store_own<DT>(dq, scale, g.dq, g.dq_rs, q, q < Lq, half);
}
// The causal backward keeps a launch per kernel: its dK/dV kernel needs the register budget of two waves per SIMD.
__global__ __launch_bounds__(256, 3) void attn_causal_bwd_dq_kernel(const AttnOps ops, const bf16_t* __restrict__ o,
                                                                    const bf16_t* __restrict__ dO, const float* __restrict__ lse2,
                                                                    float* __restrict__ delta, const AttnGrads grads, int H, int nblk,
                                                                    float scale, float scale_log2e) {
    attn_bwd_dq_body<64, true, false, true>([&]() __attribute__((always_inline)) { return head_ptrs<64, false>(ops, H, nblk, 0, blockIdx.x, gridDim.x); }, o, dO, lse2, delta, grads, scale, scale_log2e, 0);
}
__global__ __launch_bounds__(256, 3) void attn_varlen_bwd_dq_kernel(const AttnOps ops, const SeqTable tab, const bf16_t* __restrict__ o,
                                                                    const bf16_t* __restrict__ dO, const float* __restrict__ lse2,
                                                                    float* __restrict__ delta, const AttnGrads grads, int Hq, int Hkv, int M,
                                                                    float scale, float scale_log2e) {
    attn_bwd_dq_body<64, false, true, true>([&]() __attribute__((always_inline)) { return varlen_head_ptrs<64, false>(ops, tab, Hq, Hkv, M); }, o, dO, lse2, delta, grads, scale, scale_log2e, 0);
}

// one 64-query tile of the dK/dV sweep.  LDS buffer: Q tile | dO tile | lse2[64] | delta[64]
template <int HD, bool TAIL, bool CAUSAL = false>
__device__ __forceinline__ void dkv_tile(unsigned qt_l, unsigned lse_a, const TileAddr<HD>& ad, const bf16x8 (&kf)[HD / 16], const bf16x8 (&vf)[HD / 16],
                                         f32x16 (&dk)[HD / 32], f32x16 (&dv)[HD / 32], int q0, int L, float c, int half, int my_key = 0) {
    constexpr int TILE = AG<HD>::TILE;
    const unsigned do_l = qt_l + TILE;
    const unsigned lse_l = lse_a + qt_l + 2 * TILE;      // lse_a = LDS base + 16 * half: this lane's 16 query rows are 4 runs of 4 consecutive rows, qt*32 + 8g + 4*half + 0..3
    const f32x2 nc2 = {-c, -c};
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        f32x16 sacc, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = dp[r] = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 16; ++s) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag_a<HD>(qt_l, ad, qt * 32, s), kf[s], sacc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag_a<HD>(do_l, ad, qt * 32, s), vf[s], dp, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 lse4 = lds_ld128f(lse_l + (qt * 32 + 8 * g) * 4);
            const f32x4 del4 = lds_ld128f(lse_l + 256 + (qt * 32 + 8 * g) * 4);
#pragma unroll
            for (int e = 0; e < 4; e += 2) {   // two elements per instruction
                const int r = 4 * g + e;
                // p = 2^(s c - lse) as 2^-(lse - s c): the row constant enters the packed fma as it comes out of the LDS (negating it
                // first cost a v_xor per element), the sign rides on v_exp_f32's source modifier
                const f32x2 t = __builtin_elementwise_fma((f32x2){sacc[r], sacc[r + 1]}, nc2, (f32x2){lse4[e], lse4[e + 1]});
                f32x2 p = {__builtin_amdgcn_exp2f(-t[0]), __builtin_amdgcn_exp2f(-t[1])};
                if (TAIL) {
                    if (q0 + qt * 32 + reg_row(r, half) >= L) p[0] = 0.f;
                    if (q0 + qt * 32 + reg_row(r + 1, half) >= L) p[1] = 0.f;
                }
                if (CAUSAL) {     // a query never attends a later key
                    if (q0 + qt * 32 + reg_row(r, half) < my_key) p[0] = 0.f;
                    if (q0 + qt * 32 + reg_row(r + 1, half) < my_key) p[1] = 0.f;
                }
                const f32x2 ds = p * ((f32x2){dp[r], dp[r + 1]} - (f32x2){del4[e], del4[e + 1]});
                sacc[r] = p[0];
                sacc[r + 1] = p[1];
                dp[r] = ds[0];
                dp[r + 1] = ds[1];
            }
        }
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            const bf16x8 pf = pack8(sacc, sp);
            const bf16x8 dsf = pack8(dp, sp);
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt) {
                dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag_a<HD>(do_l, ad, qt * 32, sp, dt), pf, dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag_a<HD>(qt_l, ad, qt * 32, sp, dt), dsf, dk[dt], 0, 0, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dK, dV: own rows = keys; streams Q and dO tiles (both row reads and transposed reads) + lse2/delta
// ------------------------------------------------------------------------------------------------
// GROUPED (the variable-length launches): the workgroup's keys belong to one KV head that hp.group query heads read.  It sweeps those
// heads in ascending order, ascending query tiles within a head, into the same fp32 accumulators and rounds once: no atomics, no sum
// across workgroups, the same bits on every run; with one head per group this is the plain sweep.
template <int HD, bool CAUSAL, bool CROSS, bool GROUPED, class Heads>
__device__ __forceinline__ void attn_bwd_dkv_body(Heads&& heads, const bf16_t* __restrict__ dO, const float* __restrict__ lse2,
                                                  const float* __restrict__ delta, const AttnGrads grads, float scale, float scale_log2e,
                                                  int q_begin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const HeadPtrs hp = heads();
    const int64_t rs = hp.q_rs, ors = hp.ors;
    const int Lq = hp.Lq, Lk = hp.Lk;
    // query tiles from q_begin on (a multiple of 64; the rows before it got no gradient), dO compact [B, Lq - q_begin, H, HD]
    const int Lo = Lq - q_begin;
    const int k0 = hp.blk * 128 + wave * 32;
    const int key = k0 + (lane & 31);

    constexpr int TILE = AG<HD>::TILE, KS = AG<HD>::KS, DT = AG<HD>::DT;
    bf16x8 kf[KS], vf[KS];
    load_own<KS>(hp.kb, hp.k_rs, k0, Lk, lane, kf);
    load_own<KS>(hp.vb, hp.v_rs, k0, Lk, lane, vf);

    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;

    // LDS: per buffer  Q tile | dO tile | lse2[64] | delta[64]
    constexpr int BUF = 2 * TILE + 512;
    const int nt = (Lq + 63) / 64, nfull = (Lq & 63) ? nt - 1 : nt;
    const unsigned sbase = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const TileAddr<HD> ad = tile_addr<HD>(lane, sbase);
    unsigned lse_a = sbase + 16 * half;
    asm volatile("" : "+v"(lse_a));
    unsigned qoff[AG<HD>::CH / 4], dooff[AG<HD>::CH / 4];
    stage_offsets<HD>(rs, tid, qoff);
    stage_offsets<HD>(ors, tid, dooff);
    const int nfull_q = Lq / 64;       // query tiles without a ragged row
    // CAUSAL: query tiles before the workgroup's first key contribute nothing (every query < every key)
    const int t0 = CAUSAL ? max(q_begin >> 6, (hp.blk * 128) >> 6) : q_begin >> 6;
    auto sweep_head = [&](int j) __attribute__((always_inline)) {   // query head hq + j: its Q / dO columns and its lse2 / delta row
        const bf16_t* qb = hp.qb + j * HD;
        const bf16_t* dob = dO + hp.orow * ors + (int64_t)hp.hq * HD + j * HD;
        const float* lse_b = lse2 + hp.st_off + j * hp.st_hs;
        const float* del_b = delta + hp.st_off + j * hp.st_hs;
        // GROUPED: everything a ragged tile derives from the sequence length (clamped lane addresses, 32 row masks) is the same for every
        // head; hoisted out of the head loop it would stay live through every tile body (53 SGPR spills).  One opaque copy of the length per
        // head, used by everything below, keeps it inside the head.
        int Lq_h = Lq, Lo_h = Lo;
        if constexpr (GROUPED) {
            asm volatile("" : "+s"(Lq_h));
            Lo_h = Lq_h - q_begin;
        }
        auto stage = [&](int t, int buf) __attribute__((always_inline)) {
            const unsigned base = sbase + buf * BUF;
            if (t < nfull_q) {
                stage64_full<HD>(qb + (int64_t)t * 64 * rs, qoff, base, wave);
                stage64_full<HD>(dob + ((int64_t)t * 64 - q_begin) * ors, dooff, base + TILE, wave);
            } else {
                stage64<HD>(qb, rs, t * 64, Lq_h, base, tid, wave);
                stage64<HD>(dob, ors, t * 64 - q_begin, Lo_h, base + TILE, tid, wave);
            }
            if (wave < 2) {  // wave 0: lse2[64], wave 1: delta[64] by 4-byte LDS-DMA (rows past Lq clamped; masked at use)
                int qq = t * 64 + lane;
                qq = qq < Lq_h ? qq : Lq_h - 1;
                glds4_asm((wave == 0 ? lse_b : del_b) + qq, base + 2 * TILE + wave * 256);
            }
        };
        if (GROUPED && j > 0) __syncthreads();   // the previous head's last tile may have been a ragged one, which has no barrier behind it
        stage(t0, 0);
        pin_loaded(kf);
        pin_loaded(vf);
        dma_drain();
        __syncthreads();

        sweep_tiles<CAUSAL>(t0, nt, nfull, stage, [&](auto ragged, int buf, int t) __attribute__((always_inline)) {
            if constexpr (!CAUSAL) dkv_tile<HD, decltype(ragged)::value>(buf * BUF, lse_a, ad, kf, vf, dk, dv, t * 64, Lq_h, scale_log2e, half);
            else if (t < nfull && t * 64 >= k0 + 31) dkv_tile<HD, false>(buf * BUF, lse_a, ad, kf, vf, dk, dv, t * 64, Lq_h, scale_log2e, half);
            else if (t * 64 + 63 >= k0) dkv_tile<HD, true, true>(buf * BUF, lse_a, ad, kf, vf, dk, dv, t * 64, Lq_h, scale_log2e, half, key);
        });
    };
    if constexpr (GROUPED) {
        for (int j = 0; j < hp.group; ++j) sweep_head(j);
    } else {
        sweep_head(0);
    }
    const AttnGrads g = grad_ptrs<HD, CROSS>(grads, hp);
    store_own<DT>(dk, scale, g.dk, g.dk_rs, key, key < Lk, half);
    store_own<DT>(dv, 1.0f, g.dv, g.dv_rs, key, key < Lk, half);
}
__global__ __launch_bounds__(256, 2) void attn_causal_bwd_dkv_kernel(const AttnOps ops, const bf16_t* __restrict__ dO,
                                                                     const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                     const AttnGrads grads, int H, int nblk, float scale, float scale_log2e) {
    attn_bwd_dkv_body<64, true, false, false>([&]() __attribute__((always_inline)) { return head_ptrs<64, false>(ops, H, nblk, 0, blockIdx.x, gridDim.x); }, dO, lse2, delta, grads, scale, scale_log2e, 0);
}

// ------------------------------------------------------------------------------------------------
// The non-causal dense and cross backward: attn_delta_kernel, then ONE launch of attn_bwd_kernel whose workgroups take one of two roles.
// Launched apart, each of the two kernels ran one full generation of resident workgroups and then a sparse second one; in one grid the
// dQ workgroups fill the slots the dK/dV tail leaves empty.  No workgroup waits for another: the only value one role took from the other
// was delta, which now comes from the kernel in front.
// ------------------------------------------------------------------------------------------------
// delta for the kept queries: the (batch, head, 128-query block) mapping of the dQ role, a wave per 32 queries, no LDS
template <int HD, bool CROSS>
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnOps ops, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dO,
                                                         float* __restrict__ delta, int H, int nblk, int q_begin) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HeadPtrs hp = head_ptrs<HD, CROSS>(ops, H, nblk, q_begin, blockIdx.x, gridDim.x);
    const int q0 = q_begin + hp.blk * 128 + wave * 32;
    const int Lo = hp.Lq - q_begin;
    const int q = q0 + (lane & 31);
    constexpr int KS = AG<HD>::KS;
    bf16x8 of[KS], dof[KS];
    const int64_t col = hp.orow * hp.ors + (int64_t)hp.hq * HD;
    load_own<KS>(dO + col, hp.ors, q0 - q_begin, Lo, lane, dof);
    load_own<KS>(o + col, hp.ors, q0 - q_begin, Lo, lane, of);
    const float d = delta_own<KS>(of, dof);
    if (q < hp.Lq && (lane >> 5) == 0) delta[hp.st_off + q] = d;
}
// Workgroups 0 .. n_dkv-1 are the dK/dV role (first, because they run longer), the rest the dQ role.  Each role maps its own (index,
// count) through head_ptrs, so the blocks of one (batch, head) of a role still share one XCD's chunk.  The hardware deals workgroups to
// the XCDs by blockIdx.x % 8, so when n_dkv % 8 != 0 the dQ role's chunk c sits on XCD (c + n_dkv) % 8: a rotated set, still one XCD per chunk.
template <int HD, bool CROSS>
__global__ __launch_bounds__(256, 3) void attn_bwd_kernel(const AttnOps ops, const bf16_t* __restrict__ dO, const float* __restrict__ lse2,
                                                          const float* __restrict__ delta, const AttnGrads grads, int H, int nblk_q, int nblk_k,
                                                          int n_dkv, float scale, float scale_log2e, int q_begin) {
    const int id = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (id < n_dkv)
        attn_bwd_dkv_body<HD, false, CROSS, false>([&]() __attribute__((always_inline)) { return head_ptrs<HD, CROSS>(ops, H, nblk_k, q_begin, id, n_dkv); },
                                                   dO, lse2, delta, grads, scale, scale_log2e, q_begin);
    else
        attn_bwd_dq_body<HD, false, CROSS, false>([&]() __attribute__((always_inline)) { return head_ptrs<HD, CROSS>(ops, H, nblk_q, q_begin, id - n_dkv, (int)gridDim.x - n_dkv); },
                                                  nullptr, dO, lse2, delta, grads, scale, scale_log2e, q_begin);
}
// Two instantiations.  One query head per KV head: the plain sweep at the dense kernels' three waves per SIMD.  Grouped: the head loop keeps
// the staging offsets and the store addresses alive through a head's ragged last tile, which the dense kernel runs after they are dead; at
// 168 registers that spills (the build refuses it), so the grouped kernel takes the register budget of two waves per SIMD.
template <bool GROUPED>
__global__ __launch_bounds__(256, GROUPED ? 2 : 3) void attn_varlen_bwd_dkv_kernel(const AttnOps ops, const SeqTable tab, const bf16_t* __restrict__ dO,
                                                                                   const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                                   const AttnGrads grads, int Hq, int Hkv, int M, float scale,
                                                                                   float scale_log2e) {
    attn_bwd_dkv_body<64, false, true, GROUPED>([&]() __attribute__((always_inline)) { return varlen_head_ptrs<64, true>(ops, tab, Hq, Hkv, M); }, dO, lse2,
                                                delta, grads, scale, scale_log2e, 0);
}

// dQ rows of the queries before q_begin: they received no gradient (the dQ kernel only visits the kept queries)
__global__ void zero_q_rows_kernel(bf16_t* __restrict__ dqkv, int L, int q_begin, int64_t rs, int qcols) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B * q_begin * qcols / 8
    const int per_row = qcols >> 3;
    const int64_t r = idx / per_row;
    const int c = (int)(idx % per_row) * 8;
    const int64_t b = r / q_begin, q = r % q_begin;
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = f2bf(0.f);
    *(bf16x8*)(dqkv + (b * L + q) * rs + c) = z;
}

}  // namespace

// softmax scale 1 / sqrt(HD), and the same times log2(e) for the exp2-domain kernels
template <int HD>
constexpr float kScale = HD == 64 ? 0.125f : 0.17677669529663688110f;
template <int HD>
constexpr float kScaleLog2e = kScale<HD> * 1.44269504088896340736f;

static AttnOps packed_ops(const void* qkv, int L) { return AttnOps{(const bf16_t*)qkv, nullptr, nullptr, 0, 0, 0, L, L}; }
static AttnGrads packed_grads(void* dqkv) { return AttnGrads{(bf16_t*)dqkv, nullptr, nullptr, 0, 0, 0}; }

template <int HD, bool CAUSAL = false, bool CROSS = false>
static void launch_fwd(const AttnOps& ops, int B, int H, int q_begin, void* o, float* lse2, hipStream_t s) {
    const int nblk = (ops.Lq - q_begin + 127) / 128;
    hipLaunchKernelGGL((attn_fwd_kernel<HD, CAUSAL, CROSS>), dim3(nblk * B * H), dim3(256), 4 * AG<HD>::TILE, s, ops, (bf16_t*)o, lse2, H, nblk,
                       kScaleLog2e<HD>, q_begin);
}

// LDS of a backward workgroup: the dQ role's two K | V buffers, the dK/dV role's two Q | dO | lse2 | delta buffers
template <int HD>
constexpr int kDqLds = 4 * AG<HD>::TILE;
template <int HD>
constexpr int kDkvLds = 2 * (2 * AG<HD>::TILE + 512);

template <int HD, bool CROSS = false>
static void launch_bwd(const AttnOps& ops, const void* o, const void* dO, const float* lse2, int B, int H, int q_begin, const AttnGrads& grads,
                       float* delta_ws, hipStream_t s) {
    if (q_begin > 0) {   // packed launches only
        const int64_t n = (int64_t)B * q_begin * (H * HD / 8);
        hipLaunchKernelGGL(zero_q_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grads.dq, ops.Lq, q_begin, (int64_t)3 * H * HD, H * HD);
    }
    const int nblk_q = (ops.Lq - q_begin + 127) / 128, nblk_k = (ops.Lk + 127) / 128;
    const int n_dq = nblk_q * B * H, n_dkv = nblk_k * B * H;
    hipLaunchKernelGGL((attn_delta_kernel<HD, CROSS>), dim3(n_dq), dim3(256), 0, s, ops, (const bf16_t*)o, (const bf16_t*)dO, delta_ws, H, nblk_q,
                       q_begin);
    hipLaunchKernelGGL((attn_bwd_kernel<HD, CROSS>), dim3(n_dkv + n_dq), dim3(256), kDqLds<HD> > kDkvLds<HD> ? kDqLds<HD> : kDkvLds<HD>, s, ops,
                       (const bf16_t*)dO, lse2, delta_ws, grads, H, nblk_q, nblk_k, n_dkv, kScale<HD>, kScaleLog2e<HD>, q_begin);
}
static void launch_causal_bwd(const AttnOps& ops, const void* o, const void* dO, const float* lse2, int B, int H, const AttnGrads& grads,
                              float* delta_ws, hipStream_t s) {
    const int nblk = (ops.Lq + 127) / 128;
    hipLaunchKernelGGL(attn_causal_bwd_dq_kernel, dim3(nblk * B * H), dim3(256), kDqLds<64>, s, ops, (const bf16_t*)o, (const bf16_t*)dO, lse2,
                       delta_ws, grads, H, nblk, kScale<64>, kScaleLog2e<64>);
    hipLaunchKernelGGL(attn_causal_bwd_dkv_kernel, dim3(nblk * B * H), dim3(256), kDkvLds<64>, s, ops, (const bf16_t*)dO, lse2, delta_ws, grads, H,
                       nblk, kScale<64>, kScaleLog2e<64>);
}

// every operand is read and every output written 16 bytes per lane (the outputs since the widened stores of round 5)
static bool attn_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

static int attn_check(const char* who, int B, int L, int H, int hd, int q_begin) {
    VT_CHECK_ARG(hd == 64 || hd == 32, "%s: head_dim %d unsupported (64 or 32)", who, hd);
    VT_CHECK_ARG(B > 0 && L > 0 && H > 0, "%s: bad shape", who);
    VT_CHECK_ARG(q_begin >= 0 && q_begin < L && q_begin % 64 == 0, "%s: q_begin=%d must be a multiple of 64 below L=%d", who, q_begin, L);
    VT_CHECK_ARG((int64_t)B * H * 2 * (L / 128 + 1) <= 0x7fffffff, "%s: too many workgroups", who);   // the backward's two roles in one grid
    return VT_OK;
}

extern "C" int vt_attention_fwd_rows(const void* qkv, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t q_begin, void* o_compact, float* lse2,
                                     vtStream stream) {
    VT_CHECK_ARG(qkv && o_compact && lse2, "vt_attention_fwd: null pointer");
    VT_CHECK_ARG(attn_aligned(qkv, o_compact), "vt_attention_fwd: qkv and o must be 16-byte aligned");
    int rc = attn_check("vt_attention_fwd", B, L, H, hd, q_begin);
    if (rc) return rc;
    if (hd == 64) launch_fwd<64>(packed_ops(qkv, L), B, H, q_begin, o_compact, lse2, (hipStream_t)stream);
    else launch_fwd<32>(packed_ops(qkv, L), B, H, q_begin, o_compact, lse2, (hipStream_t)stream);
    VT_CHECK_LAUNCH("vt_attention_fwd");
    return VT_OK;
}

extern "C" int vt_attention_bwd_rows(const void* qkv, const void* o_compact, const void* dO_compact, const float* lse2, int32_t B, int32_t L,
                                     int32_t H, int32_t hd, int32_t q_begin, void* dqkv, float* delta_ws, vtStream stream) {
    VT_CHECK_ARG(qkv && o_compact && dO_compact && lse2 && dqkv && delta_ws, "vt_attention_bwd: null pointer");
    VT_CHECK_ARG(attn_aligned(qkv, o_compact, dO_compact, dqkv), "vt_attention_bwd: qkv, o, dO and dqkv must be 16-byte aligned");
    int rc = attn_check("vt_attention_bwd", B, L, H, hd, q_begin);
    if (rc) return rc;
    if (hd == 64) launch_bwd<64>(packed_ops(qkv, L), o_compact, dO_compact, lse2, B, H, q_begin, packed_grads(dqkv), delta_ws, (hipStream_t)stream);
    else launch_bwd<32>(packed_ops(qkv, L), o_compact, dO_compact, lse2, B, H, q_begin, packed_grads(dqkv), delta_ws, (hipStream_t)stream);
    VT_CHECK_LAUNCH("vt_attention_bwd");
    return VT_OK;
}

extern "C" int vt_attention_fwd(const void* qkv, int32_t B, int32_t L, int32_t H, int32_t hd, void* o, float* lse2, vtStream stream) {
    return vt_attention_fwd_rows(qkv, B, L, H, hd, 0, o, lse2, stream);
}

extern "C" int vt_attention_bwd(const void* qkv, const void* o, const void* dO, const float* lse2, int32_t B, int32_t L, int32_t H,
                                int32_t hd, void* dqkv, float* delta_ws, vtStream stream) {
    return vt_attention_bwd_rows(qkv, o, dO, lse2, B, L, H, hd, 0, dqkv, delta_ws, stream);
}

// ------------------------------------------------------------------------------------------------
// causal attention (the AR consumer): F.scaled_dot_product_attention(q, k, v, is_causal=True) of
// /root/reference/models/larp_ar.py:186-190 and its autograd; head_dim 64 (every llama-abs size: dim / n_head = 64)
// ------------------------------------------------------------------------------------------------
extern "C" int vt_attention_causal_fwd(const void* qkv, int32_t B, int32_t L, int32_t H, void* o, float* lse2, vtStream stream) {
    VT_CHECK_ARG(qkv && o && lse2, "vt_attention_causal_fwd: null pointer");
    VT_CHECK_ARG(B > 0 && L > 0 && H > 0, "vt_attention_causal_fwd: bad shape");
    VT_CHECK_ARG(attn_aligned(qkv, o), "vt_attention_causal_fwd: qkv and o must be 16-byte aligned");
    launch_fwd<64, true>(packed_ops(qkv, L), B, H, 0, o, lse2, (hipStream_t)stream);
    VT_CHECK_LAUNCH("vt_attention_causal_fwd");
    return VT_OK;
}

extern "C" int vt_attention_causal_bwd(const void* qkv, const void* o, const void* dO, const float* lse2, int32_t B, int32_t L, int32_t H, void* dqkv,
                                       float* delta_ws, vtStream stream) {
    VT_CHECK_ARG(qkv && o && dO && lse2 && dqkv && delta_ws, "vt_attention_causal_bwd: null pointer");
    VT_CHECK_ARG(B > 0 && L > 0 && H > 0, "vt_attention_causal_bwd: bad shape");
    VT_CHECK_ARG(attn_aligned(qkv, o, dO, dqkv), "vt_attention_causal_bwd: qkv, o, dO and dqkv must be 16-byte aligned");
    launch_causal_bwd(packed_ops(qkv, L), o, dO, lse2, B, H, packed_grads(dqkv), delta_ws, (hipStream_t)stream);
    VT_CHECK_LAUNCH("vt_attention_causal_bwd");
    return VT_OK;
}

// ------------------------------------------------------------------------------------------------
// cross attention: queries from one tensor, keys and values from another (CrossAttention.forward of
// models/model_design/base/transformer.py:127-141: flash_attn_func(q, k, v) with Lq != Lk); head_dim 64, no mask
// ------------------------------------------------------------------------------------------------
static int cross_check(const char* who, int B, int Lq, int Lk, int H, int hd) {
    VT_CHECK_ARG(hd == 64, "%s: head_dim %d unsupported (64)", who, hd);
    VT_CHECK_ARG(B > 0 && Lq > 0 && Lk > 0 && H > 0, "%s: bad shape B=%d Lq=%d Lk=%d H=%d", who, B, Lq, Lk, H);
    VT_CHECK_ARG((int64_t)B * H * (Lq / 128 + Lk / 128 + 2) <= 0x7fffffff, "%s: too many workgroups", who);   // the backward's two roles in one grid
    return VT_OK;
}
static int cross_stride_check(const char* who, const char* what, int64_t rs, int H) {
    VT_CHECK_ARG(rs >= (int64_t)64 * H && rs % 8 == 0, "%s: row stride %lld of %s must cover 64 x %d columns and be a multiple of 8", who, (long long)rs,
                 what, H);
    // the tile stagers fold (row within a 64-row tile) * rs * 2 bytes into a 32-bit lane offset: below 2^31 with rs < 2^24
    VT_CHECK_ARG(rs < ((int64_t)1 << 24), "%s: row stride %lld of %s is too large (below 2^24 elements)", who, (long long)rs, what);
    return VT_OK;
}

extern "C" int vt_attention_cross_fwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, int32_t B, int32_t Lq,
                                      int32_t Lk, int32_t H, int32_t hd, void* o, float* lse2, vtStream stream) {
    const char* who = "vt_attention_cross_fwd";
    VT_CHECK_ARG(q && k && v && o && lse2, "%s: null pointer", who);
    TRY(cross_check(who, B, Lq, Lk, H, hd));
    TRY(cross_stride_check(who, "q", q_rs, H));
    TRY(cross_stride_check(who, "k", k_rs, H));
    TRY(cross_stride_check(who, "v", v_rs, H));
    VT_CHECK_ARG(attn_aligned(q, k, v, o), "%s: q, k, v and o must be 16-byte aligned", who);
    const AttnOps ops{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, q_rs, k_rs, v_rs, Lq, Lk};
    launch_fwd<64, false, true>(ops, B, H, 0, o, lse2, (hipStream_t)stream);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_attention_cross_bwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, const void* o,
                                      const void* dO, const float* lse2, int32_t B, int32_t Lq, int32_t Lk, int32_t H, int32_t hd, void* dq,
                                      int64_t dq_rs, void* dk, int64_t dk_rs, void* dv, int64_t dv_rs, float* delta_ws, vtStream stream) {
    const char* who = "vt_attention_cross_bwd";
    VT_CHECK_ARG(q && k && v && o && dO && lse2 && dq && dk && dv && delta_ws, "%s: null pointer", who);
    TRY(cross_check(who, B, Lq, Lk, H, hd));
    TRY(cross_stride_check(who, "q", q_rs, H));
    TRY(cross_stride_check(who, "k", k_rs, H));
    TRY(cross_stride_check(who, "v", v_rs, H));
    TRY(cross_stride_check(who, "dq", dq_rs, H));
    TRY(cross_stride_check(who, "dk", dk_rs, H));
    TRY(cross_stride_check(who, "dv", dv_rs, H));
    VT_CHECK_ARG(attn_aligned(q, k, v, o) && attn_aligned(dO, dq, dk, dv), "%s: q, k, v, o, dO, dq, dk and dv must be 16-byte aligned", who);
    const AttnOps ops{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, q_rs, k_rs, v_rs, Lq, Lk};
    const AttnGrads grads{(bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dq_rs, dk_rs, dv_rs};
    launch_bwd<64, true>(ops, o, dO, lse2, B, H, 0, grads, delta_ws, (hipStream_t)stream);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

// ------------------------------------------------------------------------------------------------
// packed variable-length attention with grouped KV heads (the Attn layer of models/model_titok/base/transformer.py:32-62:
// flash_attn_varlen_func(q, k, v, cu_seqlens, ...) with Hq query heads over Hkv KV heads); head_dim 64, no mask
// ------------------------------------------------------------------------------------------------
// Everything about the boundaries is checked here, on the host array, and the table travels in the kernel arguments.
static int varlen_table(const char* who, const int32_t* cu, int n_seq, int M, int Hq, int Hkv, int hd, SeqTable* tab) {
    VT_CHECK_ARG(hd == 64, "%s: head_dim %d unsupported (64)", who, hd);
    VT_CHECK_ARG(M > 0 && Hq > 0 && Hkv > 0, "%s: bad shape M=%d Hq=%d Hkv=%d", who, M, Hq, Hkv);
    VT_CHECK_ARG(Hq % Hkv == 0, "%s: Hq=%d is not a multiple of Hkv=%d", who, Hq, Hkv);
    VT_CHECK_ARG(cu != nullptr, "%s: cu_seqlens_host is null", who);
    VT_CHECK_ARG(n_seq >= 1 && n_seq <= VT_VARLEN_MAX_SEQ, "%s: n_seq=%d outside 1..%d sequences per launch", who, n_seq, VT_VARLEN_MAX_SEQ);
    VT_CHECK_ARG(cu[0] == 0, "%s: cu_seqlens[0]=%d must be 0", who, cu[0]);
    for (int b = 0; b < n_seq; ++b)
        VT_CHECK_ARG(cu[b + 1] > cu[b], "%s: cu_seqlens must increase strictly (no empty sequence): cu[%d]=%d, cu[%d]=%d", who, b, cu[b], b + 1, cu[b + 1]);
    VT_CHECK_ARG(cu[n_seq] == M, "%s: cu_seqlens[%d]=%d must equal M=%d", who, n_seq, cu[n_seq], M);
    tab->n = n_seq;
    int blocks = 0;
    for (int b = 0; b <= n_seq; ++b) {
        tab->cu[b] = cu[b];
        tab->blk[b] = blocks;
        if (b < n_seq) blocks += (cu[b + 1] - cu[b] + 127) / 128;
    }
    for (int b = n_seq + 1; b <= VT_VARLEN_MAX_SEQ; ++b) tab->cu[b] = M, tab->blk[b] = blocks;
    tab->total = blocks;
    VT_CHECK_ARG((int64_t)blocks * Hq <= 0x7fffffff, "%s: too many workgroups", who);
    return VT_OK;
}

extern "C" int vt_attention_varlen_fwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs,
                                       const int32_t* cu_seqlens_host, int32_t n_seq, int32_t M, int32_t Hq, int32_t Hkv, int32_t hd, void* o,
                                       float* lse2, vtStream stream) {
    const char* who = "vt_attention_varlen_fwd";
    VT_CHECK_ARG(q && k && v && o && lse2, "%s: null pointer", who);
    SeqTable tab;
    TRY(varlen_table(who, cu_seqlens_host, n_seq, M, Hq, Hkv, hd, &tab));
    TRY(cross_stride_check(who, "q", q_rs, Hq));
    TRY(cross_stride_check(who, "k", k_rs, Hkv));
    TRY(cross_stride_check(who, "v", v_rs, Hkv));
    VT_CHECK_ARG(attn_aligned(q, k, v, o), "%s: q, k, v and o must be 16-byte aligned", who);
    const AttnOps ops{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, q_rs, k_rs, v_rs, 0, 0};
    hipLaunchKernelGGL(attn_varlen_fwd_kernel, dim3(tab.total * Hq), dim3(256), 4 * AG<64>::TILE, (hipStream_t)stream, ops, tab, (bf16_t*)o, lse2, Hq,
                       Hkv, M, kScaleLog2e<64>);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

extern "C" int vt_attention_varlen_bwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, const void* o,
                                       const void* dO, const float* lse2, const int32_t* cu_seqlens_host, int32_t n_seq, int32_t M, int32_t Hq,
                                       int32_t Hkv, int32_t hd, void* dq, int64_t dq_rs, void* dk, int64_t dk_rs, void* dv, int64_t dv_rs,
                                       float* delta_ws, vtStream stream) {
    const char* who = "vt_attention_varlen_bwd";
    VT_CHECK_ARG(q && k && v && o && dO && lse2 && dq && dk && dv && delta_ws, "%s: null pointer", who);
    SeqTable tab;
    TRY(varlen_table(who, cu_seqlens_host, n_seq, M, Hq, Hkv, hd, &tab));
    TRY(cross_stride_check(who, "q", q_rs, Hq));
    TRY(cross_stride_check(who, "k", k_rs, Hkv));
    TRY(cross_stride_check(who, "v", v_rs, Hkv));
    TRY(cross_stride_check(who, "dq", dq_rs, Hq));
    TRY(cross_stride_check(who, "dk", dk_rs, Hkv));
    TRY(cross_stride_check(who, "dv", dv_rs, Hkv));
    VT_CHECK_ARG(attn_aligned(q, k, v, o) && attn_aligned(dO, dq, dk, dv), "%s: q, k, v, o, dO, dq, dk and dv must be 16-byte aligned", who);
    const AttnOps ops{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, q_rs, k_rs, v_rs, 0, 0};
    const AttnGrads grads{(bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, dq_rs, dk_rs, dv_rs};
    hipLaunchKernelGGL(attn_varlen_bwd_dq_kernel, dim3(tab.total * Hq), dim3(256), kDqLds<64>, (hipStream_t)stream, ops, tab, (const bf16_t*)o,
                       (const bf16_t*)dO, lse2, delta_ws, grads, Hq, Hkv, M, kScale<64>, kScaleLog2e<64>);
    if (Hq == Hkv)
        hipLaunchKernelGGL(attn_varlen_bwd_dkv_kernel<false>, dim3(tab.total * Hkv), dim3(256), kDkvLds<64>, (hipStream_t)stream, ops,
                           tab, (const bf16_t*)dO, lse2, delta_ws, grads, Hq, Hkv, M, kScale<64>, kScaleLog2e<64>);
    else
        hipLaunchKernelGGL(attn_varlen_bwd_dkv_kernel<true>, dim3(tab.total * Hkv), dim3(256), kDkvLds<64>, (hipStream_t)stream, ops,
                           tab, (const bf16_t*)dO, lse2, delta_ws, grads, Hq, Hkv, M, kScale<64>, kScaleLog2e<64>);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
