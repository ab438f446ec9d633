// Whole-model engine for the LARP tokenizer step on gfx950: plans one workspace, then enqueues the
// complete forward (encode -> VQ -> decode) or a range of backward stages on a stream by calling the
// kernels of this library back to back.  Host code only does pointer arithmetic: no allocation, no
// synchronisation, no per-op Python -- the sequence is hipGraph-capturable.
//
// Follows /root/reference/models/larp_tokenizer.py:400-428 (encode), :456-469 (decode), :489-496
// (forward); models/transformer.py:62-70 (cat -> blocks -> last len(query) rows); timm Block
// (pre-LN attention + MLP, see oracle/larp_oracle.py block()); models/bottleneck.py:170-188.
//
// HBM layout (all row-major, rows padded to a multiple of 128 and zero-initialised once so that the
// TN weight-gradient GEMM can contract over padded rows):
//   residual stream x      fp32 [B*L, D]   one buffer per block boundary (saved for LayerNorm backward)
//   MFMA operands          bf16            LayerNorm outputs, qkv, attention out, fc1 pre/post GELU
//   weights                bf16 [N,K] and [K,N] packed copies of the fp32 masters (vt_tokenizer_pack)
// With 288 GB of HBM3E nothing is recomputed except the attention probabilities.
#include <vector>

#include "vt_common.h"

// The KL bottleneck's kernels (vt_kl.hip) are referenced weakly: the library resolves them, a link of the engine without vt_kl.o
// (a host-side test harness that only models the VQ path) still loads, and vt_tokenizer_create_kl refuses to build a KL handle there.
extern "C" int vt_kl_forward(const float* z, int64_t ldz, int64_t M, int32_t d, int32_t batch, uint64_t seed, const uint32_t* seed_counter,
                             float* mean, float* sample, void* sample_pad_bf16, int64_t ldp, float* noise, float* loss_kl, void* workspace,
                             vtStream stream) __attribute__((weak));
extern "C" int vt_kl_backward(const float* g_sample, int64_t ldg, const float* g_mean, const float* gkl, const float* z, int64_t ldz,
                              const float* noise, int64_t M, int32_t d, int32_t batch, float* dz, void* dz_pad_bf16, int64_t ldp,
                              vtStream stream) __attribute__((weak));
// The same for the rotary pass of the plain block stack (vt_rope.hip): without it vt_stack_forward_rotary / _backward_rotary refuse to run.
extern "C" int vt_rope_rotate(void* qkv, int64_t ld, int64_t M, int32_t L, int32_t H, const float* cos_tab, const float* sin_tab,
                              int32_t conjugate, vtStream stream) __attribute__((weak));

static const bool g_no_splitk = [] { const char* e = getenv("VT_GEMM_SPLITK"); return e && strcmp(e, "0") == 0; }();   // A/B switch, read once

namespace {

__global__ void gather_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ perm, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}
// dst[perm[i]] = src[i]
__global__ void scatter_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ perm, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[perm[i]] = src[i];
}

// out[0] = mean_b |x[b*seq + r0, :]|, out[1] = mean_b |x[b*seq + r1, :]|   (bottleneck.py:171-172)
// One workgroup per statistic, one WAVE per clip (the serial loop over the batch took 27 us of dependent loads for 48 KB of input);
// per row the same lane-strided partial sums and wave reduction as before, and the clips are added in index order: same bits.
__global__ __launch_bounds__(512) void rownorm_mean_kernel(const float* __restrict__ x, int64_t seq, int64_t r0, int64_t r1, int batch, int dim, float* __restrict__ out) {
    __shared__ float norms[8];
    const int which = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = which == 0 ? r0 : r1;
    float tot = 0.f;
    for (int b0 = 0; b0 < batch; b0 += 8) {
        const int b = b0 + wave;
        if (b < batch) {
            const float* p = x + ((int64_t)b * seq + r) * dim;
            float s = 0.f;
            for (int c = lane; c < dim; c += 64) s += p[c] * p[c];
            s = wave_sum(s);
            if (lane == 0) norms[wave] = sqrtf(s);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 8 && b0 + k < batch; ++k) tot += norms[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[which] = tot / (float)batch;
}

// dst[r, 0..d) = float(bf16(src[r, 0..d)))   compact copy of the in_linear output ('projected_z')
__global__ void compact_cols_kernel(const float* __restrict__ src, int64_t lds_, int rows, int d, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * d) dst[i] = src[(int64_t)(i / d) * lds_ + (i % d)];
}

struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

struct BlockBufs {
    // packed weights
    size_t qkv_wb, qkv_wt, proj_wb, proj_wt, fc1_wb, fc1_wt, fc2_wb, fc2_wt;
    // saved activations
    size_t x_mid, h1, mean1, rstd1, qkv, lse, o, h2, mean2, rstd2, dgelu, g;   // dgelu = gelu'(fc1 pre-activation), g = its gelu, both bf16
};

}  // namespace

// Which rows the second half of a block (proj, LayerNorm2, MLP; in the backward also the attention queries) runs on: n rows (n_pad with the
// 128-padding of a weight-gradient contraction) found through `map` in the [M, D] residual stream; q_begin = first query row of a sequence.
struct Rows { vtRowMap map; int n, n_pad, q_begin; };

// The LAST block of a stack only has to produce the rows the stack returns (transformer.py:69: h[:, -len(query):]): the
// last nk rows of every sequence.  Its MLP half, the attention queries and the matching backward work run on those rows
// only (compact buffers); K/V, the qkv GEMM and LayerNorm1 still cover all rows.  Enabled per stack when the first kept
// row (L - nk) is a multiple of 64.
struct LastBlock { bool enabled; Rows rows; size_t dxa, dxm, du; };   // rows.map = {nk, L, L - nk}; compact bf16 dL/dx_out, dL/dx_mid and du

// One stack of blocks: the tokenizer's encoder, its decoder, or the only one of a vtStack
struct Side {
    std::vector<BlockBufs> blocks;
    std::vector<size_t> x;   // residual stream at block boundaries (depth+1)
    LastBlock last = {};
};

// What the block machinery needs: geometry, the backward scratch and the scheduling state of the deferred weight gradients.
// vtTokenizer and vtStack are one of these plus their own members.
struct BlockEngine {
    int B, L, H, D, M, Mp, D3, D4;
    size_t ws_bytes;                         // the handle's whole workspace
    size_t dX, dh, dob, delta, ln_ws, cs_ws, cs_part;   // backward scratch
    bool splitk_on = !g_no_splitk;           // vt_tokenizer_set_split_k / vt_stack_set_split_k; VT_GEMM_SPLITK=0 starts it off
    int wg_batch = 4;                        // vt_tokenizer_set_wgrad_batch: blocks per grouped weight-gradient launch (1..WG_BATCH)
    bool data_parallel = false;              // vt_tokenizer_set_data_parallel: a collective runs next to the backward (see nt())
    bool in_backward = false;                // set by the entry points: nt() hands the split-K workspace to backward GEMMs only
    size_t splitk = 0, splitk_bytes = 0;     // vt_gemm_nt's split-K partial sums + arrival counters (zeroed by *_init_workspace)
    // bf16 gradient operands that a block's weight-gradient GEMMs read.  The wgrads of WG_BATCH consecutive blocks are
    // deferred into one grouped launch, so these rotate over WG_BATCH + 1 sets (the set a block writes its dx_in to
    // is the next block's dx_out set).
    struct GradSet { size_t dx_out, dx_mid, du, dqkv, ln_part1, ln_part2, cs_part; };   // + the block's partial sums awaiting the grouped reduction
    static constexpr int WG_BATCH = 4;
    static constexpr int NSETS_MAX = 2 * WG_BATCH + 1;
    GradSet gs[NSETS_MAX];    // WG_BATCH + 1 are in rotation; all of them when the weight gradients run on their own stream (below)
    // Data-parallel runs: the deferred weight-gradient launches (and the partial-sum reductions of the same blocks) go to a SECOND stream
    // (vt_tokenizer_set_wgrad_stream).  They are off the backward's critical path, and with a collective's workgroups resident the
    // exact-fit GEMM launches of the main stream leave most of the chip idle in their extra round: work of an
    // independent stream fills it.  Ordering: the side stream starts a group behind an event of the main stream (operands written);
    // a gradient set is rewritten by the main stream only behind the event of the group that read it (twice the sets, so that wait is
    // normally over); the last stage of backward joins the side stream.
    hipStream_t wg_stream = nullptr;
    static constexpr int NEV = 16;
    hipEvent_t ev_fork[NEV] = {}, ev_done[NEV] = {};
    int flush_id = 0;                 // groups flushed to the side stream so far (event slot = id % NEV)
    int set_flush[NSETS_MAX];         // id of the side-stream group that last read the set, -1 = none pending
    std::vector<int> sets_pending;    // sets used by the blocks whose weight gradients are queued
    int nsets() const { return wg_stream ? NSETS_MAX : WG_BATCH + 1; }
    ~BlockEngine() {
        for (int i = 0; i < NEV; ++i) {
            if (ev_fork[i]) (void)hipEventDestroy(ev_fork[i]);
            if (ev_done[i]) (void)hipEventDestroy(ev_done[i]);
        }
    }
    // host-side state of an in-flight backward
    std::vector<vtGemmTN> pending;
    std::vector<vtReduceItem> pending_red;   // partial-sum reductions of the same blocks (one grouped launch at the flush)
    int pending_blocks = 0;   // blocks whose wgrads sit in `pending`
    int set_idx = 0;          // gradient set of the block processed next
    int final_through = 0;    // stages [0, final_through) have complete gradients
};

struct vtTokenizer : BlockEngine {
    vtTokenizerConfig c;
    int Nv, Mv, Mvp, Mq, Mqp, Kp;
    std::vector<int32_t> perm_host;  // packed head row j  <-  reference row perm[j]
    // ---- workspace offsets
    size_t perm, head_b_perm, dec_query_sum;
    size_t pe_wb, in_wb, in_wt, out_wb, out_wt, head_wb, head_wt;
    Side enc, dec;
    size_t patches, zb, zproj, vq_E, vq_wnorm, vq_zn, vq_znorm, vq_idx, vq_rz, vq_rzpad, vq_losses, vq_ws, encoded_int;
    size_t hN, meanH, rstdH, yrows;
    bool kl = false;                         // vt_tokenizer_create_kl: KL bottleneck ('skl') in place of the quantizer; in_linear has 2d outputs
    size_t kl_noise = 0, kl_ws = 0;          // eps of the last forward (read by the backward), loss partial sums of vt_kl_forward
    size_t dY, dhN, dEncb, d_rz, dz_pad, dTok, tmp_vec, wg_slabs;   // backward scratch outside the blocks
    const uint32_t* seed_ctr = nullptr;   // device-side per-call counter of the stochastic VQ (graph replay), see vt_vq_forward_ctr
    int wg_tail = 0;                         // vt_tokenizer_set_wgrad_tail: the encoder's first wg_tail blocks (the LAST of the backward) flush their weight gradients block by block
};

// A stack of blocks on its own (the vt_stack_* entry points at the end of this file)
struct vtStack : BlockEngine {
    Side side;
};

static void block_geometry(BlockEngine* e, int B, int L, int H, int D) {
    e->B = B; e->L = L; e->H = H; e->D = D;
    e->M = B * L; e->Mp = (int)round_up(e->M, 128);
    e->D3 = 3 * D; e->D4 = 4 * D;
}

static void plan_blocks(const BlockEngine* e, Arena& a, Side& sd, int depth) {
    const size_t Mp = e->Mp, D = e->D, D3 = e->D3, D4 = e->D4;
    sd.blocks.resize(depth);
    for (BlockBufs& b : sd.blocks) {
        b.qkv_wb = a.take(D3 * D * 2); b.qkv_wt = a.take(D * D3 * 2);
        b.proj_wb = a.take(D * D * 2); b.proj_wt = a.take(D * D * 2);
        b.fc1_wb = a.take(D4 * D * 2); b.fc1_wt = a.take(D * D4 * 2);
        b.fc2_wb = a.take(D * D4 * 2); b.fc2_wt = a.take(D4 * D * 2);
        b.x_mid = a.take(Mp * D * 4);
        b.h1 = a.take(Mp * D * 2); b.mean1 = a.take(Mp * 4); b.rstd1 = a.take(Mp * 4);
        b.qkv = a.take(Mp * D3 * 2); b.lse = a.take((size_t)e->B * e->H * e->L * 4);
        b.o = a.take(Mp * D * 2);
        b.h2 = a.take(Mp * D * 2); b.mean2 = a.take(Mp * 4); b.rstd2 = a.take(Mp * 4);
        b.dgelu = a.take(Mp * D4 * 2); b.g = a.take(Mp * D4 * 2);
    }
}
static void plan_residuals(const BlockEngine* e, Arena& a, Side& sd) {
    sd.x.resize(sd.blocks.size() + 1);
    for (auto& x : sd.x) x = a.take((size_t)e->Mp * e->D * 4);
}

// The backward scratch of the block machinery, in the order the workspace has always had: dX, the gradient sets, dh, dob | the compact buffers
// of the sides whose last block may run on kept rows (`kept`, their last.rows set by the caller) | delta, split-K, ln_ws, cs_ws, cs_part.
// cs_cols: widest vt_colsum the handle runs over cs_ws.
static void plan_block_scratch(BlockEngine* e, Arena& a, std::initializer_list<Side*> kept, int cs_cols) {
    const size_t Mp = e->Mp, D = e->D;
    e->dX = a.take(Mp * D * 4);
    for (auto& g : e->gs) {
        g.dx_out = a.take(Mp * D * 2); g.dx_mid = a.take(Mp * D * 2);
        g.du = a.take(Mp * e->D4 * 2); g.dqkv = a.take(Mp * e->D3 * 2);
        g.ln_part1 = a.take(vt_layernorm_bwd_workspace_bytes(e->D)); g.ln_part2 = a.take(vt_layernorm_bwd_workspace_bytes(e->D));
        g.cs_part = a.take((size_t)((e->M + 191) / 192) * e->D4 * 4);
    }
    e->dh = a.take(Mp * D * 2); e->dob = a.take(Mp * D * 2);
    for (Side* sd : kept) {
        LastBlock& lb = sd->last;
        lb.dxa = a.take((size_t)lb.rows.n_pad * D * 2); lb.dxm = a.take((size_t)lb.rows.n_pad * D * 2); lb.du = a.take((size_t)lb.rows.n_pad * e->D4 * 2);
    }
    e->delta = a.take((size_t)e->B * e->H * e->L * 4);
    e->splitk_bytes = vt_gemm_nt_splitk_workspace_bytes();
    e->splitk = a.take(e->splitk_bytes);
    e->ln_ws = a.take(vt_layernorm_bwd_workspace_bytes(e->D));
    e->cs_ws = a.take(vt_colsum_workspace_bytes(cs_cols));
    e->cs_part = a.take((size_t)((e->M + 191) / 192) * e->D4 * 4);  // per-M-tile column sums out of the fc2-dgrad epilogue
}

static int create_tokenizer(const vtTokenizerConfig* cfg, bool kl, vtTokenizer** out) {
    const char* fn = kl ? "vt_tokenizer_create_kl" : "vt_tokenizer_create";
    VT_CHECK_ARG(cfg && out, "%s: null pointer", fn);
    const vtTokenizerConfig& c = *cfg;
    VT_CHECK_ARG(c.B > 0 && c.C > 0 && c.T > 0 && c.S > 0 && c.pt > 0 && c.p > 0, "%s: bad geometry", fn);
    VT_CHECK_ARG(c.T % c.pt == 0 && c.S % c.p == 0 && c.p % 8 == 0, "%s: T%%pt, S%%p, p%%8 must be 0", fn);
    VT_CHECK_ARG(c.D % 256 == 0 && c.D <= 1024 && c.H * 64 == c.D, "%s: D=%d H=%d unsupported (head_dim must be 64, D in 256..1024)", fn, c.D, c.H);
    VT_CHECK_ARG(c.depth_enc > 0 && c.depth_dec > 0 && c.Nq > 0 && (kl || c.K > 0), "%s: bad depth/Nq/K", fn);
    VT_CHECK_ARG(c.d == 8 || c.d == 16 || c.d == 24 || c.d == 32, "%s: bottleneck_dim %d unsupported (8,16,24,32)", fn, c.d);
    VT_CHECK_ARG((c.C * c.pt * c.p * c.p) % 64 == 0, "%s: patch volume must be a multiple of 64", fn);
    VT_CHECK_ARG(!kl || (vt_kl_forward && vt_kl_backward), "%s: the KL kernels (vt_kl.hip) are not linked into this library", fn);
    vtTokenizer* t = new vtTokenizer();
    t->c = c;
    t->kl = kl;
    t->Nv = (c.T / c.pt) * (c.S / c.p) * (c.S / c.p);
    block_geometry(t, c.B, t->Nv + c.Nq, c.H, c.D);
    t->Mv = c.B * t->Nv; t->Mvp = (int)round_up(t->Mv, 128);
    t->Mq = c.B * c.Nq; t->Mqp = (int)round_up(t->Mq, 128);
    t->Kp = c.C * c.pt * c.p * c.p;
    // head row permutation: packed order (c,dt,dy,dx)  <-  reference order (dt,dy,dx,c)  (larp_tokenizer.py:452-453)
    t->perm_host.resize(t->Kp);
    for (int ch = 0; ch < c.C; ++ch)
        for (int dt = 0; dt < c.pt; ++dt)
            for (int dy = 0; dy < c.p; ++dy)
                for (int dx = 0; dx < c.p; ++dx) {
                    const int packed = ((ch * c.pt + dt) * c.p + dy) * c.p + dx;
                    const int ref = ((dt * c.p + dy) * c.p + dx) * c.C + ch;
                    t->perm_host[packed] = ref;
                }
    Arena a;
    const size_t D = c.D, Mvp = t->Mvp, Mqp = t->Mqp, Kp = t->Kp;
    t->perm = a.take(Kp * 4); t->head_b_perm = a.take(Kp * 4); t->dec_query_sum = a.take((size_t)t->Nv * D * 4);
    t->pe_wb = a.take(D * Kp * 2);
    t->in_wb = a.take((size_t)64 * D * 2); t->in_wt = a.take(D * 64 * 2);
    t->out_wb = a.take(D * 64 * 2); t->out_wt = a.take((size_t)64 * D * 2);
    t->head_wb = a.take(Kp * D * 2); t->head_wt = a.take(D * Kp * 2);
    plan_blocks(t, a, t->enc, c.depth_enc);
    plan_blocks(t, a, t->dec, c.depth_dec);
    plan_residuals(t, a, t->enc);
    plan_residuals(t, a, t->dec);
    t->patches = a.take(Mvp * Kp * 2);
    t->zb = a.take(Mqp * D * 2);
    t->zproj = a.take(Mqp * 64 * 4);
    if (kl) {
        // the bf16 sample (out_linear operand) lives in vq_rzpad; the quantizer's buffers are not planned
        t->vq_E = t->vq_wnorm = t->vq_zn = t->vq_znorm = t->vq_idx = t->vq_rz = t->vq_losses = t->vq_ws = 0;
        t->vq_rzpad = a.take(Mqp * 64 * 2);
        t->kl_noise = a.take(Mqp * c.d * 4); t->kl_ws = a.take(VT_KL_WORKSPACE_BYTES);
    } else {
        t->vq_E = a.take((size_t)c.K * c.d * 4); t->vq_wnorm = a.take((size_t)c.K * 4);
        t->vq_zn = a.take(Mqp * c.d * 4); t->vq_znorm = a.take(Mqp * 4); t->vq_idx = a.take(Mqp * 8);
        t->vq_rz = a.take(Mqp * c.d * 4); t->vq_rzpad = a.take(Mqp * 64 * 2); t->vq_losses = a.take(64);
        t->vq_ws = a.take(vt_vq_workspace_bytes(t->Mq, c.K, c.d));
    }
    t->encoded_int = a.take(Mqp * D * 4);
    t->hN = a.take(Mvp * D * 2); t->meanH = a.take(Mvp * 4); t->rstdH = a.take(Mvp * 4);
    t->yrows = a.take(Mvp * Kp * 4);
    for (Side* sd : {&t->enc, &t->dec}) {   // the encoder returns its Nq latent rows, the decoder its Nv video rows
        const int nk = sd == &t->enc ? c.Nq : t->Nv, q_begin = t->L - nk;
        sd->last.rows = Rows{{nk, t->L, q_begin}, c.B * nk, (int)round_up(c.B * nk, 128), q_begin};
        sd->last.enabled = q_begin % 64 == 0 && q_begin > 0;
    }
    plan_block_scratch(t, a, {&t->enc, &t->dec}, (int)(Kp > (size_t)t->D4 ? Kp : t->D4));
    t->dY = a.take(Mvp * Kp * 2); t->dhN = a.take(Mvp * D * 2);
    t->dEncb = a.take(Mqp * D * 2); t->d_rz = a.take(Mqp * 64 * 4); t->dz_pad = a.take(Mqp * 64 * 2);
    t->dTok = a.take(Mvp * D * 2);
    t->tmp_vec = a.take((Kp > (size_t)t->D4 ? Kp : t->D4) * 4);
    t->wg_slabs = a.take((size_t)16 * D * 64 * 4);  // split-M partials of the two skinny (d-wide) weight gradients
    t->ws_bytes = a.off;
    *out = t;
    return VT_OK;
}

extern "C" int vt_tokenizer_create(const vtTokenizerConfig* cfg, vtTokenizer** out) { return create_tokenizer(cfg, false, out); }
extern "C" int vt_tokenizer_create_kl(const vtTokenizerConfig* cfg, vtTokenizer** out) { return create_tokenizer(cfg, true, out); }

extern "C" void vt_tokenizer_destroy(vtTokenizer* t) { delete t; }
extern "C" size_t vt_tokenizer_workspace_bytes(const vtTokenizer* t) { return t ? t->ws_bytes : 0; }
extern "C" int32_t vt_tokenizer_num_backward_stages(const vtTokenizer* t) { return t ? 3 + t->c.depth_enc + t->c.depth_dec : 0; }
static int set_split_k(BlockEngine* e, int32_t on, const char* fn) {
    VT_CHECK_ARG(e, "%s: null handle", fn);
    e->splitk_on = on != 0;
    return VT_OK;
}
extern "C" int vt_tokenizer_set_split_k(vtTokenizer* t, int32_t on) { return set_split_k(t, on, "vt_tokenizer_set_split_k"); }
extern "C" int vt_stack_set_split_k(vtStack* t, int32_t on) { return set_split_k(t, on, "vt_stack_set_split_k"); }
// Data-parallel runs: the weight-gradient launches on a stream of their own (see the members above); NULL = single-stream schedule.
extern "C" int vt_tokenizer_set_wgrad_stream(vtTokenizer* t, vtStream side) {
    VT_CHECK_ARG(t, "vt_tokenizer_set_wgrad_stream: null handle");
    VT_CHECK_ARG(t->pending.empty() && t->pending_red.empty(), "vt_tokenizer_set_wgrad_stream: a backward is in flight");
    t->wg_stream = (hipStream_t)side;
    for (int i = 0; i < BlockEngine::NSETS_MAX; ++i) t->set_flush[i] = -1;
    t->sets_pending.clear();
    if (side) {
        for (int i = 0; i < BlockEngine::NEV; ++i) {
            if (!t->ev_fork[i] && hipEventCreateWithFlags(&t->ev_fork[i], hipEventDisableTiming) != hipSuccess) { vt_set_error("vt_tokenizer_set_wgrad_stream: event creation failed"); return VT_ERR_LAUNCH; }
            if (!t->ev_done[i] && hipEventCreateWithFlags(&t->ev_done[i], hipEventDisableTiming) != hipSuccess) { vt_set_error("vt_tokenizer_set_wgrad_stream: event creation failed"); return VT_ERR_LAUNCH; }
        }
    }
    return VT_OK;
}
// Data-parallel runs: the gradients of a 4-block group only become final -- and their all-reduce can only start -- at the group's grouped
// weight-gradient launch, so with the default schedule the encoder's blocks 3..0 (113 MB of fp32 gradients at config B) are reduced after
// the last backward kernel, fully exposed.  With n > 0 the encoder's blocks below n are flushed block by block (n = 3: groups 3-2 | 1 | 0),
// which leaves one block's 28 MB for the tail and costs three launches that do not fill whole rounds of the chip (+ ~0.1 ms of compute).
// Same kernels on the same operands: gradients are bit-identical to the default schedule.
extern "C" int vt_tokenizer_set_wgrad_tail(vtTokenizer* t, int32_t n) {
    VT_CHECK_ARG(t && n >= 0, "vt_tokenizer_set_wgrad_tail: null handle or negative count");
    t->wg_tail = n;
    return VT_OK;
}
// Data-parallel runs: a gradient all-reduce's persistent workgroups hold CUs during the backward; nt() then launches the backward's
// GEMMs that have more 192x192 tiles than the chip has CUs one tile per workgroup (vtGemmNT.tile = 6).  Same bits.
extern "C" int vt_tokenizer_set_data_parallel(vtTokenizer* t, int32_t on) {
    VT_CHECK_ARG(t, "vt_tokenizer_set_data_parallel: null handle");
    t->data_parallel = on != 0;
    return VT_OK;
}
// blocks per grouped weight-gradient launch, 1..4 (default 4: 768 tiles = three whole rounds of the chip).  Smaller groups hand the gradient
// reducer finished slices sooner and, with the weight gradients on their own stream, keep that stream supplied with work throughout the backward.
extern "C" int vt_tokenizer_set_wgrad_batch(vtTokenizer* t, int32_t n) {
    VT_CHECK_ARG(t && n >= 1 && n <= BlockEngine::WG_BATCH, "vt_tokenizer_set_wgrad_batch: null handle or n outside 1..%d", BlockEngine::WG_BATCH);
    VT_CHECK_ARG(t->pending.empty(), "vt_tokenizer_set_wgrad_batch: a backward is in flight");
    t->wg_batch = n;
    return VT_OK;
}
extern "C" int vt_tokenizer_set_seed_counter(vtTokenizer* t, const uint32_t* seed_counter) {
    VT_CHECK_ARG(t, "vt_tokenizer_set_seed_counter: null handle");
    t->seed_ctr = seed_counter;
    return VT_OK;
}
extern "C" int vt_tokenizer_init_workspace(vtTokenizer* t, void* ws, vtStream stream) {
    VT_CHECK_ARG(t && ws, "vt_tokenizer_init_workspace: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, t->ws_bytes, s) != hipSuccess) { vt_set_error("vt_tokenizer_init_workspace: memset failed"); return VT_ERR_LAUNCH; }
    if (hipMemcpyAsync(WS(int32_t, t->perm), t->perm_host.data(), (size_t)t->Kp * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
        vt_set_error("vt_tokenizer_init_workspace: perm upload failed");
        return VT_ERR_LAUNCH;
    }
    return VT_OK;
}

// Attention backward of one block: the two-kernel form (dQ kernel + dK/dV kernel, 7 products).  The five-product kernel with an ordered
// dQ hand-off that round 3 built was correct and bit-reproducible but slower (346 vs 244 us at the step's shape) and left the tree in
// round 4; its record: DESIGN.md section 5 "Attention backward, round 3", profiles/r03_attention_bwd_*.
static int attn_bwd(BlockEngine* e, void* ws, const void* qkv, const void* o, const void* dO, const float* lse, int q_begin, void* dqkv, vtStream s) {
    return vt_attention_bwd_rows(qkv, o, dO, lse, e->B, e->L, e->H, e->D / e->H, q_begin, dqkv, WS(float, e->delta), s);
}

static int copy_d2d(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        vt_set_error("device-to-device copy of %zu bytes failed", bytes);
        return VT_ERR_LAUNCH;
    }
    return VT_OK;
}

static vtPackJob pack_job(const float* w, int N, int K, const int32_t* perm, void* wb, int64_t ldd, void* wt, int64_t lddT) {
    vtPackJob q;
    q.w = w; q.N = N; q.K = K; q.row_perm = perm; q.wb = wb; q.ldd = ldd; q.wt = wt; q.lddT = lddT;
    return q;
}

static void pack_block_jobs(const BlockEngine* e, const std::vector<BlockBufs>& v, const vtBlockTensors* bl, void* ws, std::vector<vtPackJob>& jobs) {
    const int D = e->D, D3 = e->D3, D4 = e->D4;
    for (size_t i = 0; i < v.size(); ++i) {
        const BlockBufs& b = v[i];
        jobs.push_back(pack_job(bl[i].qkv_w, D3, D, nullptr, WS(void, b.qkv_wb), D, WS(void, b.qkv_wt), D3));
        jobs.push_back(pack_job(bl[i].proj_w, D, D, nullptr, WS(void, b.proj_wb), D, WS(void, b.proj_wt), D));
        jobs.push_back(pack_job(bl[i].fc1_w, D4, D, nullptr, WS(void, b.fc1_wb), D, WS(void, b.fc1_wt), D4));
        jobs.push_back(pack_job(bl[i].fc2_w, D, D4, nullptr, WS(void, b.fc2_wb), D4, WS(void, b.fc2_wt), D));
    }
}

extern "C" int vt_tokenizer_pack(vtTokenizer* t, const vtTokenizerTensors* P, void* ws, vtStream s) {
    VT_CHECK_ARG(t && P && ws && P->enc_blocks && P->dec_blocks, "vt_tokenizer_pack: null pointer");
    const vtTokenizerConfig& c = t->c;
    const int D = c.D, Kp = t->Kp;
    std::vector<vtPackJob> jobs;   // every bf16 operand copy of the model: 4 grouped launches instead of ~100 single ones
    jobs.push_back(pack_job(P->pe_w, D, Kp, nullptr, WS(void, t->pe_wb), Kp, nullptr, 0));
    jobs.push_back(pack_job(P->in_w, t->kl ? 2 * c.d : c.d, D, nullptr, WS(void, t->in_wb), D, WS(void, t->in_wt), 64));    // [d,D] and [D,64] (KL: 2d rows)
    jobs.push_back(pack_job(P->out_w, D, c.d, nullptr, WS(void, t->out_wb), 64, WS(void, t->out_wt), D));  // [D,64] and [64,D]
    jobs.push_back(pack_job(P->head_w, Kp, D, WS(int32_t, t->perm), WS(void, t->head_wb), D, WS(void, t->head_wt), Kp));
    pack_block_jobs(t, t->enc.blocks, P->enc_blocks, ws, jobs);
    pack_block_jobs(t, t->dec.blocks, P->dec_blocks, ws, jobs);
    TRY(vt_pack_weights_grouped(jobs.data(), (int)jobs.size(), s));
    hipLaunchKernelGGL(gather_f32_kernel, dim3((Kp + 255) / 256), dim3(256), 0, (hipStream_t)s, P->head_b, WS(int32_t, t->perm), Kp, WS(float, t->head_b_perm));
    TRY(vt_assemble_rows(WS(float, t->dec_query_sum), t->Nv, 0, 1, t->Nv, D, nullptr, P->dec_patch_query, P->dec_token_type, s));
    VT_CHECK_LAUNCH("vt_tokenizer_pack");
    return VT_OK;
}

// the input-gradient GEMMs of the engine carry the split-K workspace: at one or two clips per GPU the N = D GEMMs are 72 / 144 tiles
// and vt_gemm_nt splits their K (vtGemmNT.splitk_ws); at the headline batch nothing qualifies and the field is ignored
static vtGemmNT nt(const BlockEngine* t, void* ws, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, int epi, void* out,
                   int64_t ldo) {
    vtGemmNT p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.M = M; p.N = N; p.K = K; p.epi = epi; p.out = out; p.ldo = ldo;
    // backward only: the forward pass of a clip stays bit-identical whatever batch it runs in (sampled token ids, reconstructions);
    // its gradients already differ across batch sizes in the last fp32 bits (summation over the batch's rows)
    if (t->splitk_bytes && t->in_backward && t->splitk_on) { p.splitk_ws = WS(void, t->splitk); p.splitk_ws_bytes = (int64_t)t->splitk_bytes; }
    // data-parallel runs (vt_tokenizer_set_data_parallel): launches with more 192x192 tiles than one round of the chip go out one tile per
    // workgroup instead of as 256 persistent workgroups with fixed tile lists.  Equal speed on a free chip (62.9 vs 63.2 us on fc1 forward,
    // measured at whole rounds: 768 / 1024 tiles); with a collective's workgroups holding CUs the hardware dispatcher hands the remaining
    // tiles to whichever CU is free (4 rounds -> 5), where a persistent workgroup that could not start runs its whole list after the
    // others have finished theirs (x 1.67 measured with a single-GPU stand-in, tools/cu_thief_stats.sh -- not yet under a real collective)
    // (backward only: that is where the gradient all-reduce runs, and the forward's GELU launch would fill its look-up table once per tile)
    if (t->data_parallel && t->in_backward && M % 192 == 0 && N % 192 == 0 && (long)(M / 192) * (N / 192) > 256) p.tile = 6;
    return p;
}

static const LastBlock* kept_rows(const Side& sd, int i) { return i + 1 == (int)sd.blocks.size() && sd.last.enabled ? &sd.last : nullptr; }

// one timm Block forward: x_in -> x_out (both fp32 [M,D]).  kept: the last block of a stack (see LastBlock); rows outside the kept suffix
// of x_out are NOT written.  rope_cos / rope_sin (both or neither): q and k are rotated in place behind the
// qkv GEMM (ResidualAttentionBlock1, simpletransformer.py:46-53), so the saved qkv is the rotated one the attention backward needs.
static int block_forward(BlockEngine* e, const BlockBufs& b, const vtBlockTensors& w, const float* x_in, float* x_out, const LastBlock* kept,
                         void* ws, vtStream s, const float* rope_cos = nullptr, const float* rope_sin = nullptr) {
    const int M = e->M, D = e->D, D3 = e->D3, D4 = e->D4;
    const vtRowMap id = {0, 0, 0};
    const Rows r = kept ? kept->rows : Rows{id, M, e->Mp, 0};
    TRY(vt_layernorm_fwd(x_in, id, w.norm1_w, w.norm1_b, 1e-5f, M, D, WS(void, b.h1), WS(float, b.mean1), WS(float, b.rstd1), s));
    vtGemmNT g = nt(e, ws, WS(void, b.h1), D, WS(void, b.qkv_wb), D, M, D3, D, VT_EPI_BF16, WS(void, b.qkv), D3);
    TRY(vt_gemm_nt(&g, s));
    if (rope_cos) TRY(vt_rope_rotate(WS(void, b.qkv), D3, M, e->L, e->H, rope_cos, rope_sin, 0, s));
    TRY(vt_attention_fwd_rows(WS(void, b.qkv), e->B, e->L, e->H, D / e->H, r.q_begin, WS(void, b.o), WS(float, b.lse), s));
    g = nt(e, ws, WS(void, b.o), D, WS(void, b.proj_wb), D, r.n, D, D, VT_EPI_F32, WS(void, b.x_mid), D);
    g.bias = w.proj_b; g.residual = x_in; g.ldr = D; g.omap = r.map;
    TRY(vt_gemm_nt(&g, s));
    TRY(vt_layernorm_fwd(WS(float, b.x_mid), r.map, w.norm2_w, w.norm2_b, 1e-5f, r.n, D, WS(void, b.h2), WS(float, b.mean2), WS(float, b.rstd2), s));
    g = nt(e, ws, WS(void, b.h2), D, WS(void, b.fc1_wb), D, r.n, D4, D, VT_EPI_BF16_GELU_GRAD, WS(void, b.dgelu), D4);
    g.out2 = WS(void, b.g); g.ldo2 = D4; g.bias = w.fc1_b;
    TRY(vt_gemm_nt(&g, s));
    g = nt(e, ws, WS(void, b.g), D4, WS(void, b.fc2_wb), D4, r.n, D, D4, VT_EPI_F32, x_out, D);
    g.bias = w.fc2_b; g.residual = WS(float, b.x_mid); g.ldr = D; g.omap = r.map;
    TRY(vt_gemm_nt(&g, s));
    return VT_OK;
}

static int run_blocks_forward(BlockEngine* e, const Side& sd, const vtBlockTensors* w, void* ws, vtStream s, const float* rope_cos = nullptr,
                              const float* rope_sin = nullptr) {
    for (int i = 0; i < (int)sd.blocks.size(); ++i)
        TRY(block_forward(e, sd.blocks[i], w[i], WS(float, sd.x[i]), WS(float, sd.x[i + 1]), kept_rows(sd, i), ws, s, rope_cos, rope_sin));
    return VT_OK;
}

// out_linear of the bottleneck: the bf16 regularised latents in vq_rzpad ([Mq, 64]) -> encoded (fp32 [Mq, D], bf16-rounded under autocast)
static int out_linear(vtTokenizer* t, const vtTokenizerTensors* P, void* ws, float* encoded, vtStream s) {
    vtGemmNT g = nt(t, ws, WS(void, t->vq_rzpad), 64, WS(void, t->out_wb), 64, t->Mq, t->c.D, 64, VT_EPI_F32, encoded, t->c.D);
    g.bias = P->out_b; g.round_bf16 = 1;
    return vt_gemm_nt(&g, s);
}

// encode up to the bottleneck's in_linear: patch embed, encoder blocks, the two norm statistics, z = in_linear(latent rows) into zproj
// (fp32, row stride 64; d columns, 2d for a KL handle)
static int encode_trunk(vtTokenizer* t, const vtTokenizerTensors* P, const float* video, void* ws, float* input_norms, vtStream s) {
    const vtTokenizerConfig& c = t->c;
    const int D = c.D, L = t->L, Nv = t->Nv, Nq = c.Nq;
    // 1. patchify + patch-embed GEMM (+bias +sincos PE) written straight into rows [0,Nv) of every sequence
    TRY(vt_patchify(video, c.B, c.C, c.T, c.S, c.pt, c.p, WS(void, t->patches), s));
    float* x0 = WS(float, t->enc.x[0]);
    vtGemmNT g = nt(t, ws, WS(void, t->patches), t->Kp, WS(void, t->pe_wb), t->Kp, t->Mv, D, t->Kp, VT_EPI_F32, x0, D);
    g.bias = P->pe_b; g.rowmod = P->enc_patch_pe; g.rowmod_period = Nv; g.omap = vtRowMap{Nv, L, 0};
    g.round_bf16 = 1;  // conv output is bf16 under autocast before the fp32 PE add
    TRY(vt_gemm_nt(&g, s));
    // 2. learned latent queries broadcast into rows [Nv, L)   (larp_tokenizer.py:410, transformer.py:64)
    TRY(vt_assemble_rows(x0, L, Nv, c.B, Nq, D, nullptr, P->enc_query, nullptr, s));
    // 3. encoder blocks
    TRY(run_blocks_forward(t, t->enc, P->enc_blocks, ws, s));
    const float* xe = WS(float, t->enc.x[c.depth_enc]);
    const vtRowMap qmap = {Nq, L, Nv};  // the last Nq rows of every sequence (transformer.py:69)
    // 4. bottleneck: norm stats, in_linear (the regularizer and out_linear follow in the caller)
    if (input_norms)
        hipLaunchKernelGGL(rownorm_mean_kernel, dim3(2), dim3(512), 0, (hipStream_t)s, xe, (int64_t)L, (int64_t)Nv, (int64_t)L - 1, c.B, D, input_norms);
    TRY(vt_cast_rows(xe, qmap, t->Mq, D, WS(void, t->zb), D, s));
    g = nt(t, ws, WS(void, t->zb), D, WS(void, t->in_wb), D, t->Mq, t->kl ? 2 * c.d : c.d, D, VT_EPI_F32, WS(void, t->zproj), 64);
    g.bias = P->in_b; g.round_bf16 = 1;
    return vt_gemm_nt(&g, s);
}

extern "C" int vt_tokenizer_encode(vtTokenizer* t, const vtTokenizerTensors* P, const float* video, void* ws,
                                   const vtTokenizerOutputs* out, uint64_t seed, vtStream s) {
    VT_CHECK_ARG(t && P && video && ws && out, "vt_tokenizer_encode: null pointer");
    VT_CHECK_ARG(!t->kl, "vt_tokenizer_encode: the handle has the KL bottleneck (vt_tokenizer_create_kl): use vt_tokenizer_encode_kl");
    t->in_backward = false;
    VT_CHECK_ARG(out->encoded && out->indices && out->losses, "vt_tokenizer_encode: encoded/indices/losses outputs are required");
    const vtTokenizerConfig& c = t->c;
    TRY(encode_trunk(t, P, video, ws, out->input_norms, s));
    if (out->projected_z)
        hipLaunchKernelGGL(compact_cols_kernel, dim3((t->Mq * c.d + 255) / 256), dim3(256), 0, (hipStream_t)s, WS(float, t->zproj), (int64_t)64, t->Mq, c.d, out->projected_z);
    TRY(vt_vq_forward_ctr(WS(float, t->zproj), 64, P->codebook, t->Mq, c.K, c.d, c.vq_mode, c.l2_normalized, c.inv_tau, c.beta, c.codebook_w,
                      seed, t->seed_ctr, WS(float, t->vq_E), WS(float, t->vq_wnorm), WS(float, t->vq_zn), WS(float, t->vq_znorm), WS(int64_t, t->vq_idx),
                      WS(float, t->vq_rz), WS(void, t->vq_rzpad), 64, WS(float, t->vq_losses), WS(void, t->vq_ws), s));
    hipStream_t hs = (hipStream_t)s;
    TRY(copy_d2d(out->indices, WS(void, t->vq_idx), (size_t)t->Mq * 8, hs));
    TRY(copy_d2d(out->losses, WS(void, t->vq_losses), 16, hs));
    if (out->unregularized_z) TRY(copy_d2d(out->unregularized_z, WS(void, t->vq_zn), (size_t)t->Mq * c.d * 4, hs));
    if (out->regularized_z) TRY(copy_d2d(out->regularized_z, WS(void, t->vq_rz), (size_t)t->Mq * c.d * 4, hs));
    if (out->emb) TRY(copy_d2d(out->emb, WS(void, t->vq_E), (size_t)c.K * c.d * 4, hs));
    TRY(out_linear(t, P, ws, out->encoded, s));
    VT_CHECK_LAUNCH("vt_tokenizer_encode");
    return VT_OK;
}

// KL bottleneck: z = in_linear(x) [Mq, 2d] -> vt_kl_forward (mean, sample, eps, loss_kl; bf16 sample into vq_rzpad) -> out_linear(sample)
extern "C" int vt_tokenizer_encode_kl(vtTokenizer* t, const vtTokenizerTensors* P, const float* video, void* ws,
                                      const vtTokenizerKLOutputs* out, uint64_t seed, vtStream s) {
    VT_CHECK_ARG(t && P && video && ws && out, "vt_tokenizer_encode_kl: null pointer");
    VT_CHECK_ARG(t->kl, "vt_tokenizer_encode_kl: the handle has the VQ bottleneck (vt_tokenizer_create): use vt_tokenizer_encode");
    VT_CHECK_ARG(out->encoded && out->loss_kl, "vt_tokenizer_encode_kl: encoded/loss_kl outputs are required");
    t->in_backward = false;
    const vtTokenizerConfig& c = t->c;
    const int pd = 2 * c.d;
    TRY(encode_trunk(t, P, video, ws, out->input_norms, s));
    if (out->projected_z)
        hipLaunchKernelGGL(compact_cols_kernel, dim3((t->Mq * pd + 255) / 256), dim3(256), 0, (hipStream_t)s, WS(float, t->zproj), (int64_t)64, t->Mq, pd, out->projected_z);
    TRY(vt_kl_forward(WS(float, t->zproj), 64, t->Mq, c.d, c.B, seed, t->seed_ctr, out->mean, out->regularized_z, WS(void, t->vq_rzpad), 64,
                      WS(float, t->kl_noise), out->loss_kl, WS(void, t->kl_ws), s));
    if (out->noise) TRY(copy_d2d(out->noise, WS(void, t->kl_noise), (size_t)t->Mq * c.d * 4, (hipStream_t)s));
    TRY(out_linear(t, P, ws, out->encoded, s));
    VT_CHECK_LAUNCH("vt_tokenizer_encode_kl");
    return VT_OK;
}

extern "C" int vt_tokenizer_codes_to_encoded(vtTokenizer* t, const vtTokenizerTensors* P, const int64_t* indices, void* ws,
                                             float* encoded, vtStream s) {
    VT_CHECK_ARG(t && P && indices && ws && encoded, "vt_tokenizer_codes_to_encoded: null pointer");
    VT_CHECK_ARG(!t->kl, "vt_tokenizer_codes_to_encoded: the handle has the KL bottleneck (no codebook)");
    t->in_backward = false;
    const vtTokenizerConfig& c = t->c;
    TRY(vt_vq_prep_codebook(P->codebook, c.K, c.d, c.l2_normalized, WS(float, t->vq_E), WS(float, t->vq_wnorm), WS(void, t->vq_ws), s));
    TRY(vt_vq_gather(WS(float, t->vq_E), indices, t->Mq, c.K, c.d, nullptr, WS(void, t->vq_rzpad), 64, s));
    return out_linear(t, P, ws, encoded, s);
}

extern "C" int vt_tokenizer_decode(vtTokenizer* t, const vtTokenizerTensors* P, const float* encoded, void* ws, float* pred, vtStream s) {
    VT_CHECK_ARG(t && P && encoded && ws && pred, "vt_tokenizer_decode: null pointer");
    t->in_backward = false;
    const vtTokenizerConfig& c = t->c;
    const int D = c.D, L = t->L, Nv = t->Nv, Nq = c.Nq;
    float* x0 = WS(float, t->dec.x[0]);
    // decoder sequence = [encoded + latent PE | patch queries (+ token type)]   (larp_tokenizer.py:463-466)
    TRY(vt_assemble_rows(x0, L, 0, c.B, Nq, D, encoded, P->dec_latent_pe, nullptr, s));
    TRY(vt_assemble_rows(x0, L, Nq, c.B, Nv, D, nullptr, WS(float, t->dec_query_sum), nullptr, s));
    TRY(run_blocks_forward(t, t->dec, P->dec_blocks, ws, s));
    // head on the last Nv rows: LayerNorm(1e-6) -> Linear (rows permuted to (c,dt,dy,dx)) -> unpatchify
    const vtRowMap vmap = {Nv, L, Nq};
    TRY(vt_layernorm_fwd(WS(float, t->dec.x[c.depth_dec]), vmap, P->head_norm_w, P->head_norm_b, 1e-6f, t->Mv, D, WS(void, t->hN),
                         WS(float, t->meanH), WS(float, t->rstdH), s));
    vtGemmNT g = nt(t, ws, WS(void, t->hN), D, WS(void, t->head_wb), D, t->Mv, t->Kp, D, VT_EPI_F32, WS(void, t->yrows), t->Kp);
    g.bias = WS(float, t->head_b_perm);
    TRY(vt_gemm_nt(&g, s));
    TRY(vt_unpatchify(WS(float, t->yrows), c.B, c.C, c.T, c.S, c.pt, c.p, pred, s));
    return VT_OK;
}

static vtGemmTN tn(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int P, int Q, float* out, int64_t ldo) {
    vtGemmTN p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.M = M; p.P = P; p.Q = Q; p.out = out; p.ldo = ldo; p.p_lim = P; p.q_lim = Q;
    return p;
}

// A weight gradient whose output is only a few tiles (bottleneck in/out_linear: D x d) would occupy a handful of the
// 256 CUs for the whole token dimension.  Split the tokens into up to 16 slabs, run them as one grouped launch into
// partial outputs, and add the slabs in a fixed order.
static int skinny_wgrad(vtTokenizer* t, vtGemmTN w, void* ws, vtStream s) {
    int ns = 16;
    while (ns > 1 && (w.M % (64 * ns)) != 0) ns >>= 1;
    if (ns == 1) return vt_gemm_tn_grouped(&w, 1, s);
    const int rows = w.M / ns;
    const size_t slab = (size_t)w.p_lim * w.q_lim;
    vtGemmTN pr[16];
    float* part = WS(float, t->wg_slabs);
    for (int i = 0; i < ns; ++i) {
        pr[i] = w;
        pr[i].A = (const char*)w.A + (size_t)i * rows * w.lda * 2;
        pr[i].B = (const char*)w.B + (size_t)i * rows * w.ldb * 2;
        pr[i].M = rows;
        pr[i].out = part + i * slab;
        pr[i].ldo = w.q_lim;
    }
    TRY(vt_gemm_tn_grouped(pr, ns, s));
    if (w.ldo == w.q_lim) return vt_sum_slabs(part, ns, (int64_t)slab, (int)slab, w.out, s);
    vt_set_error("skinny_wgrad: output must be dense");
    return VT_ERR_INVALID;
}

// the main stream is about to rewrite gradient set `set`: wait for the side-stream group that still reads it
static int wait_set(BlockEngine* t, int set, vtStream s) {
    if (t->wg_stream && t->set_flush[set] >= 0) {
        if (hipStreamWaitEvent((hipStream_t)s, t->ev_done[t->set_flush[set] % BlockEngine::NEV], 0) != hipSuccess) { vt_set_error("wait_set: hipStreamWaitEvent failed"); return VT_ERR_LAUNCH; }
        t->set_flush[set] = -1;
    }
    return VT_OK;
}
// all side-stream groups of this backward are done before the main stream goes on (end of backward)
static int join_wgrad_stream(BlockEngine* t, vtStream s) {
    if (t->wg_stream && t->flush_id > 0) {
        if (hipStreamWaitEvent((hipStream_t)s, t->ev_done[(t->flush_id - 1) % BlockEngine::NEV], 0) != hipSuccess) { vt_set_error("join_wgrad_stream: hipStreamWaitEvent failed"); return VT_ERR_LAUNCH; }
        for (int i = 0; i < BlockEngine::NSETS_MAX; ++i) t->set_flush[i] = -1;   // the side stream runs its groups in order
    }
    return VT_OK;
}

static int flush_wgrads(BlockEngine* t, int stage_done, vtStream main_s) {
    vtStream s = main_s;
    if (t->wg_stream) {
        hipEvent_t fork = t->ev_fork[t->flush_id % BlockEngine::NEV];
        if (hipEventRecord(fork, (hipStream_t)main_s) != hipSuccess || hipStreamWaitEvent(t->wg_stream, fork, 0) != hipSuccess) { vt_set_error("flush_wgrads: fork failed"); return VT_ERR_LAUNCH; }
        s = (vtStream)t->wg_stream;
    }
    for (size_t i = 0; i < t->pending.size(); i += VT_TN_MAX_GROUP) {
        const int n = (int)((t->pending.size() - i) < VT_TN_MAX_GROUP ? (t->pending.size() - i) : VT_TN_MAX_GROUP);
        TRY(vt_gemm_tn_grouped(t->pending.data() + i, n, s));
    }
    t->pending.clear();
    for (size_t i = 0; i < t->pending_red.size(); i += VT_REDUCE_MAX_GROUP) {
        const int n = (int)((t->pending_red.size() - i) < VT_REDUCE_MAX_GROUP ? (t->pending_red.size() - i) : VT_REDUCE_MAX_GROUP);
        TRY(vt_reduce_grouped(t->pending_red.data() + i, n, s));
    }
    t->pending_red.clear();
    t->pending_blocks = 0;
    t->final_through = stage_done;
    if (t->wg_stream) {
        if (hipEventRecord(t->ev_done[t->flush_id % BlockEngine::NEV], t->wg_stream) != hipSuccess) { vt_set_error("flush_wgrads: event record failed"); return VT_ERR_LAUNCH; }
        for (int set : t->sets_pending) t->set_flush[set] = t->flush_id;
        t->flush_id++;
    }
    t->sets_pending.clear();
    return VT_OK;
}

// queue the reduction of a LayerNorm backward's partials / of the gelu' epilogue's column sums
static void queue_ln_reduce(BlockEngine* t, const float* part, int nslab, int D, float* dgamma, float* dbeta, float* dxsum) {
    vtReduceItem q;
    q.partial = part; q.nslab = nslab; q.width = D; q.nout = dxsum ? 3 : 2; q.lanes = nslab >= 128 ? 32 : 8; q.slab_stride = (int64_t)3 * D;
    q.o[0] = dgamma; q.o[1] = dbeta; q.o[2] = dxsum;
    t->pending_red.push_back(q);
}
static void queue_slab_sum(BlockEngine* t, const float* part, int nslab, int width, float* out) {
    vtReduceItem q;
    q.partial = part; q.nslab = nslab; q.width = width; q.nout = 1; q.lanes = nslab >= 128 ? 32 : 8; q.slab_stride = width;
    q.o[0] = out; q.o[1] = q.o[2] = nullptr;
    t->pending_red.push_back(q);
}

// Backward of one block.  In: dX (fp32) and gs[set].dx_out (bf16) hold dL/dx_out.  Out: dX holds dL/dx_in and its bf16
// copy goes to gs[next set].dx_out.  The four weight-gradient GEMMs are queued (e->pending), not launched.
// prev_bias_grad: where sum_rows(dL/dx_in) goes (= bias gradient of whatever produced x_in), may be NULL.
// kept: the last block of a stack (see LastBlock).  dL/dx_out is zero outside the kept rows, so the MLP half, proj and the query side of
// attention run on the compact kept rows; qkv input gradient, K/V gradients and LayerNorm1 cover all rows as usual.
// rope_cos / rope_sin: the block's forward rotated q and k; dq and dk are rotated back (conjugate) before anything reads dqkv.
// (kept together with rope tables has no caller -- the tokenizer passes no tables, a vtStack keeps every row -- and has never been run.)
static int block_backward(BlockEngine* e, const BlockBufs& b, const vtBlockTensors& w, const vtBlockTensors& gr, const float* x_in,
                          float* prev_bias_grad, const LastBlock* kept, void* ws, vtStream s, const float* rope_cos = nullptr,
                          const float* rope_sin = nullptr) {
    const int M = e->M, Mp = e->Mp, D = e->D, D3 = e->D3, D4 = e->D4;
    const vtRowMap id = {0, 0, 0};
    const Rows r = kept ? kept->rows : Rows{id, M, Mp, 0};
    const int set_next = (e->set_idx + 1) % e->nsets();
    TRY(wait_set(e, e->set_idx, s));
    TRY(wait_set(e, set_next, s));
    e->sets_pending.push_back(e->set_idx);
    const BlockEngine::GradSet& g0 = e->gs[e->set_idx];
    const BlockEngine::GradSet& g1 = e->gs[set_next];
    float* dX = WS(float, e->dX);
    void* dXa = WS(void, kept ? kept->dxa : g0.dx_out);   // kept: compact bf16 copies of dL/dx_out and dL/dx_mid, and du: rows >= r.n stay zero
    void* dXm = WS(void, kept ? kept->dxm : g0.dx_mid);
    void* du = WS(void, kept ? kept->du : g0.du);
    void* dqkv = WS(void, g0.dqkv);
    if (kept) TRY(vt_cast_rows(dX, r.map, r.n, D, dXa, D, s));
    // fc2 dgrad fused with GELU': du = (dx_out . W2) * gelu'(u), gelu'(u) as the fc1 forward saved it (bf16)
    vtGemmNT g = nt(e, ws, dXa, D, WS(void, b.fc2_wt), D, r.n, D4, D, VT_EPI_BF16_MULAUX, du, D4);
    g.aux = WS(void, b.dgelu); g.ldaux = D4;
    g.colsum_partial = WS(float, g0.cs_part);  // fc1 bias gradient = column sums of du, taken in the epilogue; summed at the flush
    TRY(vt_gemm_nt(&g, s));
    queue_slab_sum(e, WS(float, g0.cs_part), (r.n + 191) / 192, D4, gr.fc1_b);
    // fc1 dgrad
    g = nt(e, ws, du, D4, WS(void, b.fc1_wt), D4, r.n, D, D4, VT_EPI_BF16, WS(void, e->dh), D);
    TRY(vt_gemm_nt(&g, s));
    // LayerNorm2 backward + residual: dx_mid = dx_out + ln_bwd(dh2) (in place in dX; bf16 copy -> dXm, compact for kept rows); column sum = proj bias grad
    int nsl = 0;
    TRY(vt_layernorm_bwd_partials(WS(void, e->dh), WS(float, b.x_mid), r.map, w.norm2_w, WS(float, b.mean2), WS(float, b.rstd2), dX, r.n, D, dX,
                                  kept ? nullptr : dXm, WS(float, g0.ln_part2), &nsl, s));
    queue_ln_reduce(e, WS(float, g0.ln_part2), nsl, D, gr.norm2_w, gr.norm2_b, gr.proj_b);
    if (kept) TRY(vt_cast_rows(dX, r.map, r.n, D, dXm, D, s));
    // proj dgrad
    g = nt(e, ws, dXm, D, WS(void, b.proj_wt), D, r.n, D, D, VT_EPI_BF16, WS(void, e->dob), D);
    TRY(vt_gemm_nt(&g, s));
    // attention backward
    TRY(attn_bwd(e, ws, WS(void, b.qkv), WS(void, b.o), WS(void, e->dob), WS(float, b.lse), r.q_begin, dqkv, s));
    if (rope_cos) TRY(vt_rope_rotate(dqkv, D3, M, e->L, e->H, rope_cos, rope_sin, 1, s));
    // qkv dgrad
    g = nt(e, ws, dqkv, D3, WS(void, b.qkv_wt), D3, M, D, D3, VT_EPI_BF16, WS(void, e->dh), D);
    TRY(vt_gemm_nt(&g, s));
    // the block's four weight gradients: queued for the grouped launch
    e->pending.push_back(tn(dXa, D, WS(void, b.g), D4, r.n_pad, D, D4, gr.fc2_w, D4));
    e->pending.push_back(tn(du, D4, WS(void, b.h2), D, r.n_pad, D4, D, gr.fc1_w, D));
    e->pending.push_back(tn(dXm, D, WS(void, b.o), D, r.n_pad, D, D, gr.proj_w, D));
    e->pending.push_back(tn(dqkv, D3, WS(void, b.h1), D, Mp, D3, D, gr.qkv_w, D));
    e->pending_blocks++;
    // LayerNorm1 backward + residual: dx_in = dx_mid + ln_bwd(dh) (in place; bf16 copy -> next set's dx_out)
    TRY(vt_layernorm_bwd_partials(WS(void, e->dh), x_in, id, w.norm1_w, WS(float, b.mean1), WS(float, b.rstd1), dX, M, D, dX, WS(void, g1.dx_out),
                                  WS(float, g0.ln_part1), &nsl, s));
    queue_ln_reduce(e, WS(float, g0.ln_part1), nsl, D, gr.norm1_w, gr.norm1_b, prev_bias_grad);
    e->set_idx = set_next;
    return VT_OK;
}

// The backward stage of block i of a side, then the flush rule of its weight gradients: one grouped launch once wg_batch blocks are queued,
// at the side's first block, or where the caller asks for it (flush_now).  need_wgrad = false: a frozen stack (generator-side pass through
// the discriminator) wants the input gradient only, so the queued GEMMs and reductions are dropped.
static int backward_block_stage(BlockEngine* e, const Side& sd, int i, const vtBlockTensors* w, const vtBlockTensors* gr, bool need_wgrad,
                                bool flush_now, int stage_done, void* ws, vtStream s, const float* rope_cos = nullptr,
                                const float* rope_sin = nullptr) {
    TRY(block_backward(e, sd.blocks[i], w[i], gr[i], WS(float, sd.x[i]), i > 0 ? gr[i - 1].fc2_b : nullptr, kept_rows(sd, i), ws, s, rope_cos,
                       rope_sin));
    if (!need_wgrad) {
        e->pending.clear();
        e->pending_red.clear();
        e->pending_blocks = 0;
    } else if (e->pending_blocks >= e->wg_batch || i == 0 || flush_now) {
        TRY(flush_wgrads(e, stage_done, s));
    }
    return VT_OK;
}

extern "C" int vt_tokenizer_backward(vtTokenizer* t, const vtTokenizerTensors* P, const float* d_pred, const float* gscal, void* ws,
                                     const vtTokenizerTensors* G, int32_t stage_begin, int32_t stage_end, int32_t* final_through,
                                     vtStream s) {
    VT_CHECK_ARG(t && P && ws && G && G->enc_blocks && G->dec_blocks, "vt_tokenizer_backward: null pointer");
    t->in_backward = true;
    const vtTokenizerConfig& c = t->c;
    const int nstage = vt_tokenizer_num_backward_stages(t);
    VT_CHECK_ARG(stage_begin >= 0 && stage_end <= nstage && stage_begin <= stage_end, "vt_tokenizer_backward: bad stage range");
    const int D = c.D, L = t->L, Nv = t->Nv, Nq = c.Nq, Kp = t->Kp;
    const vtRowMap id = {0, 0, 0};
    const vtRowMap vmap = {Nv, L, Nq};   // decoder: last Nv rows
    const vtRowMap qmap = {Nq, L, Nv};   // encoder: last Nq rows
    const vtRowMap lmap = {Nq, L, 0};    // decoder: first Nq rows (latents)
    const vtRowMap tmap = {Nv, L, 0};    // encoder: first Nv rows (video tokens)
    hipStream_t hs = (hipStream_t)s;
    float* dX = WS(float, t->dX);
    for (int st = stage_begin; st < stage_end; ++st) {
        if (st == 0) {
            t->pending.clear();
            t->pending_red.clear(); t->pending_blocks = 0; t->set_idx = 0; t->final_through = 0;
            t->sets_pending.clear();
            TRY(join_wgrad_stream(t, s));    // (a previous backward that was not run to its last stage)
            // ---- head: d_pred -> patch rows (c,dt,dy,dx) -> dgrad / wgrad -> LayerNorm backward into the last Nv rows
            VT_CHECK_ARG(d_pred, "vt_tokenizer_backward: stage 0 needs d_pred");
            TRY(vt_patchify(d_pred, c.B, c.C, c.T, c.S, c.pt, c.p, WS(void, t->dY), s));
            vtGemmNT g = nt(t, ws, WS(void, t->dY), Kp, WS(void, t->head_wt), Kp, t->Mv, D, Kp, VT_EPI_BF16, WS(void, t->dhN), D);
            TRY(vt_gemm_nt(&g, s));
            vtGemmTN w = tn(WS(void, t->dY), Kp, WS(void, t->hN), D, t->Mvp, Kp, D, G->head_w, D);
            w.row_perm = WS(int32_t, t->perm);
            TRY(vt_gemm_tn_grouped(&w, 1, s));
            TRY(vt_colsum(WS(void, t->dY), 1, Kp, id, t->Mv, Kp, WS(float, t->tmp_vec), WS(void, t->cs_ws), s));
            hipLaunchKernelGGL(scatter_f32_kernel, dim3((Kp + 255) / 256), dim3(256), 0, hs, WS(float, t->tmp_vec), WS(int32_t, t->perm), Kp, G->head_b);
            // rows < Nq of the last decoder block's output are dropped by the slice => zero gradient
            TRY(vt_zero_rows(dX, WS(void, t->gs[0].dx_out), lmap, t->Mq, D, s));
            TRY(vt_layernorm_bwd(WS(void, t->dhN), WS(float, t->dec.x[c.depth_dec]), vmap, P->head_norm_w, WS(float, t->meanH), WS(float, t->rstdH),
                                 nullptr, t->Mv, D, dX, WS(void, t->gs[0].dx_out), G->head_norm_w, G->head_norm_b,
                                 nullptr, WS(void, t->ln_ws), s));
            // fc2 bias grad of the last decoder block = column sum of dL/dx_out (all rows; zero rows add nothing)
            TRY(vt_colsum(dX, 0, D, id, t->M, D, G->dec_blocks[c.depth_dec - 1].fc2_b, WS(void, t->cs_ws), s));
            t->final_through = 1;
        } else if (st <= c.depth_dec) {
            const int i = c.depth_dec - st;  // decoder blocks, last first
            TRY(backward_block_stage(t, t->dec, i, P->dec_blocks, G->dec_blocks, true, false, st + 1, ws, s));
        } else if (st == c.depth_dec + 1) {
            // ---- bottleneck.  dX holds dL/d(decoder input sequence)
            if (G->dec_token_type) TRY(vt_colsum(dX, 0, D, vmap, t->Mv, D, G->dec_token_type, WS(void, t->cs_ws), s));
            TRY(vt_cast_rows(dX, lmap, t->Mq, D, WS(void, t->dEncb), D, s));  // d encoded (bf16 under autocast)
            TRY(vt_colsum(WS(void, t->dEncb), 1, D, id, t->Mq, D, G->out_b, WS(void, t->cs_ws), s));
            // out_linear: dgrad -> d regularized_z [Mq,64]; wgrad -> dW_out [D,d]
            vtGemmNT g = nt(t, ws, WS(void, t->dEncb), D, WS(void, t->out_wt), D, t->Mq, 64, D, VT_EPI_F32, WS(void, t->d_rz), 64);
            TRY(vt_gemm_nt(&g, s));
            vtGemmTN w = tn(WS(void, t->dEncb), D, WS(void, t->vq_rzpad), 64, t->Mqp, D, 64, G->out_w, c.d);
            w.q_lim = c.d;
            TRY(skinny_wgrad(t, w, ws, s));
            const int pd = t->kl ? 2 * c.d : c.d;   // in_linear outputs
            if (t->kl) {
                // KL backward: reparameterised sample + KL term to the interleaved (mean, logvar) columns of z
                TRY(vt_kl_backward(WS(float, t->d_rz), 64, nullptr, gscal, WS(float, t->zproj), 64, WS(float, t->kl_noise), t->Mq, c.d, c.B, nullptr,
                                   WS(void, t->dz_pad), 64, s));
            } else {
                // VQ backward: straight-through + commitment to z, codebook loss to the embedding
                TRY(vt_vq_backward(WS(float, t->d_rz), 64, gscal, c.beta, c.codebook_w, WS(float, t->vq_zn), WS(float, t->vq_znorm), WS(float, t->vq_E),
                                   WS(float, t->vq_wnorm), WS(int64_t, t->vq_idx), t->Mq, c.K, c.d, c.l2_normalized, nullptr, WS(void, t->dz_pad), 64,
                                   c.freeze_codebook ? nullptr : G->codebook, WS(void, t->vq_ws), s));
            }
            // in_linear: bias grad, wgrad, dgrad scattered into the last Nq rows of the encoder output gradient
            TRY(vt_colsum(WS(void, t->dz_pad), 1, 64, id, t->Mq, 64, WS(float, t->tmp_vec), WS(void, t->cs_ws), s));
            TRY(copy_d2d(G->in_b, WS(void, t->tmp_vec), (size_t)pd * 4, hs));
            w = tn(WS(void, t->dz_pad), 64, WS(void, t->zb), D, t->Mqp, 64, D, G->in_w, D);
            w.p_lim = pd;
            TRY(skinny_wgrad(t, w, ws, s));
            // (the encoder goes on in the rotation of gradient sets where the decoder stopped: with the weight gradients on their own
            // stream, set 0 may still be read by the decoder's last group)
            TRY(wait_set(t, t->set_idx, s));
            TRY(vt_zero_rows(dX, WS(void, t->gs[t->set_idx].dx_out), tmap, t->Mv, D, s));  // video-token rows get no gradient from the bottleneck
            g = nt(t, ws, WS(void, t->dz_pad), 64, WS(void, t->in_wt), 64, t->Mq, D, 64, VT_EPI_F32, dX, D);
            g.out2 = WS(void, t->gs[t->set_idx].dx_out); g.ldo2 = D; g.omap = qmap;
            TRY(vt_gemm_nt(&g, s));
            TRY(vt_colsum(dX, 0, D, id, t->M, D, G->enc_blocks[c.depth_enc - 1].fc2_b, WS(void, t->cs_ws), s));
            t->final_through = st + 1;
        } else if (st <= c.depth_dec + 1 + c.depth_enc) {
            const int i = c.depth_enc - (st - c.depth_dec - 1);   // encoder blocks, last first; the first wg_tail flush block by block
            TRY(backward_block_stage(t, t->enc, i, P->enc_blocks, G->enc_blocks, true, i < t->wg_tail, st + 1, ws, s));
        } else {
            // ---- patch embed + learned queries.  dX holds dL/d(encoder input sequence)
            TRY(vt_batch_sum(dX, qmap, c.B, Nq, D, G->enc_query, s));
            TRY(vt_cast_rows(dX, tmap, t->Mv, D, WS(void, t->dTok), D, s));
            TRY(vt_colsum(WS(void, t->dTok), 1, D, id, t->Mv, D, G->pe_b, WS(void, t->cs_ws), s));
            vtGemmTN w = tn(WS(void, t->dTok), D, WS(void, t->patches), Kp, t->Mvp, D, Kp, G->pe_w, Kp);
            TRY(vt_gemm_tn_grouped(&w, 1, s));
            TRY(join_wgrad_stream(t, s));    // every gradient of the step is behind the caller's stream from here on
            t->final_through = st + 1;
        }
    }
    if (final_through) *final_through = t->final_through;
    VT_CHECK_LAUNCH("vt_tokenizer_backward");
    return VT_OK;
}

// The same, for a caller that reduces finished gradient slices between stages (parallel.GradReducer): runs stages from stage_begin until
// *final_through advances (a group of weight gradients was flushed) or the last stage is done, and returns the stage to go on with in
// *stage_next.  One call per reported slice (~8 per backward at 12 + 12 blocks) instead of one per stage (27): the host side of the
// reference's own recipe, one clip per GPU under data parallelism, is what this shortens.
extern "C" int vt_tokenizer_backward_until_flush(vtTokenizer* t, const vtTokenizerTensors* P, const float* d_pred, const float* gscal, void* ws,
                                                 const vtTokenizerTensors* G, int32_t stage_begin, int32_t* stage_next, int32_t* final_through,
                                                 vtStream s) {
    VT_CHECK_ARG(t && stage_next && final_through, "vt_tokenizer_backward_until_flush: null pointer");
    const int nstage = vt_tokenizer_num_backward_stages(t);
    VT_CHECK_ARG(stage_begin >= 0 && stage_begin < nstage, "vt_tokenizer_backward_until_flush: bad first stage");
    const int before = stage_begin == 0 ? 0 : t->final_through;
    int st = stage_begin;
    int32_t ft = before;
    do {
        TRY(vt_tokenizer_backward(t, P, d_pred, gscal, ws, G, st, st + 1, &ft, s));
        ++st;
    } while (st < nstage && ft == before);
    *stage_next = st;
    *final_through = ft;
    return VT_OK;
}


// ------------------------------------------------------------------------------------------------
// A stack of timm Blocks on its own: transformer_encoder_parallel / transformer_encoder_fused called outside the
// tokenizer (models/transformer.py:8-70) and the discriminator's encoder (models/loss.py:150-155).  Same block
// machinery and workspace discipline as the tokenizer (a BlockEngine with one Side); head_dim 64 or 32, any L.
// One workspace per forward whose backward is still pending.
// ------------------------------------------------------------------------------------------------
extern "C" int vt_stack_create(const vtStackConfig* cfg, vtStack** out) {
    VT_CHECK_ARG(cfg && out, "vt_stack_create: null pointer");
    const int B = cfg->B, L = cfg->L, D = cfg->D, H = cfg->H, depth = cfg->depth;
    VT_CHECK_ARG(B > 0 && L > 0 && depth > 0 && H > 0 && D % H == 0 && (D / H == 64 || D / H == 32),
                 "vt_stack_create: B=%d L=%d D=%d H=%d depth=%d (head_dim must be 64 or 32)", B, L, D, H, depth);
    VT_CHECK_ARG(D == 128 || D == 384 || (D % 256 == 0 && D <= 1024), "vt_stack_create: width %d unsupported (128, 256, 384, 512, 768, 1024)", D);
    vtStack* t = new vtStack();
    block_geometry(t, B, L, H, D);
    Arena a;
    plan_blocks(t, a, t->side, depth);
    plan_residuals(t, a, t->side);
    plan_block_scratch(t, a, {}, t->D4);   // every row of the stack is returned: no kept-rows last block
    t->ws_bytes = a.off;
    *out = t;
    return VT_OK;
}

extern "C" void vt_stack_destroy(vtStack* t) { delete t; }
extern "C" size_t vt_stack_workspace_bytes(const vtStack* t) { return t ? t->ws_bytes : 0; }

extern "C" int vt_stack_init_workspace(vtStack* t, void* ws, vtStream stream) {
    VT_CHECK_ARG(t && ws, "vt_stack_init_workspace: null pointer");
    if (hipMemsetAsync(ws, 0, t->ws_bytes, (hipStream_t)stream) != hipSuccess) { vt_set_error("vt_stack_init_workspace: memset failed"); return VT_ERR_LAUNCH; }
    return VT_OK;
}

// cos_tab / sin_tab of the rotary variants: NULL (both) = the plain stack, bit for bit; a rotary stack needs head_dim 64 and vt_rope.hip
static int check_rotary(const vtStack* t, const float* cos_tab, const float* sin_tab, const char* fn) {
    VT_CHECK_ARG((cos_tab == nullptr) == (sin_tab == nullptr), "%s: cos_tab and sin_tab must both be given or both be NULL", fn);
    if (!cos_tab) return VT_OK;
    VT_CHECK_ARG(vt_rope_rotate != nullptr, "%s: the rotary kernel (vt_rope.hip) is not linked into this library", fn);
    VT_CHECK_ARG(t->D == 64 * t->H, "%s: rotary q/k need head_dim 64 (D=%d H=%d)", fn, t->D, t->H);
    return VT_OK;
}

extern "C" int vt_stack_forward_rotary(vtStack* t, const vtBlockTensors* blocks, const float* cos_tab, const float* sin_tab, const float* x_in,
                                       void* ws, float* x_out, vtStream s) {
    const char* fn = (cos_tab || sin_tab) ? "vt_stack_forward_rotary" : "vt_stack_forward";
    VT_CHECK_ARG(t && blocks && x_in && ws && x_out, "%s: null pointer", fn);
    TRY(check_rotary(t, cos_tab, sin_tab, "vt_stack_forward_rotary"));
    t->in_backward = false;
    const size_t bytes = (size_t)t->M * t->D * 4;
    hipStream_t hs = (hipStream_t)s;
    TRY(copy_d2d(WS(void, t->side.x.front()), x_in, bytes, hs));
    std::vector<vtPackJob> jobs;
    pack_block_jobs(t, t->side.blocks, blocks, ws, jobs);
    TRY(vt_pack_weights_grouped(jobs.data(), (int)jobs.size(), s));
    TRY(run_blocks_forward(t, t->side, blocks, ws, s, cos_tab, sin_tab));
    TRY(copy_d2d(x_out, WS(void, t->side.x.back()), bytes, hs));
    VT_CHECK_LAUNCH(fn);
    return VT_OK;
}

extern "C" int vt_stack_forward(vtStack* t, const vtBlockTensors* blocks, const float* x_in, void* ws, float* x_out, vtStream s) {
    return vt_stack_forward_rotary(t, blocks, nullptr, nullptr, x_in, ws, x_out, s);
}

extern "C" int vt_stack_backward_rotary(vtStack* t, const vtBlockTensors* blocks, const float* cos_tab, const float* sin_tab, const float* dy,
                                        void* ws, const vtBlockTensors* grads, float* dx, int32_t need_wgrad, vtStream s) {
    const char* fn = (cos_tab || sin_tab) ? "vt_stack_backward_rotary" : "vt_stack_backward";
    VT_CHECK_ARG(t && blocks && dy && ws && grads && dx, "%s: null pointer", fn);
    TRY(check_rotary(t, cos_tab, sin_tab, "vt_stack_backward_rotary"));
    t->in_backward = true;
    const int depth = (int)t->side.blocks.size(), D = t->D;
    const size_t bytes = (size_t)t->M * D * 4;
    const vtRowMap id = {0, 0, 0};
    hipStream_t hs = (hipStream_t)s;
    float* dX = WS(float, t->dX);
    t->pending.clear();
    t->pending_red.clear(); t->pending_blocks = 0; t->set_idx = 0; t->final_through = 0;
    TRY(copy_d2d(dX, dy, bytes, hs));
    TRY(vt_cast_rows(dX, id, t->M, D, WS(void, t->gs[0].dx_out), D, s));
    TRY(vt_colsum(dX, 0, D, id, t->M, D, grads[depth - 1].fc2_b, WS(void, t->cs_ws), s));
    for (int i = depth - 1; i >= 0; --i) TRY(backward_block_stage(t, t->side, i, blocks, grads, need_wgrad != 0, false, 0, ws, s, cos_tab, sin_tab));
    TRY(copy_d2d(dx, dX, bytes, hs));
    VT_CHECK_LAUNCH(fn);
    return VT_OK;
}

extern "C" int vt_stack_backward(vtStack* t, const vtBlockTensors* blocks, const float* dy, void* ws, const vtBlockTensors* grads,
                                 float* dx, int32_t need_wgrad, vtStream s) {
    return vt_stack_backward_rotary(t, blocks, nullptr, nullptr, dy, ws, grads, dx, need_wgrad, s);
}
