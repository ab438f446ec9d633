/* vt_hip.h -- C ABI of libvt_hip.so: the MI355X (gfx950) kernels behind the LARP tokenizer's
 * encode -> quantize -> decode training step.
 *
 * The reference (zhxie0117/video-tokenizer) is pure Python and has NO FFI of its own: the path
 * sits behind its model registry (models/models.py:8-27) and runs torch / timm library ops.
 * This header is the boundary the build introduces beneath those Python classes; each entry
 * point names the reference line whose arithmetic it replaces.  The Python side that binds
 * it (ctypes, tensor.data_ptr(), torch.cuda.current_stream().cuda_stream) is in
 * video-tokenizer_amd/hip.py; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - every function enqueues work on `stream` (a hipStream_t) and returns immediately;
 *     nothing here allocates, frees or synchronises (hipGraph-capturable).
 *   - the caller owns every buffer (outputs, saved-for-backward, workspaces); sizes come
 *     from the matching *_workspace_bytes().
 *   - return 0 on success, <0 on error; vt_last_error() gives the thread-local message.
 *   - "bf16" buffers are raw 16-bit bfloat16; `void*` is used for them in signatures.
 */
#ifndef VT_HIP_H
#define VT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* vtStream; /* hipStream_t */

enum { VT_OK = 0, VT_ERR_INVALID = -1, VT_ERR_LAUNCH = -2, VT_ERR_UNSUPPORTED = -3 };

int vt_abi_version(void);
int vt_last_error(char* buf, size_t n);

/* row r of a logical [rows, dim] operand lives at physical row
 *   (r / grp) * stride + off + (r % grp)        (grp == 0: identity)
 * Used to read/write a slice "rows off..off+grp of every sequence of length stride" in place,
 * e.g. the last len(query) tokens that TransformerEncoderParallel keeps (transformer.py:69). */
typedef struct {
    int32_t grp;
    int64_t stride;
    int64_t off;
} vtRowMap;

/* ------------------------------------------------------------------------------------------
 * GEMM "NT": C[M,N] = A[M,K] . B[N,K]^T, bf16 operands, fp32 accumulate on MFMA.
 * Replaces nn.Linear / F.linear under autocast(bf16): timm Block's qkv/proj/fc1/fc2
 * (models/transformer.py:52-59), Bottleneck.in_linear/out_linear (models/bottleneck.py:109-110,
 * 142,163), OutputLayer.linear (models/larp_tokenizer.py:35,40) and the Conv3d of PatchEmbed3D
 * seen as a GEMM over gathered patches (models/embed.py:82,110), plus their input gradients.
 * K must be a multiple of 64; M and N are arbitrary (edge tiles are clamped on load, masked on
 * store).
 * ------------------------------------------------------------------------------------------ */
enum {
    VT_EPI_BF16 = 0,       /* out(bf16) = acc [+ bias]                                        */
    VT_EPI_BF16_GELU = 1,  /* out(bf16) = u = acc + bias ; out2(bf16) = gelu_erf(u)           */
    VT_EPI_F32 = 2,        /* out(f32)  = [round_bf16](acc [+ bias]) [+ residual] [+ rowmod]; */
                           /*             optional out2(bf16) copy; optional output row map   */
    VT_EPI_BF16_DGELU = 3, /* out(bf16) = acc * gelu_erf'(aux)      (aux = saved u, bf16)     */
    VT_EPI_BF16_GELU_GRAD = 4, /* with u = bf16(acc + bias): out(bf16) = gelu_erf'(u), out2(bf16) = gelu_erf(u), both from one
                                  evaluation; u itself is not written.  out2 is required and carries the bits VT_EPI_BF16_GELU
                                  writes.  The forward of a Linear + GELU whose backward is VT_EPI_BF16_MULAUX              */
    VT_EPI_BF16_MULAUX = 5 /* out(bf16) = bf16(acc [+ bias]) * aux   (aux bf16 [M,N], e.g. the saved gelu_erf'(u): the
                              VT_EPI_BF16_DGELU product with gelu' rounded to bf16 once, and no erf / exp per element)       */
};

typedef struct {
    const void* A; int64_t lda; /* bf16 [M,K] */
    const void* B; int64_t ldb; /* bf16 [N,K] */
    int32_t M, N, K;
    int32_t epi;
    void* out; int64_t ldo;
    void* out2; int64_t ldo2;
    const float* bias;                       /* [N] or NULL                                   */
    const float* residual; int64_t ldr;      /* f32, indexed like `out` (after the row map)   */
    const float* rowmod; int32_t rowmod_period; /* f32 [period,N] added at row (r % period)   */
    const void* aux; int64_t ldaux;          /* bf16 [M,N]                                    */
    vtRowMap omap;                           /* VT_EPI_F32 only                               */
    int32_t round_bf16;                      /* VT_EPI_F32 only                               */
    float* colsum_partial;                   /* VT_EPI_BF16_DGELU / VT_EPI_BF16_MULAUX only, optional: fp32 [ceil(M/192), N]; row t = column
                                                sums of the bf16-rounded output over rows [192 t, 192 t + 192) (fixed
                                                order, no atomics).  vt_sum_slabs over the rows gives the bias gradient
                                                of the Linear whose pre-activation (or its saved gelu') is `aux`, without re-reading `out` */
    float out_scale;                         /* VT_EPI_F32 only: 0 = none; otherwise the finished value (after bias, rounding, residual,
                                                rowmod) is multiplied by it -- the 1/sqrt(i+1) rescale of the residual stream after
                                                layer i of models/model_new/base/transformer.py:88-90 -- before out / out2 are written */
    int32_t tile;                            /* tile generation for THIS call: 0 = automatic (use this; 192x192x64 tiles on a
                                                3-stage LDS-DMA ring, one persistent workgroup per CU, when the problem fills
                                                them, else 128x128x64).  Tests / tuning: 1 = force 128 (2-deep ring), 16 = force 128
                                                (4-deep ring), 2 = force 192, 6 = 192x192 one tile per
                                                workgroup, 7 = the M <= 64 weight-streaming kernel, 19 = 192x192 walking its tiles as a
                                                row-major list, 19 + W (W = 1..12) = in column blocks of W tile columns (A/B timing of the
                                                order, same results).  Every other value is VT_ERR_INVALID: 3, 4, 8..15, 17 and 18 once
                                                selected timing experiments inside the 192x192 kernel (some with wrong results on purpose)
                                                and 5 a 192x96 instantiation that no dispatch rule picked; they are gone, and no caller
                                                passed them.  Results do not depend on the choice (same fp32
                                                summation order) unless K is split, below.  The library keeps no such setting between calls.
                                                Automatic tile order of both NT kernels (vt_auto_col_block): column blocks of the width
                                                nearest the square root of the tiles one XCD has in flight, the tile columns cut into
                                                near-equal blocks; the row-major list when one block would span the matrix.
                                                VT_GEMM_TILE_ORDER=W in the environment (read once per process) forces W, as 19 + W does
                                                per call, for every NT launch of either kernel: whole-step A/B timing */
    void* splitk_ws; int64_t splitk_ws_bytes; /* optional workspace of vt_gemm_nt_splitk_workspace_bytes() bytes, 256-byte aligned, ZERO when first
                                                handed over (its first 4 KiB are arrival counters the kernel returns to zero) and used by one stream
                                                at a time.  With it, a launch of the 128x128 kernel that would leave most CUs idle (the N = 768
                                                GEMMs of a one-clip training step: 72 tiles, K up to 3072) splits K over up to 8 workgroups per
                                                tile; the last to arrive adds the fp32 partial sums in split order and runs the epilogue:
                                                run-to-run bit-identical, but not the unsplit summation order.  NULL: never split */
    int32_t splitk;                          /* 0 = automatic (needs splitk_ws), 1 = never, 2..8 = this many (tests / tuning; tile 0, 1 or 16) */
} vtGemmNT;
size_t vt_gemm_nt_splitk_workspace_bytes(void);

int vt_gemm_nt(const vtGemmNT* p_host, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * GEMM "TN", grouped: for each problem g  C_g[P,Q] = A_g[M,P]^T . B_g[M,Q]  (fp32 out).
 * Weight gradients dW = dY^T X of every nn.Linear / the Conv3d above (what autograd derives
 * for F.linear); all problems of one launch share one grid so a transformer block's four
 * weight gradients fill the chip without split-K or atomics.  M % 64 == 0, P % 8 == 0,
 * Q % 8 == 0; rows >= p_lim and cols >= q_lim of C are not stored; row_perm (optional,
 * int32[p_lim]) scatters row p of C to row row_perm[p].  At most VT_TN_MAX_GROUP problems.
 * ------------------------------------------------------------------------------------------ */
#define VT_TN_MAX_GROUP 16
typedef struct {
    const void* A; int64_t lda; /* bf16 [M,P]  (dY) */
    const void* B; int64_t ldb; /* bf16 [M,Q]  (X)  */
    int32_t M, P, Q;
    float* out; int64_t ldo;
    int32_t p_lim, q_lim;
    const int32_t* row_perm;
    int32_t tile;               /* problem 0's value selects the tile generation of the launch: 0 = automatic, 1 = 128x128, 2 = 192x192,
                                   7 = 192x192 without the cross-K-tile register pipeline (round-1 kernel, A/B timing; same bits) */
} vtGemmTN;

int vt_gemm_tn_grouped(const vtGemmTN* problems_host, int32_t n_problems, vtStream stream);



/* ------------------------------------------------------------------------------------------
 * LayerNorm (fp32 in, fp32 statistics, bf16 out for the next MFMA GEMM).
 * Replaces nn.LayerNorm inside timm Block (norm1/norm2, eps 1e-5; models/transformer.py:52-59)
 * and OutputLayer.norm_final (eps 1e-6; models/larp_tokenizer.py:34,39), forward and backward.
 * dim in {256,512,768,1024}.  Row r of x/dres/dx/dx_bf16 is at physical row xmap(r); y, dy, mean,
 * rstd are indexed by r.  Backward also adds the residual-stream gradient `dres` (may be NULL)
 * and emits column sums: dgamma, dbeta and (optional) dxsum = sum_r dx[r,:] (the bias gradient
 * of the Linear that produced this residual stream).
 * ------------------------------------------------------------------------------------------ */
int vt_layernorm_fwd(const float* x, vtRowMap xmap, const float* gamma, const float* beta, float eps, int64_t rows,
                     int32_t dim, void* y_bf16, float* mean, float* rstd, vtStream stream);
size_t vt_layernorm_bwd_workspace_bytes(int32_t dim);
int vt_layernorm_bwd(const void* dy_bf16, const float* x, vtRowMap xmap, const float* gamma, const float* mean,
                     const float* rstd, const float* dres, int64_t rows, int32_t dim, float* dx, void* dx_bf16,
                     float* dgamma, float* dbeta, float* dxsum, void* workspace, vtStream stream);

/* column sums out[c] = sum_r src[map(r), c] (bias gradients of nn.Linear); src bf16 or fp32 */
size_t vt_colsum_workspace_bytes(int32_t width);
int vt_colsum(const void* src, int32_t src_is_bf16, int64_t ld, vtRowMap map, int64_t rows, int32_t width, float* out,
              void* workspace, vtStream stream);
/* out[j,:] = sum_b src[map(b*n + j), :]  -- gradient of encoder_latent_query_embed, which
 * larp_tokenizer.py:410 broadcasts over the batch with .repeat(b,1,1) */
int vt_batch_sum(const float* src, vtRowMap map, int32_t batch, int32_t n, int32_t dim, float* out, vtStream stream);
/* zero rows map(r), r < rows, of an fp32 matrix and/or its bf16 twin (rows a sliced backward does not write) */
int vt_zero_rows(float* a, void* b_bf16, vtRowMap map, int64_t rows, int32_t dim, vtStream stream);
/* out[c] = sum_s slabs[s*slab_stride + c], fixed order (combine split-M partial weight gradients) */
int vt_sum_slabs(const float* slabs, int32_t nslab, int64_t slab_stride, int32_t width, float* out, vtStream stream);
/* dst[r,:] = bf16(src[map(r),:]) */
int vt_cast_rows(const float* src, vtRowMap map, int64_t rows, int32_t dim, void* dst_bf16, int64_t ldd, vtStream stream);
/* dst[b*seq + off + j, :] = src[b*n + j, :] + table[j, :] + vec[:]   (each term optional)
 * sequence assembly: torch.cat([context, query]) of transformer.py:64 without a copy kernel per
 * operand, `z + decoder_latent_pe` (larp_tokenizer.py:463-464) and the query-embed broadcasts
 * (:410, :465). */
int vt_assemble_rows(float* dst, int64_t seq, int64_t off, int32_t batch, int32_t n, int32_t dim, const float* src,
                     const float* table, const float* vec, vtStream stream);
/* fp32 master weight W[N,K] -> bf16 W[N,ldd] and/or bf16 W^T[K,lddT]; packed row r = W[row_perm[r]] */
int vt_pack_weight(const float* w, int32_t N, int32_t K, const int32_t* row_perm, void* wb, int64_t ldd, void* wt,
                   int64_t lddT, vtStream stream);
/* the same for many weights at once (after an optimizer step every bf16 operand copy is refreshed); jobs is a host array */
#define VT_PACK_MAX_GROUP 32
typedef struct {
    const float* w; int32_t N, K; const int32_t* row_perm;
    void* wb; int64_t ldd; void* wt; int64_t lddT;
} vtPackJob;
int vt_pack_weights_grouped(const vtPackJob* jobs_host, int32_t n_jobs, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * (T,H,W) patchify / unpatchify.  Patch-row columns are in (c,dt,dy,dx) order == Conv3d weight
 * flattening (models/embed.py:82,110-112); unpatchify is the inverse and, with the head weight
 * rows permuted at pack time, replaces LARPTokenizer.unpatchify's einops permute + .contiguous()
 * (models/larp_tokenizer.py:441-454,493).  p % 8 == 0.  The one-segment case of the kernel of csrc/vt_patch.hip (the lane layout, the
 * patch map and the rounding are csrc/vt_patch_map.h, shared with the _dual and _clips entry points), validated like vt_patchify_dual
 * below: VT_ERR_INVALID for a null or misaligned pointer, a size <= 0, T % pt, S % p, p % 8; S and p are reported as H = W and ph = pw.
 * ------------------------------------------------------------------------------------------ */
int vt_patchify(const float* video, int32_t B, int32_t C, int32_t T, int32_t S, int32_t pt, int32_t p, void* rows_bf16,
                vtStream stream);
int vt_unpatchify(const float* rows, int32_t B, int32_t C, int32_t T, int32_t S, int32_t pt, int32_t p, float* video,
                  vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Two-segment patchify / unpatchify (csrc/vt_patch.hip): the ends of `autoencoder_dualpatch`.  Its encoder cuts the clip along time,
 * x[:, :, :pt_first] into Conv3d(kernel = stride = (pt_first, ph, pw)) and x[:, :, pt_first:] into Conv3d((pt_rest, ph, pw))
 * (models/model_dualpatch/base/blocks.py:99-112); its decoder ends in two ConvTranspose3d whose outputs are concatenated along T
 * (blocks.py:252-257).  video fp32 [B, C, T, H, W] contiguous; frames [0, T0) <-> rows0 [B (T0/pt0)(H/ph)(W/pw), C pt0 ph pw], frames
 * [T0, T) <-> rows1 [B ((T-T0)/pt1)(H/ph)(W/pw), C pt1 ph pw]; token order (t, h, w) t-major per clip and column order (c, dt, dy, dx) as
 * vt_patchify, and the same rounding to bf16.  vt_unpatchify_dual reads two fp32 row matrices and writes every element of video exactly
 * once.  One launch each: no slice copy of the video, no torch.cat of the output.  H != W and ph != pw are fine.  Checked on the host
 * before anything is launched (VT_ERR_INVALID, vt_last_error names the entry point and the offending value): pointers non-null and
 * 16-byte aligned, every size > 0, 0 < T0 < T, T0 % pt0 == 0, (T - T0) % pt1 == 0, H % ph == 0, W % pw == 0, pw % 8 == 0.
 * ------------------------------------------------------------------------------------------ */
int vt_patchify_dual(const float* video, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0, int32_t pt0, int32_t pt1,
                     int32_t ph, int32_t pw, void* rows0_bf16, void* rows1_bf16, vtStream stream);
int vt_unpatchify_dual(const float* rows0, const float* rows1, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t T0, int32_t pt0,
                       int32_t pt1, int32_t ph, int32_t pw, float* video, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * The 3D ResNet ends of `autoencoder_cnnvit` (models/model_cnnvit/base/cnnvit.py): 3x3x3 convolution with padding 1, GroupNorm with an
 * optional swish, nearest-neighbour upsampling, and the video layout pair.  Activations are bf16 channels-last [B, T, H, W, C] (the memory
 * of a torch [B, C, T, H, W] tensor in channels_last_3d); channel counts are multiples of 16 up to 1024 (the 3-channel video ends are
 * zero-padded to 16 by the layout pair and the weight pack).  Strides (st, sh, sw) are (1,1,1), (1,2,2) or (2,2,2); T, H, W are always the
 * extents of the convolution's INPUT, its output has ((n - 1) / s + 1) per axis.  Everything is checked on the host before any launch
 * (VT_ERR_INVALID, vt_last_error names the entry point and the value); no atomics; every sum has a fixed order, so a second call gives the
 * same bits.
 *
 * vt_conv3d_pack_weight: the fp32 parameter [Cout, Cin, 3, 3, 3] -> the bf16 operand image of the forward (for_dgrad 0) or of the input
 *   gradient (for_dgrad 1: transposed, taps mirrored), vt_conv3d_packed_elems(n_abi, k_abi) bf16 elements (n, k = cout_abi, cin_abi forward and
 *   cin_abi, cout_abi for dgrad); rows / columns past Cout / Cin are zero.
 * vt_conv3d_fwd: out = bf16(acc + bias); with `residual` (same shape as out, may be null) out = bf16(float(bf16(acc + bias)) + float(res)).
 * vt_conv3d_dgrad: dx bf16 [B, T, H, W, Cin] from dy bf16 [B, T', H', W', Cout], fp32 sum.
 * vt_conv3d_wgrad: dw fp32 [cout_lim, cin_lim, 3, 3, 3] (the leading part of the channel ranges: the parameter's own extents at a padded
 *   end), summed over all B T' H' W' output positions; `workspace` holds vt_conv3d_wgrad_workspace_bytes(...) of fp32 partials.
 * ------------------------------------------------------------------------------------------ */
size_t vt_conv3d_packed_elems(int32_t n_abi, int32_t k_abi);
int vt_conv3d_pack_weight(const float* w, int32_t Cout, int32_t Cin, int32_t cout_abi, int32_t cin_abi, int32_t for_dgrad, void* packed_bf16,
                          vtStream stream);
int vt_conv3d_fwd(const void* x_bf16, const void* w_packed, const float* bias, const void* residual_bf16, int32_t B, int32_t T, int32_t H, int32_t W,
                  int32_t Cin, int32_t Cout, int32_t st, int32_t sh, int32_t sw, void* out_bf16, vtStream stream);
int vt_conv3d_dgrad(const void* dy_bf16, const void* w_packed_dgrad, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t st,
                    int32_t sh, int32_t sw, void* dx_bf16, vtStream stream);
size_t vt_conv3d_wgrad_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t st, int32_t sh, int32_t sw,
                                       int32_t cout_lim, int32_t cin_lim);
int vt_conv3d_wgrad(const void* x_bf16, const void* dy_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t st, int32_t sh,
                    int32_t sw, int32_t cout_lim, int32_t cin_lim, float* dw, void* workspace, vtStream stream);
/* GroupNorm(G, C, eps) over (C/G channels x P positions) of each clip of x bf16 [B, P, C]; swish 1: z = y sigmoid(y).  Statistics in fp32 from
 * the bf16 input, variance as the mean of squared deviations from the mean; y rounded to bf16 once; mean / rstd fp32 [B, G].  The backward
 * takes the forward's input, mean and rstd and gives dx bf16 and dgamma / dbeta fp32 [C].  One workspace size serves both. */
size_t vt_groupnorm_workspace_bytes(int32_t B, int64_t P, int32_t C, int32_t G);
int vt_groupnorm_fwd(const void* x_bf16, const float* gamma, const float* beta, float eps, int32_t B, int64_t P, int32_t C, int32_t G, int32_t swish,
                     void* y_bf16, float* mean, float* rstd, void* workspace, vtStream stream);
int vt_groupnorm_bwd(const void* dz_bf16, const void* x_bf16, const float* gamma, const float* beta, const float* mean, const float* rstd, int32_t B,
                     int64_t P, int32_t C, int32_t G, int32_t swish, void* dx_bf16, float* dgamma, float* dbeta, void* workspace, vtStream stream);
/* nearest-neighbour upsampling by (ft, fh, fw) = (2,2,2) or (1,2,2), src = dst / f; T, H, W are the SOURCE extents.  The backward adds the 4 or 8
 * children of a source position in fp32, in (t, h, w) order, and rounds once. */
int vt_upsample_nearest_fwd(const void* x_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t ft, int32_t fh, int32_t fw, void* out_bf16,
                            vtStream stream);
int vt_upsample_nearest_bwd(const void* dout_bf16, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t ft, int32_t fh, int32_t fw, void* dx_bf16,
                            vtStream stream);
/* fp32 video [B, C, T, H, W] -> bf16 channels-last [B, T, H, W, Cpad] with channels C .. Cpad - 1 zero, and back (fp32 holding the bf16 values;
 * the pad channels are not read) */
int vt_video_to_channels_last(const float* video, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t Cpad, void* out_bf16, vtStream stream);
int vt_channels_last_to_video(const void* x_bf16, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t Cpad, float* video, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention, head_dim 64, no mask (timm Attention -> F.scaled_dot_product_attention inside
 * timm Block, models/transformer.py:52-59).  qkv bf16 [B,L,3,H,64]; o/dO bf16 [B,L,H,64];
 * lse2 fp32 [B,H,L] (log2-domain LSE of the scaled scores, saved for backward);
 * delta_ws fp32 [B,H,L] scratch.  Any L >= 1 (tail rows/keys are masked).  qkv, o, dO and dqkv 16-byte aligned (every
 * operand is read and every output written 16 bytes per lane; a misaligned pointer returns VT_ERR_INVALID).
 * ------------------------------------------------------------------------------------------ */
int vt_attention_fwd(const void* qkv, int32_t B, int32_t L, int32_t H, int32_t hd, void* o, float* lse2, vtStream stream);
int vt_attention_bwd(const void* qkv, const void* o, const void* dO, const float* lse2, int32_t B, int32_t L, int32_t H,
                     int32_t hd, void* dqkv, float* delta_ws, vtStream stream);
/* causal variant (head_dim 64): query q attends keys 0..q -- F.scaled_dot_product_attention(..., is_causal=True) inside the AR
 * consumer's Attention (models/larp_ar.py:186-190) and its autograd.  Same layouts as above. */
int vt_attention_causal_fwd(const void* qkv, int32_t B, int32_t L, int32_t H, void* o, float* lse2, vtStream stream);
int vt_attention_causal_bwd(const void* qkv, const void* o, const void* dO, const float* lse2, int32_t B, int32_t L, int32_t H, void* dqkv,
                            float* delta_ws, vtStream stream);
/* The same for the queries q_begin .. L-1 only (q_begin a multiple of 64): `transformer_encoder_parallel` returns
 * h[:, -len(query):] (models/transformer.py:69), so in the LAST block of a stack the other rows' attention outputs are
 * never read and their output gradients are zero.  o / dO are compact [B, L - q_begin, H, hd]; keys/values, lse2,
 * delta_ws and dqkv keep the full length (dQ rows before q_begin are written as zeros, dK/dV get the kept queries'
 * contributions). */
int vt_attention_fwd_rows(const void* qkv, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t q_begin, void* o_compact, float* lse2,
                          vtStream stream);
int vt_attention_bwd_rows(const void* qkv, const void* o_compact, const void* dO_compact, const float* lse2, int32_t B, int32_t L,
                          int32_t H, int32_t hd, int32_t q_begin, void* dqkv, float* delta_ws, vtStream stream);
/* Cross attention: the queries come from one tensor, the keys and values from another (CrossAttention of
 * models/model_design/base/transformer.py:92-141, `flash_attn_func(q, k, v)` with 2048 queries and 256 first-frame keys).  All
 * operands bf16.  Row r of batch b of q starts at q + (b * Lq + r) * q_rs, head h at columns 64h .. 64h+63 of the row; k and v
 * likewise with Lk rows per batch and strides of their own (two pointers: k may be a normalised copy while v is read in place from
 * the to_kv output).  o / dO compact [B, Lq, H, 64]; lse2, delta_ws fp32 [B, H, Lq].  dq covers B * Lq rows, dk and dv B * Lk
 * rows; columns 0 .. 64H-1 of every row are written, the rest of a wider buffer is not touched.  Scale 64^-0.5, no mask, any
 * Lq >= 1 and Lk >= 1.  hd must be 64, every stride >= 64H, below 2^24 and a multiple of 8 elements, every pointer 16-byte aligned
 * (VT_ERR_INVALID + vt_last_error otherwise).  The kernels and tile code of vt_attention_*: with q = qkv, k = qkv + 64H,
 * v = qkv + 128H, every stride 192H and Lq = Lk the results are bit-identical to vt_attention_fwd / _bwd. */
int vt_attention_cross_fwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, int32_t B, int32_t Lq,
                           int32_t Lk, int32_t H, int32_t hd, void* o, float* lse2, vtStream stream);
int vt_attention_cross_bwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, const void* o,
                           const void* dO, const float* lse2, int32_t B, int32_t Lq, int32_t Lk, int32_t H, int32_t hd, void* dq,
                           int64_t dq_rs, void* dk, int64_t dk_rs, void* dv, int64_t dv_rs, float* delta_ws, vtStream stream);

/* Packed variable-length attention with grouped KV heads (the Attn layer of models/model_titok/base/transformer.py:32-62, which calls
 * flash_attn_varlen_func): n_seq sequences lie one behind the other in the M = cu_seqlens[n_seq] rows of every operand, sequence b is
 * rows cu_seqlens[b] .. cu_seqlens[b+1]-1 and attends only inside itself.  q is a view [M, 64 Hq], k and v views [M, 64 Hkv] of bf16
 * buffers with row strides q_rs / k_rs / v_rs (the three column blocks of one [M, 64 (Hq + 2 Hkv)] projection are the main caller);
 * Hq % Hkv == 0 and query head h reads KV head h / (Hq / Hkv) (repeat_interleave, flash-attn's convention).  o / dO bf16 dense
 * [M, 64 Hq]; lse2 and delta_ws fp32 [Hq, M]; dq [M, 64 Hq], dk and dv [M, 64 Hkv] with their own row strides.  Scale 64^-0.5, no mask.
 * cu_seqlens_host is a HOST array of n_seq + 1 entries, read before the call returns: it is validated here (cu[0] == 0, strictly
 * increasing -- an empty sequence is refused --, cu[n_seq] == M, 1 <= n_seq <= VT_VARLEN_MAX_SEQ) and travels to the kernels by value
 * in their arguments, so no kernel reads a boundary from device memory and the launch can be captured in a graph.  Strides and
 * alignment as for vt_attention_cross_* (VT_ERR_INVALID + vt_last_error otherwise).  The grid is exactly sum_b ceil(L_b / 128) workgroups
 * per head.  dK/dV sums the query heads of a group in ascending order inside one workgroup: no atomics, the same bits on every run.  The
 * kernels and tile code of vt_attention_cross_*: with one sequence and Hq == Hkv the results are bit-identical to B = 1, Lq = Lk = M. */
#define VT_VARLEN_MAX_SEQ 64
int vt_attention_varlen_fwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs,
                            const int32_t* cu_seqlens_host, int32_t n_seq, int32_t M, int32_t Hq, int32_t Hkv, int32_t hd, void* o, float* lse2,
                            vtStream stream);
int vt_attention_varlen_bwd(const void* q, int64_t q_rs, const void* k, int64_t k_rs, const void* v, int64_t v_rs, const void* o,
                            const void* dO, const float* lse2, const int32_t* cu_seqlens_host, int32_t n_seq, int32_t M, int32_t Hq,
                            int32_t Hkv, int32_t hd, void* dq, int64_t dq_rs, void* dk, int64_t dk_rs, void* dv, int64_t dv_rs, float* delta_ws,
                            vtStream stream);

/* Data movement of the packed `titok` model (models/model_titok/base/blocks.py:82-222; csrc/vt_packed.hip).  Every table is a HOST array,
 * read and validated before the call returns, and travels to the kernel by value in its arguments (as cu_seqlens_host above): at most
 * VT_VARLEN_MAX_SEQ entries, no kernel reads a boundary or a pointer table from device memory, the launches can be captured in a graph.
 * No atomics: every result has the same bits on every run.  A violation returns VT_ERR_INVALID, vt_last_error names the entry point and
 * the offending value, and nothing is launched.
 *
 * vt_patchify_clips: n clips, clip b its own contiguous fp32 [C, T_b, H_b, W_b] at the 16-byte aligned device pointer clips_host[b].data,
 * -> bf16 patch rows [sum_b G_b, Kp], G_b = (T_b/pt)(H_b/p)(W_b/p), Kp = C*pt*p*p; column order (c, dt, dy, dx) and token order (t, h, w)
 * as vt_patchify; clip b starts at row sum_{a<b} G_a; one launch.  H_b != W_b is fine; p % 8 == 0, T_b % pt == 0, H_b % p == 0 and
 * W_b % p == 0 are required, and `rows` must be sum_b G_b (the row count the caller allocated).
 * vt_unpatchify_clips: the inverse on fp32 rows [sum_b G_b, Kp], written into the n clips. */
typedef struct {
    void* data;        /* device pointer, fp32 [C, T, H, W] contiguous, 16-byte aligned */
    int32_t T, H, W;
} vtClip;
int vt_patchify_clips(const vtClip* clips_host, int32_t n, int32_t C, int32_t pt, int32_t p, void* rows_bf16, int64_t rows, vtStream stream);
int vt_unpatchify_clips(const float* rows_f32, int64_t rows, const vtClip* clips_host, int32_t n, int32_t C, int32_t pt, int32_t p,
                        vtStream stream);
/* A packed fp32 [M, D] in which sequence b is rows cu[b] .. cu[b+1]-1 and splits after its first lead[b] rows into a lead and a tail
 * segment (the encoder's [latent tokens | patch rows], the decoder's [codes | mask tokens]).  `which` chooses one of the two.
 * cu[0] == 0, strictly increasing, cu[n_seq] == M; 1 <= lead[b] < cu[b+1] - cu[b] (both segments non-empty); 1 <= n_seq <=
 * VT_VARLEN_MAX_SEQ; D % 4 == 0; every pointer 16-byte aligned.
 * vt_packed_scatter: every row of dst [M, D] is written: the chosen segments take, in order, the rows of the compact src
 * [sum_b |segment_b|, D]; the rows of the other segments take vec[D], or zeros when vec is NULL.
 * vt_packed_gather: out compact [sum_b |segment_b|, D] = the chosen segments' rows of packed, in order.
 * vt_packed_segment_colsum: out[D] = the sum over every row of the chosen segments, in a fixed order (slabs of consecutive rows, then
 * the slabs in order), read in place; workspace: vt_packed_segment_colsum_workspace_bytes(D) bytes. */
enum { VT_PACKED_LEAD = 0, VT_PACKED_TAIL = 1 };
int vt_packed_scatter(const float* src, const float* vec, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq, int32_t M,
                      int32_t D, int32_t which, float* dst, vtStream stream);
int vt_packed_gather(const float* packed, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq, int32_t M, int32_t D,
                     int32_t which, float* out, vtStream stream);
size_t vt_packed_segment_colsum_workspace_bytes(int32_t D);
int vt_packed_segment_colsum(const float* packed, const int32_t* cu_seqlens_host, const int32_t* lead_host, int32_t n_seq, int32_t M, int32_t D,
                             int32_t which, float* out, void* workspace, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Vector quantisation (SimpleVectorQuantizer.forward, models/bottleneck.py:262-324).
 *   mode 0: stochastic=False  argmin(|z|^2+|e|^2-2z.e)           (:282-290)
 *   mode 1: eval-deterministic argmax(softmax(z.e/tau))           (:275-278)
 *   mode 2: training default   multinomial(softmax(z.e/tau))      (:280)  via Gumbel-max, counter RNG
 * z_in fp32 [N,ldz]; codebook fp32 [K,d] (nn.Embedding weight); d in {8,16,24,32}.
 * Outputs (all caller-owned, saved for backward): E [K,d] = normalised codebook ('emb'), wnorm [K],
 * zn [N,d] ('unregularized_z'), znorm [N], idx int64 [N] ('bottleneck_rep'), rz fp32 [N,d]
 * ('regularized_z' = z + (q - z)), optional rz_pad bf16 [N,ldp] (cols >= d untouched),
 * losses[4] = {loss_q, loss_commit, loss_codebook, mse}.  Index arithmetic is bit-exact against
 * oracle/vq_oracle.c (sequential fp32 FMA chain; lowest index wins ties).
 * Backward: gscal = device {dL/dloss_q, dL/dloss_commit, dL/dloss_codebook} (may be NULL);
 * g_rz = dL/dregularized_z fp32 [N,ldg] (may be NULL); outputs dz_in (fp32 [N,d] and/or bf16
 * [N,ldp]) and the dense codebook gradient dW [K,d] (deterministic, no atomics: one-hot product on the exact
 * fp32 MFMA, cost independent of how the tokens spread over the codes); dW == NULL skips it (frozen codebook: the 'sq'
 * quantizer `VectorQuantizer` of models/model_new/quantizer/fsq.py:144-230, K = 196 560, which is vt_vq_forward mode 1 with
 * inv_tau = 1 and loss = d * loss_q).  `workspace`: vt_vq_workspace_bytes(N,K,d) bytes, the forward's scratch may be reused.
 * N, K >= 1; every row stride given with a non-NULL buffer (ldp, ldg) is >= d.  Checked on the host: VT_ERR_INVALID + vt_last_error,
 * nothing is launched.
 * ------------------------------------------------------------------------------------------ */
size_t vt_vq_workspace_bytes(int32_t N, int32_t K, int32_t d);
int vt_vq_forward(const float* z_in, int64_t ldz, const float* codebook, int32_t N, int32_t K, int32_t d, int32_t mode,
                  int32_t l2_normalized, float inv_tau, float beta, float codebook_w, uint64_t seed, float* E, float* wnorm,
                  float* zn, float* znorm, int64_t* idx, float* rz, void* rz_pad_bf16, int64_t ldp, float* losses,
                  void* workspace, vtStream stream);
/* the same with a per-call counter that lives in DEVICE memory (mode 2 only; may be NULL): the sampling noise is hashed from
 * seed + *seed_counter, so a captured launch draws fresh noise on every replay once the caller increments the counter in the graph */
int vt_vq_forward_ctr(const float* z_in, int64_t ldz, const float* codebook, int32_t N, int32_t K, int32_t d, int32_t mode,
                      int32_t l2_normalized, float inv_tau, float beta, float codebook_w, uint64_t seed, const uint32_t* seed_counter,
                      float* E, float* wnorm, float* zn, float* znorm, int64_t* idx, float* rz, void* rz_pad_bf16, int64_t ldp,
                      float* losses, void* workspace, vtStream stream);
int vt_vq_backward(const float* g_rz, int64_t ldg, const float* gscal, float beta, float codebook_w, const float* zn,
                   const float* znorm, const float* E, const float* wnorm, const int64_t* idx, int32_t N, int32_t K,
                   int32_t d, int32_t l2_normalized, float* dz_in, void* dz_pad_bf16, int64_t ldp, float* dW,
                   void* workspace, vtStream stream);
/* get_codebook_entry (bottleneck.py:327-344): E = normalise(codebook) then out[n,:] = E[idx[n],:] */
int vt_vq_prep_codebook(const float* codebook, int32_t K, int32_t d, int32_t l2_normalized, float* E, float* wnorm,
                        void* workspace, vtStream stream);
int vt_vq_gather(const float* E, const int64_t* idx, int32_t N, int32_t K, int32_t d, float* out, void* out_pad_bf16,
                 int64_t ldp, vtStream stream);


/* ------------------------------------------------------------------------------------------
 * Finite scalar quantizer: FSQ.forward / quantize / codes_to_indices / indices_to_codes of the reference's
 * TiTok-style autoencoders (models/model_new/quantizer/fsq.py:76-131; levels [8,8,8,5,5,5] or [8,8,8,8,5,5,5,5],
 * models/model_new/autoencoder.py:59,140,640).  z, codes, dcodes, dz are [N, d] row-major, fp32 (is_bf16 = 0) or
 * bf16 (is_bf16 = 1: the reference up-casts to fp32, computes, and casts codes back, :122-129); indices int32 [N]
 * (may be NULL in forward).  `levels_host`: d ints on the HOST, each >= 2, prod <= 2^24, d <= 16.
 * Backward is the straight-through estimator autograd derives: dz = dcodes / (levels // 2) * half_l * (1 - tanh^2).
 * One launch each; indices and codes are bit-exact against the reference's fp32 arithmetic.
 * ------------------------------------------------------------------------------------------ */
int vt_fsq_codebook_size(const int32_t* levels_host, int32_t d, int64_t* size);
int vt_fsq_forward(const void* z, int32_t is_bf16, int64_t N, int32_t d, const int32_t* levels_host, void* codes,
                   int32_t* indices, vtStream stream);
int vt_fsq_backward(const void* z, const void* dcodes, int32_t is_bf16, int64_t N, int32_t d, const int32_t* levels_host,
                    void* dz, vtStream stream);
int vt_fsq_indices_to_codes(const int32_t* indices, int64_t N, int32_t d, const int32_t* levels_host, void* codes,
                            int32_t is_bf16, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Token gate of `autoencoder_stat` (models/model_stat/autoencoder.py:69-138, base/blocks.py:11-24,89): the adaptive-length
 * tokenizer scores each latent row with ProbPredictor = Linear(W, W) -> GELU -> Linear(W, 1) -> Sigmoid and zeroes the rows it
 * drops before FSQ.  The first Linear + GELU is vt_gemm_nt (VT_EPI_BF16_GELU: u and g = gelu(u), bf16 [M, W] with row stride ld);
 * these two calls are the rest.  W % 128 == 0, W <= 1024; g, u, dU, w2 16-byte aligned; probs, mask fp32 [M]; z, codes, dz,
 * dcodes fp32 [M, d]; indices int32 [M] (may be NULL); w2 fp32 [W], b2 / db2 fp32 [1] (device).
 *   forward:  p = bf16(sigmoid(bf16(g . w2 + b2))); mask by `mode`; codes, indices = FSQ(z * mask) exactly as vt_fsq_forward.
 *             VT_STAT_SAMPLE keeps row m iff u_m < p with u_m a counter-hash uniform of (seed, m); VT_STAT_THRESHOLD iff p > 0.5;
 *             VT_STAT_ONES keeps every row; VT_STAT_FORCED copies mask_in.  z == NULL: probabilities and mask only.
 *   backward: dz = fsq'(z * mask) dcodes * mask; dp = [ste](sum_c (fsq'(z * mask) dcodes)_c z_c + dmask) + dprobs (dprobs / dmask
 *             may be NULL); dlogit = dp p (1 - p); dU = bf16(dlogit w2 * gelu'(u)); dw2 = sum_m dlogit_m g_m, db2 = sum_m dlogit_m
 *             (per-workgroup partials in `workspace` of vt_stat_gate_workspace_bytes(W) bytes, summed in a fixed order: no atomics,
 *             bit-identical run to run).  `ste` = the mask is the straight-through `(mask - p).detach() + p` (sampled or forced).
 * ------------------------------------------------------------------------------------------ */
enum { VT_STAT_SAMPLE = 0, VT_STAT_THRESHOLD = 1, VT_STAT_ONES = 2, VT_STAT_FORCED = 3 };
size_t vt_stat_gate_workspace_bytes(int32_t W);
int vt_stat_gate_forward(const void* g, int64_t ldg, const float* w2, const float* b2, const float* z, int64_t M, int32_t W, int32_t d,
                         const int32_t* levels_host, int32_t mode, uint64_t seed, const float* mask_in, float* probs, float* mask,
                         float* codes, int32_t* indices, vtStream stream);
int vt_stat_gate_backward(const float* dcodes, const float* dprobs, const float* dmask, const float* z, const float* mask,
                          const float* probs, const void* u, const void* g, int64_t ld, const float* w2, int64_t M, int32_t W, int32_t d,
                          const int32_t* levels_host, int32_t ste, void* dU, float* dz, float* dw2, float* db2, void* workspace,
                          vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Diagonal-Gaussian KL bottleneck: the 'skl' regularizer (`SummedKLDivergenceRegularizer` over
 * `DiagonalGaussianDistribution`, models/bottleneck.py:36-64, 347-375) between in_linear and out_linear.
 * z fp32 [M, ldz] holds 2d interleaved columns: mean = z[:, 0::2], logvar = clamp(z[:, 1::2], -30, 20) (bounds inclusive).
 *   forward:  eps = standard normal from a counter hash of (seed, *seed_counter, element index r * d + c) (Box-Muller on element
 *             pairs; seed_counter is device memory and may be NULL, the low seed word plus *seed_counter as in vt_vq_forward_ctr, so
 *             a replayed hipGraph draws fresh noise and eager / replayed calls draw the same sequence); sample = mean + exp(logvar/2) eps
 *             (the reference always samples, in eval mode too).  Writes mean, sample, noise fp32 [M, d] (each may be NULL), the bf16
 *             copy of sample with row stride ldp, columns d..ldp zeroed (may be NULL), and loss_kl[0] = sum_{r,c} 0.5 (mean^2 +
 *             exp(logvar) - 1 - logvar) / batch (the per-sample sum averaged over `batch` = M / rows per sample).  The sum runs over
 *             per-workgroup partials in `workspace` (VT_KL_WORKSPACE_BYTES) in a fixed order: no float atomics, bit-identical run to run.
 *   backward: g_sample = dL/dsample [M, ldg] (may be NULL), g_mean = dL/dmean [M, d] (may be NULL), gkl = device {dL/dloss_kl}
 *             (may be NULL); dmean = g_sample + g_mean + (gkl / batch) mean, dlogvar_raw = [-30 <= z_odd <= 20] (g_sample eps std / 2
 *             + (gkl / batch) (var - 1) / 2) -> dz fp32 [M, 2d] interleaved and / or its bf16 copy with row stride ldp >= 2d, columns
 *             2d..ldp zeroed (either may be NULL, not both).
 * d % 4 == 0 (8, 16, 24, 32 on the engine), M % batch == 0; z, mean, sample, noise, dz 16-byte aligned, ldz % 4 == 0; bf16 outputs,
 * g_sample and g_mean 8-byte aligned, ldp % 4 == 0, ldg % 2 == 0.  Checked on the host: VT_ERR_INVALID + vt_last_error.
 * ------------------------------------------------------------------------------------------ */
#define VT_KL_WORKSPACE_BYTES 4096
int vt_kl_forward(const float* z, int64_t ldz, int64_t M, int32_t d, int32_t batch, uint64_t seed, const uint32_t* seed_counter,
                  float* mean, float* sample, void* sample_pad_bf16, int64_t ldp, float* noise, float* loss_kl, void* workspace,
                  vtStream stream);
int vt_kl_backward(const float* g_sample, int64_t ldg, const float* g_mean, const float* gkl, const float* z, int64_t ldz,
                   const float* noise, int64_t M, int32_t d, int32_t batch, float* dz, void* dz_pad_bf16, int64_t ldp, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Glue of the TiTok-style transformer block (models/model_new/base/transformer.py:11-63, rope.py:18-24): the block's
 * GEMMs, its LayerNorm over D and the attention itself are vt_gemm_nt / vt_layernorm_* / vt_attention_*; these are the
 * HBM-bound passes in between.  All matrices bf16 row-major, 16-byte aligned; head_dim is 64 (utils.py:6), D = 64 H.
 *   qkvg [M, 4D]  = to_qkv(x), columns q | k | v | gate (chunk(4), :46), M = B * L rows, row r has position r % L.
 *   vt_qknorm_rope_fwd: q, k <- rotary(LayerNorm_64(q or k; eps, affine q_w/q_b, k_w/k_b)) (:52-56), v copied; writes
 *     the packed [M, 3D] operand of vt_attention_fwd.  cos/sin: fp32 [L, 32] = real/imag of freqs_cis (rope.py:27-46,
 *     95-112), pair j of a head rotates (x[2j], x[2j+1]).
 *   vt_qknorm_rope_bwd: dqkv [M, 3D] (from vt_attention_bwd) -> columns 0..3D of dqkvg [M, 4D]; parameter gradients
 *     dq_w, dq_b, dk_w, dk_b fp32 [64] each (any may be NULL); workspace of vt_qknorm_rope_bwd_workspace_bytes().
 *   vt_sigmoid_gate_fwd: og [M, D] = o * sigmoid(gate) (:61), gate read in place from columns 3D..4D of qkvg.
 *   vt_sigmoid_gate_bwd: dog -> d_o [M, D] and columns 3D..4D of dqkvg.
 *   vt_geglu_fwd: a[:, :I] = gelu_erf(h[:, I:2I]) * h[:, :I]  (GEGLU, :11-17), h [M, 2I], a has row stride lda >= I
 *     (pad columns are not written: zero them once if lda is the 64-padded contraction dim of the next GEMM).
 *   vt_geglu_bwd: da -> dh [M, 2I].
 * Rounding follows autocast(bf16): every tensor the reference materialises in bf16 is rounded at the same point.
 * ------------------------------------------------------------------------------------------ */
int vt_qknorm_rope_fwd(const void* qkvg, int64_t M, int32_t L, int32_t H, const float* q_w, const float* q_b, const float* k_w,
                       const float* k_b, float eps, const float* cos_tab, const float* sin_tab, void* qkv_out, vtStream stream);
size_t vt_qknorm_rope_bwd_workspace_bytes(void);
int vt_qknorm_rope_bwd(const void* qkvg, const void* dqkv, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w,
                       float eps, const float* cos_tab, const float* sin_tab, void* dqkvg, float* dq_w, float* dq_b, float* dk_w,
                       float* dk_b, void* workspace, vtStream stream);
/* The grouped-projection twin of vt_qknorm_rope_* for the packed variable-length layer (Attn of models/model_titok/base/transformer.py:32-62;
 * csrc/vt_varlen.hip).  qkv bf16 [M, 64 (Hq + 2 Hkv)] (row stride in_rs), columns q | k | v = to_qkv(x) of a packed batch of M rows;
 * qkv_out the same layout (row stride out_rs): every q head gets LayerNorm_64 with q_w / q_b, every k head with k_w / k_b, both are then
 * rotated, v is copied.  Row m uses table row m: cos_tab / sin_tab are fp32 [M, 32], there is no period.  The backward takes the gradient
 * of qkv_out (dqkv_out, row stride g_rs, what vt_attention_varlen_bwd wrote) and writes the gradient of qkv in the same layout (dqkv, row
 * stride d_rs); dq_w, dq_b, dk_w, dk_b fp32 [64] each (any may be NULL) through fixed-order per-workgroup partials in a workspace of
 * vt_qknorm_rope_gqa_bwd_workspace_bytes().  Hq % Hkv == 0; strides >= 64 (Hq + 2 Hkv) and multiples of 8; buffers and tables 16-byte
 * aligned (VT_ERR_INVALID + vt_last_error otherwise).  Columns outside the three blocks and rows past M are neither read nor written.
 * The same kernels as vt_qknorm_rope_*: with Hq == Hkv, in_rs = 4D and out_rs = 3D the output is bit-identical to vt_qknorm_rope_fwd
 * called with L = M, and likewise the gradients to vt_qknorm_rope_bwd. */
int vt_qknorm_rope_gqa_fwd(const void* qkv, int64_t in_rs, int64_t M, int32_t Hq, int32_t Hkv, const float* q_w, const float* q_b,
                           const float* k_w, const float* k_b, float eps, const float* cos_tab, const float* sin_tab, void* qkv_out,
                           int64_t out_rs, vtStream stream);
size_t vt_qknorm_rope_gqa_bwd_workspace_bytes(void);
int vt_qknorm_rope_gqa_bwd(const void* qkv, int64_t in_rs, const void* dqkv_out, int64_t g_rs, int64_t M, int32_t Hq, int32_t Hkv,
                           const float* q_w, const float* k_w, float eps, const float* cos_tab, const float* sin_tab, void* dqkv, int64_t d_rs,
                           float* dq_w, float* dq_b, float* dk_w, float* dk_b, void* workspace, vtStream stream);
int vt_sigmoid_gate_fwd(const void* o, const void* qkvg, int64_t M, int32_t D, void* og, vtStream stream);
int vt_sigmoid_gate_bwd(const void* dog, const void* o, const void* qkvg, int64_t M, int32_t D, void* d_o, void* dqkvg, vtStream stream);
/* the same pair with the gate at any column offset and row stride (gate / dgate point at the first gate column of row 0; strides
 * >= D, multiples of 8): CrossAttention of model_design reads it from columns D..2D of the [M, 2D] projection [to_q ; to_gate].
 * gate = qkvg + 3D with stride 4D is vt_sigmoid_gate_*, bit for bit. */
int vt_sigmoid_gate_cols_fwd(const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* og, vtStream stream);
int vt_sigmoid_gate_cols_bwd(const void* dog, const void* o, const void* gate, int64_t gate_rs, int64_t M, int32_t D, void* d_o, void* dgate,
                             int64_t dgate_rs, vtStream stream);
int vt_geglu_fwd(const void* h, int64_t M, int32_t I, void* a, int64_t lda, vtStream stream);
int vt_geglu_bwd(const void* da, int64_t lda, const void* h, int64_t M, int32_t I, void* dh, vtStream stream);
/* dst[r, :] = scale * src[r, :] (fp32, may be in place) and/or its bf16 copy: the incoming gradient of a layer whose output was
 * rescaled by 1/sqrt(i+1), produced once for the fp32 residual path and the bf16 GEMM operand.  dim % 4 == 0. */
int vt_scale_rows(const float* src, float scale, int64_t rows, int32_t dim, float* dst_f32, void* dst_bf16, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * AR consumer (`LARP_AR`, models/larp_ar.py:233-438; consumes the tokenizer's `bottleneck_rep`): the kernels its layers need
 * beyond vt_gemm_* and vt_attention_causal_*.
 *   vt_rmsnorm_fwd / _bwd: RMSNorm (models/norm.py:6-17) y = x * rsqrt(mean(x^2) + eps) * w, x fp32 [rows, dim], y bf16, rstd fp32
 *     [rows] saved; backward adds `dres` (may be NULL), writes dx fp32 and/or bf16 and dw [dim] (fixed-order partial sums in
 *     `workspace` of vt_rmsnorm_bwd_workspace_bytes(dim)).  dim in {384, 768, 1024, 1280, 1536, 2560} (the llama-abs sizes).
 *     csrc/vt_rmsnorm.hip, with the two other RMSNorm families below: one pair of kernel templates, one dispatch.
 *   vt_swiglu_fwd / _bwd: FeedForward (larp_ar.py:122-136) a = silu(w1 x) * (w3 x) on the packed projection h [M, 2I] = [w3 x | w1 x].
 *   vt_decode_attention: one new token per sequence against the KV cache (larp_ar.py:138-190, `mask = causal_mask[:, None, pos]`):
 *     q bf16 [B, H, 64], caches bf16 [>=B, H, Lmax, 64], keys 0..n_keys-1 -> o bf16 [B, H, 64].
 *   vt_decode_attention_step: the same for the generation loop (ar/generate.py:99-123) without a host round trip: `pos_dev` (device
 *     int32: the new token's position = number of earlier keys) is read by the kernel, the new token's k / v are taken from the
 *     packed projection row qkv [B, 3 * H * 64] = [q | k | v], stored into the caches at `pos` (KVCache.update, larp_ar.py:153-161)
 *     and attended together with keys 0..pos-1.  With it one decode step has no host-side dependency and can be replayed as a hipGraph.
 * ------------------------------------------------------------------------------------------ */
int vt_rmsnorm_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, void* y_bf16, float* rstd, vtStream stream);
size_t vt_rmsnorm_bwd_workspace_bytes(int32_t dim);
int vt_rmsnorm_bwd(const void* dy_bf16, const float* x, const float* w, const float* rstd, const float* dres, int64_t rows, int32_t dim,
                   float* dx, void* dx_bf16, float* dw, void* workspace, vtStream stream);
/* vt_rmsnorm_any_*: the same kernels (csrc/vt_rmsnorm.hip), additionally at the widths 128, 256 and 512 of model_design (its 'small' is 512 wide, which
 * vt_rmsnorm_* refuses); bit-equal to vt_rmsnorm_* at the widths both accept. */
int vt_rmsnorm_any_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, void* y_bf16, float* rstd, vtStream stream);
size_t vt_rmsnorm_any_bwd_workspace_bytes(int32_t dim);
int vt_rmsnorm_any_bwd(const void* dy_bf16, const float* x, const float* w, const float* rstd, const float* dres, int64_t rows, int32_t dim,
                       float* dx, void* dx_bf16, float* dw, void* workspace, vtStream stream);
/* RMSNorm over each 64-element head vector of a bf16 row: q_norm / k_norm of model_design's attention layers
 * (models/model_design/base/transformer.py:18-27, 114-115, 134-135).  x, y, dy, dx bf16 [M, >= 64H] with a row stride each (>= 64H, a
 * multiple of 8; 16-byte aligned), w / dw fp32 [64].  Rounding of the reference under autocast: y = bf16(bf16(x * rstd) * w),
 * rstd = rsqrt(mean(x^2) + eps) in fp32.  Not in place (the backward reads x).  Backward: rstd recomputed,
 * dx = rstd g - x rstd^3 / 64 sum(x g), g = w dy; dx may be dy itself (same pointer and stride) and otherwise overlaps neither dy nor x; dw = sum dy x rstd from 512 per-workgroup partials in `workspace`
 * (vt_head_rmsnorm_bwd_workspace_bytes()) summed in a fixed order by a second launch: no float atomics, bit-identical run to run. */
int vt_head_rmsnorm_fwd(const void* x, int64_t x_rs, const float* w, float eps, int64_t M, int32_t H, void* y, int64_t y_rs, vtStream stream);
size_t vt_head_rmsnorm_bwd_workspace_bytes(void);
int vt_head_rmsnorm_bwd(const void* dy, int64_t dy_rs, const void* x, int64_t x_rs, const float* w, float eps, int64_t M, int32_t H, void* dx,
                        int64_t dx_rs, float* dw, void* workspace, vtStream stream);
/* Row passes of model_design's self-attention block and stack (models/model_design/base/transformer.py:46-85, 148-216; csrc/vt_design.hip,
 * the final norm csrc/vt_rmsnorm.hip).
 *   vt_qkrms_rope_fwd: the RMS twin of vt_qknorm_rope_fwd.  qkvg bf16 [M, >= 3D] (row stride in_rs; the block passes the [M, 4D] output of one
 *     GEMM on [to_qkv ; to_gate], columns q | k | v | gate) -> qkv_out bf16 [M, 3D] (row stride out_rs), the packed operand of vt_attention_fwd:
 *     q and k per head t = bf16(bf16(x rstd) w), rstd = rsqrt(mean(x^2) + eps) in fp32 (vt_head_rmsnorm_fwd), then the rotation of
 *     vt_rope_rotate (row m has position m % L, tables fp32 [L, 32]); v copied.  Bit for bit that chain of three passes.  D = 64 H, M = B L;
 *     row strides >= 3D and multiples of 8, buffers 16-byte aligned.  Columns past 3D and rows past M are neither read nor written.
 *   vt_qkrms_rope_bwd: dqkv bf16 [M, 3D] dense (from vt_attention_bwd) -> columns 0..3D of dqkvg (row stride out_rs): dq, dk rotated by the
 *     conjugate and rounded to bf16, then the backward of vt_head_rmsnorm_bwd (the same device functions, csrc/vt_headvec.h) with rstd recomputed from qkvg; dv copied.  dq_w / dk_w fp32 [64]
 *     (either may be NULL) from 512 per-workgroup partials in `workspace` (vt_qkrms_rope_bwd_workspace_bytes()) that a second launch sums in a
 *     fixed order.  Not in place.
 *   vt_residual_scale_fwd: out = x + float(bf16(s y)), the residual `x + res_scale * f(x)` (:176-183) with s = *scale_dev a 0-dim parameter
 *     in DEVICE memory (no host read: capturable).  x, y, out fp32 [rows, dim], y holding bf16 values; torch forms the product in bf16 (s is
 *     converted to bf16, the fp32 product rounded once) and adds the fp32 x after.  dim % 4 == 0, any rows, 16-byte aligned, not in place.
 *   vt_residual_scale_bwd: g = bf16(dout); dy = float(bf16(s g)); *dscale = sum g y in fp32 from at most 256 per-workgroup partials in
 *     `workspace` (vt_residual_scale_bwd_workspace_bytes()) summed in a fixed order by a second launch: bit-identical run to run.  dscale NULL
 *     (a frozen scale): y and workspace may be NULL too.
 *   vt_rmsnorm_any_f32_fwd / _bwd: vt_rmsnorm_any_* with an fp32, unrounded output y = x rstd w and an fp32 incoming gradient (final_norm of the
 *     stack, :211-216: the reference's RMSNorm on an fp32 input returns fp32).  The same kernel templates with T = float, so rstd, dx and dw are
 *     bit-equal to vt_rmsnorm_any_* on a gradient that bf16 represents exactly, and y differs by its rounding only.  Same widths, dw from fixed-order partials
 *     (vt_rmsnorm_any_f32_bwd_workspace_bytes(dim)). */
int vt_qkrms_rope_fwd(const void* qkvg, int64_t in_rs, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w, float eps,
                      const float* cos_tab, const float* sin_tab, void* qkv_out, int64_t out_rs, vtStream stream);
size_t vt_qkrms_rope_bwd_workspace_bytes(void);
int vt_qkrms_rope_bwd(const void* qkvg, int64_t in_rs, const void* dqkv, int64_t M, int32_t L, int32_t H, const float* q_w, const float* k_w,
                      float eps, const float* cos_tab, const float* sin_tab, void* dqkvg, int64_t out_rs, float* dq_w, float* dk_w,
                      void* workspace, vtStream stream);
int vt_residual_scale_fwd(const float* x, const float* y, const float* scale_dev, int64_t rows, int32_t dim, float* out, vtStream stream);
size_t vt_residual_scale_bwd_workspace_bytes(void);
int vt_residual_scale_bwd(const float* dout, const float* y, const float* scale_dev, int64_t rows, int32_t dim, float* dy, float* dscale,
                          void* workspace, vtStream stream);
int vt_rmsnorm_any_f32_fwd(const float* x, const float* w, float eps, int64_t rows, int32_t dim, float* y, float* rstd, vtStream stream);
size_t vt_rmsnorm_any_f32_bwd_workspace_bytes(int32_t dim);
int vt_rmsnorm_any_f32_bwd(const float* dy, const float* x, const float* w, const float* rstd, int64_t rows, int32_t dim, float* dx, float* dw,
                           void* workspace, vtStream stream);
int vt_swiglu_fwd(const void* h, int64_t M, int32_t I, void* a, vtStream stream);
int vt_swiglu_bwd(const void* da, const void* h, int64_t M, int32_t I, void* dh, vtStream stream);
int vt_decode_attention(const void* q, const void* k_cache, const void* v_cache, int32_t B, int32_t H, int64_t Lmax, int32_t n_keys, void* o,
                        vtStream stream);
int vt_decode_attention_step(const void* qkv, void* k_cache, void* v_cache, int32_t B, int32_t H, int64_t Lmax, const int32_t* pos_dev, void* o,
                             vtStream stream);
/* vt_decode_norm_linear: Linear(RMSNorm(x)) for the M <= 64 token rows of a decode step as ONE launch (x fp32 [M, K], norm_w fp32 [K],
 * W bf16 [N, K] row-major, K % 128 == 0, N % 16 == 0).  mode 0: out bf16 [M, ldo >= N] (wqkv); mode 1: W = [w3 ; w1] interleaved in slabs
 * of 8 + 8 rows, out bf16 [M, ldo >= N / 2] = silu(w1 y) * (w3 y) (FeedForward, larp_ar.py:135); mode 2: out fp32 [M, ldo >= N] holding
 * the bf16-rounded values (the LM head).  Bit-identical to vt_rmsnorm_fwd + vt_gemm_nt(tile 7) [+ vt_swiglu_fwd].
 * norm_w == NULL: x is the already normalised bf16 [M, K] operand (only the Linear and its epilogue are fused). */
int vt_decode_norm_linear(const void* x, const float* norm_w, float eps, const void* W_bf16, int32_t M, int32_t N, int32_t K, int32_t mode, void* out,
                          int64_t ldo, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * A stack of those layers as ONE enqueue per direction: `ResidualAttentionBlock.forward` (transformer.py:66-91) and the
 * backward autograd derives for it -- x <- (x + Attn(x)); x <- (x + ffd(x)); x <- x / sqrt(i+1) for i = 0..depth-1 -- the
 * transformer of every `autoencoder_*` model (Encoder / Decoder / Decoder_unify, base/blocks.py).  Per layer forward: cast,
 * 4 GEMMs, vt_qknorm_rope_fwd, vt_attention_fwd, vt_sigmoid_gate_fwd, vt_layernorm_fwd, vt_geglu_fwd (11 launches); backward
 * 16 launches + one grouped weight-gradient launch.  The caller owns parameters / gradients (fp32, the reference's layout:
 * to_qkv [4D, D], q/k_norm [64], out_proj [D, D], ffd LayerNorm [D], ffd.1 [2 inner, D], ffd.3 [D, inner]), the rotary tables
 * (fp32 [L, 32] each) and one workspace per forward whose backward is pending.  B * L % 64 == 0, D = 64 H.
 * ------------------------------------------------------------------------------------------ */
typedef struct { int32_t B, L, D, H, depth, inner; } vtGatedStackConfig;
typedef struct { float *to_qkv_w, *q_norm_w, *q_norm_b, *k_norm_w, *k_norm_b, *out_proj_w, *ln_w, *ln_b, *fc1_w, *fc2_w; } vtGatedLayerTensors;
typedef struct vtGatedStack vtGatedStack;
int vt_gated_stack_create(const vtGatedStackConfig* cfg, vtGatedStack** out);
void vt_gated_stack_destroy(vtGatedStack* st);
size_t vt_gated_stack_workspace_bytes(const vtGatedStack* st);
int vt_gated_stack_init_workspace(vtGatedStack* st, void* ws, vtStream stream);
/* repack != 0: refresh the bf16 operand copies of the weights first (after an optimizer step / load_state_dict) */
int vt_gated_stack_forward(vtGatedStack* st, const vtGatedLayerTensors* layers_host, const float* cos_tab, const float* sin_tab,
                           const float* x_in, void* ws, float* x_out, int32_t repack, vtStream stream);
int vt_gated_stack_backward(vtGatedStack* st, const vtGatedLayerTensors* layers_host, const float* cos_tab, const float* sin_tab,
                            const float* dy, void* ws, const vtGatedLayerTensors* grads_host, float* dx, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Fused Adam (+ optional EMA) over flat fp32 buffers: replaces optimizer.step() of torch.optim.Adam
 * (trainers/larp_tokenizer_trainer.py:160-212 builds Adam(lr, betas); :376-377 steps it) and
 * update_ema (trainers/base_trainer.py:769-779), one HBM-bound pass.  n % 4 == 0; step counts from 1;
 * ema may be NULL.  torch.optim.Adam semantics (L2 weight decay, no amsgrad).
 * ------------------------------------------------------------------------------------------ */
int vt_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int32_t step, float* ema, float ema_decay, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Whole-model engine: LARPTokenizer.forward = encode -> bottleneck(VQ) -> decode
 * (models/larp_tokenizer.py:400-428, 456-469, 489-496; TransformerEncoderParallel.forward
 * models/transformer.py:62-70; Bottleneck.forward models/bottleneck.py:170-188) and the backward
 * autograd derives for it, as ONE enqueue per direction (no per-op host work; hipGraph-capturable).
 * Mixed precision follows torch.autocast(bf16) on the reference: fp32 parameters, residual stream,
 * LayerNorm statistics, VQ and pixels; bf16 MFMA operands with fp32 accumulation.
 *
 * The caller owns: parameters/gradients (fp32, reference state-dict layout), one workspace of
 * vt_tokenizer_workspace_bytes() (zeroed once by vt_tokenizer_init_workspace), and the outputs.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t B, C, T, S, pt, p;            /* batch per GPU, channels, frames, side, patch sizes      */
    int32_t D, H, depth_enc, depth_dec;   /* hidden (768), heads (12 => head_dim 64), block counts   */
    int32_t Nq, d, K;                     /* bottleneck_token_num, bottleneck_dim, codebook_size     */
    int32_t vq_mode, l2_normalized;       /* 0 l2-argmin | 1 cos-argmax | 2 cos-sample               */
    float inv_tau, beta, codebook_w;      /* 1/stochastic_temperature, commitment / codebook weights */
    int32_t freeze_codebook;              /* 1: no codebook gradient is computed or written (bottleneck_type 'sq',
                                             models/larp_tokenizer.py:225-229: frozen 196 560 x 24 codebook) */
} vtTokenizerConfig;

typedef struct {                          /* one timm Block; same struct (non-const use) for grads   */
    float *norm1_w, *norm1_b, *qkv_w, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} vtBlockTensors;

typedef struct {                          /* parameters OR their gradients (buffers NULL in grads)   */
    float *pe_w, *pe_b;                   /* x_embedder.proj.{weight [D,C*pt*p*p], bias}             */
    float *enc_patch_pe;                  /* encoder_patch_pe [Nv,D]           (buffer)              */
    float *enc_query;                     /* encoder_latent_query_embed [Nq,D]                        */
    float *dec_latent_pe;                 /* decoder_latent_pe [Nq,D]          (buffer)              */
    float *dec_patch_query;               /* decoder_patch_query_embed [Nv,D]  (buffer)              */
    float *dec_token_type;                /* decoder_patch_query_token_type_embed [D] or NULL         */
    float *in_w, *in_b, *out_w, *out_b;   /* bottleneck.in_linear / out_linear                        */
    float *codebook;                      /* bottleneck.regularizer.embedding.weight [K,d]            */
    float *head_norm_w, *head_norm_b, *head_w, *head_b; /* final_layer.norm_final / linear          */
    const vtBlockTensors* enc_blocks;     /* host array [depth_enc]                                   */
    const vtBlockTensors* dec_blocks;     /* host array [depth_dec]                                   */
} vtTokenizerTensors;

typedef struct {                          /* forward outputs (device, caller-owned)                   */
    float* pred_frames;                   /* [B,C,T,S,S]                                              */
    float* encoded;                       /* [B,Nq,D]  'encoded'                                      */
    int64_t* indices;                     /* [B,Nq]    'bottleneck_rep'                               */
    float* projected_z;                   /* [B*Nq,d]  'projected_z' (in_linear output)               */
    float* unregularized_z;               /* [B*Nq,d]                                                 */
    float* regularized_z;                 /* [B*Nq,d]                                                 */
    float* emb;                           /* [K,d]     'emb' (normalised codebook)                    */
    float* losses;                        /* [4] loss_q, loss_commit, loss_codebook, mse              */
    float* input_norms;                   /* [2] input_norm_first, input_norm_last                    */
} vtTokenizerOutputs;

typedef struct vtTokenizer vtTokenizer;

int vt_tokenizer_create(const vtTokenizerConfig* cfg, vtTokenizer** out);
void vt_tokenizer_destroy(vtTokenizer* tk);
size_t vt_tokenizer_workspace_bytes(const vtTokenizer* tk);
int vt_tokenizer_init_workspace(vtTokenizer* tk, void* workspace, vtStream stream);
/* fp32 master weights -> packed bf16 operands (call after every optimizer step) */
int vt_tokenizer_pack(vtTokenizer* tk, const vtTokenizerTensors* params, void* workspace, vtStream stream);
/* encode: video -> encoded + VQ outputs.  decode: encoded -> pred_frames.  forward = both. */
int vt_tokenizer_encode(vtTokenizer* tk, const vtTokenizerTensors* params, const float* video, void* workspace,
                        const vtTokenizerOutputs* out, uint64_t seed, vtStream stream);
int vt_tokenizer_decode(vtTokenizer* tk, const vtTokenizerTensors* params, const float* encoded, void* workspace,
                        float* pred_frames, vtStream stream);
/* bottleneck.decode (models/bottleneck.py:166-168): indices -> encoded */
int vt_tokenizer_codes_to_encoded(vtTokenizer* tk, const vtTokenizerTensors* params, const int64_t* indices, void* workspace,
                                  float* encoded, vtStream stream);
/* backward of forward(); stages run in order head(0), decoder blocks (1..depth_dec, last block
 * first), bottleneck, encoder blocks, patch-embed; [stage_begin, stage_end) lets the caller
 * interleave gradient all-reduce buckets between stages.  d_pred [B,C,T,S,S] fp32;
 * gscal = device {dL/dloss_q, dL/dloss_commit, dL/dloss_codebook} or NULL.
 * The weight-gradient GEMMs of up to 4 consecutive transformer blocks are deferred and issued as ONE
 * grouped launch (768 tiles of 192x192 = 3 full rounds of the 256 CUs), so the gradients of a stage
 * may become final a few stages later: *final_through (optional) receives the number of leading stages
 * whose gradients are complete once the enqueued work has run. */
int32_t vt_tokenizer_num_backward_stages(const vtTokenizer* tk);
/* device-side per-call counter of the stochastic quantizer (see vt_vq_forward_ctr); NULL (the default) = the by-value seed alone */
int vt_tokenizer_set_seed_counter(vtTokenizer* tk, const uint32_t* seed_counter);
/* Split K in the BACKWARD input-gradient GEMMs that would leave most CUs idle (vtGemmNT.splitk_ws; one or two clips per GPU): on by
 * default (VT_GEMM_SPLITK=0 in the environment starts every handle with it off).  Forward GEMMs are never split: a clip's tokens and
 * reconstruction do not depend on the batch it runs in.  With the split, its GRADIENTS are summed in a different fp32 order than in a
 * larger batch and, re-rounded to bf16 layer after layer, differ from them at the bf16 noise level (~5e-3 relative on the deepest
 * layers) instead of ~1e-6: switch it off where bit-stable gradients across batch sizes matter more than the ~8 % it buys. */
int vt_tokenizer_set_split_k(vtTokenizer* tk, int32_t on);
/* Data-parallel runs (ABI 7).  The weight gradients of four consecutive blocks are produced by ONE grouped launch, so a group's gradients are
 * final -- and DistributedDataParallel's bucketed all-reduce of them (trainers/base_trainer.py:388) can start -- only there; by default the
 * encoder's blocks 3..0 finish at the very end of backward and their 113 MB (config B) are reduced with nothing left to overlap.  n > 0: the
 * encoder's blocks below n flush block by block (n = 3: groups 3-2 | 1 | 0), leaving one block's gradients for the exposed tail at the price
 * of three launches that do not fill whole rounds of the chip.  Bit-identical gradients.  parallel.DataParallelTokenizer sets n = 3. */
int vt_tokenizer_set_wgrad_tail(vtTokenizer* tk, int32_t n);
/* Data-parallel runs (ABI 7).  side != NULL: the grouped weight-gradient launches and the partial-sum reductions of the same blocks are
 * enqueued on `side` instead of the caller's stream, behind an event of the caller's stream; the caller's stream waits for them at the last
 * stage of backward (and before it rewrites an operand buffer a pending group still reads).  They are off the critical path of backward, and
 * while a collective's workgroups hold CUs the exact-fit GEMM launches of the main stream leave most of the chip idle in their extra round:
 * an independent stream fills it.  A consumer of a finished gradient slice (final_through of vt_tokenizer_backward) must wait for BOTH
 * streams.  Same kernels on the same operands: bit-identical gradients.  NULL restores the single-stream schedule.  Not capturable. */
int vt_tokenizer_set_wgrad_stream(vtTokenizer* tk, vtStream side);
/* Blocks per grouped weight-gradient launch, 1..4 (default 4 = 768 tiles = three whole rounds of the chip at config B).  (ABI 7) */
int vt_tokenizer_set_wgrad_batch(vtTokenizer* tk, int32_t n);
int vt_tokenizer_backward(vtTokenizer* tk, const vtTokenizerTensors* params, const float* d_pred, const float* gscal,
                          void* workspace, const vtTokenizerTensors* grads, int32_t stage_begin, int32_t stage_end,
                          int32_t* final_through, vtStream stream);
/* Data-parallel runs (ABI 8).  on != 0: a collective's workgroups share the chip with the backward (DistributedDataParallel's bucketed
 * all-reduce, trainers/base_trainer.py:388), so the backward's GEMMs with more 192x192 tiles than CUs are launched one tile per workgroup
 * (vtGemmNT.tile = 6) and the hardware hands tiles to whichever CU is free.  Bit-identical gradients.  (ABI 7 tied this to
 * vt_tokenizer_set_wgrad_tail(n > 0).) */
int vt_tokenizer_set_data_parallel(vtTokenizer* tk, int32_t on);
/* vt_tokenizer_backward for a caller that reduces finished gradient slices between stages (ABI 8): runs stages from stage_begin until
 * *final_through advances (a group of weight gradients was flushed) or the last stage is done; *stage_next = the stage to go on with
 * (== vt_tokenizer_num_backward_stages() when the backward is complete).  ~8 calls per backward at 12 + 12 blocks instead of 27. */
int vt_tokenizer_backward_until_flush(vtTokenizer* tk, const vtTokenizerTensors* params, const float* d_pred, const float* gscal,
                                      void* workspace, const vtTokenizerTensors* grads, int32_t stage_begin, int32_t* stage_next,
                                      int32_t* final_through, vtStream stream);

/* The same engine with the KL bottleneck ('skl', see vt_kl_forward) instead of VQ: in_linear has 2d outputs (in_w [2d, D], in_b [2d]),
 * vt_kl_forward / vt_kl_backward take the place of the quantizer.  vt_tokenizer_create_kl ignores K, vq_mode, l2_normalized, inv_tau,
 * beta, codebook_w and freeze_codebook.  A KL handle works with pack, decode, backward, backward_until_flush, set_seed_counter and
 * every set_* option; there params.codebook is NULL and gscal = device {dL/dloss_kl} or NULL.  vt_tokenizer_encode and
 * vt_tokenizer_codes_to_encoded on a KL handle, and vt_tokenizer_encode_kl on a VQ handle, return VT_ERR_INVALID. */
typedef struct {                          /* forward outputs of a KL handle (device, caller-owned)    */
    float* encoded;                       /* [B,Nq,D]  'encoded' = out_linear(sample)                  */
    float* mean;                          /* [B*Nq,d]  'bottleneck_rep' (may be NULL)                  */
    float* projected_z;                   /* [B*Nq,2d] in_linear output (may be NULL)                  */
    float* regularized_z;                 /* [B*Nq,d]  the sample (may be NULL)                        */
    float* noise;                         /* [B*Nq,d]  eps of the sample (may be NULL)                 */
    float* loss_kl;                       /* [1]                                                       */
    float* input_norms;                   /* [2] input_norm_first, input_norm_last (may be NULL)       */
} vtTokenizerKLOutputs;
int vt_tokenizer_create_kl(const vtTokenizerConfig* cfg, vtTokenizer** out);
int vt_tokenizer_encode_kl(vtTokenizer* tk, const vtTokenizerTensors* params, const float* video, void* workspace,
                           const vtTokenizerKLOutputs* out, uint64_t seed, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * A stack of timm Blocks on its own (fp32 [B, L, D] in and out): `transformer_encoder_parallel` / `_fused` called
 * outside LARPTokenizer (models/transformer.py:8-70; cat / slice of context and query stay with the caller) and the
 * discriminator's encoder (models/loss.py:150-155: width 384, 12 heads of 32, L = 1025).  head_dim 64 or 32; D in
 * {128,256,384,512,768,1024}; any L.  The forward re-packs the bf16 operand copies of the weights, saves its
 * activations in `ws` (vt_stack_workspace_bytes, zeroed once by vt_stack_init_workspace -- padded rows must stay
 * zero) and the backward of the SAME ws returns dL/dx and, unless need_wgrad == 0 (frozen stack: input gradient
 * only), every parameter gradient (weight gradients of 4 blocks per grouped launch).  A second forward before
 * the first one's backward needs its own ws.
 * ------------------------------------------------------------------------------------------ */
typedef struct { int32_t B, L, D, H, depth; } vtStackConfig;
typedef struct vtStack vtStack;
int vt_stack_create(const vtStackConfig* cfg, vtStack** out);
void vt_stack_destroy(vtStack* st);
size_t vt_stack_workspace_bytes(const vtStack* st);
int vt_stack_init_workspace(vtStack* st, void* ws, vtStream stream);
int vt_stack_set_split_k(vtStack* st, int32_t on);   /* as vt_tokenizer_set_split_k */
int vt_stack_forward(vtStack* st, const vtBlockTensors* blocks_host, const float* x_in, void* ws, float* x_out, vtStream stream);
int vt_stack_backward(vtStack* st, const vtBlockTensors* blocks_host, const float* dy, void* ws, const vtBlockTensors* grads_host,
                      float* dx, int32_t need_wgrad, vtStream stream);

/* ------------------------------------------------------------------------------------------
 * Rotary position embedding on the plain block stack: `ResidualAttentionBlock1` (models/model_new/base/simpletransformer.py:26-121),
 * the layer of `autoencoder_convpatchify_simplytransformer` = the timm Block above with apply_rotary_emb (base/rope.py:18-24) on q and k.
 *   vt_rope_rotate: rotates the q and k column blocks of the packed bf16 attention operand qkv [M, 3D] (row stride ld >= 2D, ld % 8 == 0,
 *     D = 64 H: head_dim 64 only, columns [q | k | v] as vt_attention_fwd reads them) IN PLACE; columns 2D.. (v) are neither read nor
 *     written, nor are rows M.. of a padded buffer.  Row m has position m % L (any M, any L).  cos_tab / sin_tab: fp32 [L, 32], the tables
 *     of vt_qknorm_rope_fwd (real / imaginary part of freqs_cis); pair j of every head is (x[2j], x[2j+1]).  conjugate = 0:
 *     y = x (cos + i sin), the forward; conjugate = 1: y = x (cos - i sin), the backward of the rotation, applied to dq and dk.  bf16 in,
 *     fp32 arithmetic, one rounding to bf16 (`.type_as(x)` on the bf16 Linear output under autocast).  qkv and the tables 16-byte aligned.
 *     Checked on the host: VT_ERR_INVALID + vt_last_error.
 *   vt_stack_forward_rotary / vt_stack_backward_rotary: vt_stack_forward / vt_stack_backward with the rotation between the qkv GEMM and
 *     the attention (the saved qkv is the rotated one) and its conjugate on dqkv directly behind the attention backward, before the qkv
 *     input-gradient GEMM and the queued weight gradient read it.  The tables (device memory, [L, 32] for the stack's L) travel with every
 *     call and nothing is kept on the handle, so one vtStack serves rotary and plain callers.  cos_tab == sin_tab == NULL is the plain
 *     stack, bit for bit (vt_stack_forward / vt_stack_backward are exactly that).  Tables given: head_dim must be 64.
 * ------------------------------------------------------------------------------------------ */
int vt_rope_rotate(void* qkv, int64_t ld, int64_t M, int32_t L, int32_t H, const float* cos_tab, const float* sin_tab, int32_t conjugate,
                   vtStream stream);
int vt_stack_forward_rotary(vtStack* st, const vtBlockTensors* blocks_host, const float* cos_tab, const float* sin_tab, const float* x_in,
                            void* ws, float* x_out, vtStream stream);
int vt_stack_backward_rotary(vtStack* st, const vtBlockTensors* blocks_host, const float* cos_tab, const float* sin_tab, const float* dy,
                             void* ws, const vtBlockTensors* grads_host, float* dx, int32_t need_wgrad, vtStream stream);

#ifdef __cplusplus
}
#endif
#endif /* VT_HIP_H */
