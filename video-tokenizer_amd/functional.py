"""Autograd functions over the C-ABI ops: the standalone forwards of the reference's sub-modules.

The tokenizer step itself runs in the fused C++ engine (engine.py).  The reference resolves its
sub-modules by registry name as well (`transformer_encoder_parallel`, `transformer_encoder_fused`,
`bottleneck`, `vq`) and calls them on their own -- and the GAN branch of the step is a stack
of the same timm Blocks (models/loss.py:119-204).  These functions give those call sites the same
kernels: every matrix product, LayerNorm, attention and codebook search below is a libvt_hip call; torch
only owns the tensors, the autograd graph and a few O(B x D) glue ops.

Mixed-precision contract = the engine's: fp32 residual stream and LayerNorm statistics,
bf16 MFMA operands with fp32 accumulation, Linear outputs rounded to bf16 where autocast would.
No CPU path: CPU tensors are refused by hip.ptr().

The layers of the reference's `autoencoder_design` are here as well: CrossAttentionLayer, and the self-attention block of its stack
(SelfAttentionLayer, FeedForwardLayer, ResidualScale with the learnable 0-dim residual scale read on the device, RMSNormF32 for the stack's
fp32 final norm); design.py holds their parameters.

The packed `titok` model's Functions are at the end: VarlenAttend / VarlenAttentionLayer (the layer of models/model_titok), its residual sibling
and VarlenFeedForwardLayer (one Function per half block), and the data movement of csrc/vt_packed.hip (PatchRowsClips, UnpatchifyClips, PackedScatter,
PackedGather); varlen.py and titok_model.py hold their parameters.

Last come the ends of `autoencoder_dualpatch` (DualPatchEmbed, DualConvTransposePatch, DualDecoderStream: a clip cut along time into two segments
with a patch size each, the two-segment entry points of csrc/vt_patch.hip); dualpatch.py holds their parameters.

The 3D ResNet ends of `autoencoder_cnnvit` close the file (Conv3x3x3, GroupNormSwish, UpsampleNearest, VideoToChannelsLast, ChannelsLastToVideo:
csrc/vt_conv3d.hip, vt_groupnorm.hip); cnnvit.py holds their parameters.  They take and return logical [B, C, T, H, W] bf16 tensors whose
memory is channels-last ([B, T, H, W, C], torch.channels_last_3d), which is what the kernels read.
"""
import ctypes
import functools
import inspect
import operator

import torch

from . import hip, packs


def _pad64(m):
    return (m + 63) // 64 * 64


def _zeros(rows, cols, dev, dtype=torch.bfloat16):
    return torch.zeros(rows, cols, device=dev, dtype=dtype)


class _WeightGrads:
    """The weight gradients of one backward, the Python counterpart of the C++ engine's pending list (vt_engine.hip, flush_wgrads): add()
    queues dW = dY^T X and returns its fp32 [P, Q] tensor, run() fills all of them with one grouped launch, in the order they were added.  The
    kernels contract over rows in steps of 64: operands with a ragged row count are zero-padded here, each distinct tensor once per queue."""

    def __init__(self):
        self.jobs, self.padded = [], {}

    def _rows64(self, t):
        M = t.shape[0]
        if M % 64 == 0:
            return t
        hit = self.padded.get(id(t))              # (t, copy): holding t keeps its id from being given to another tensor
        if hit is None:
            z = torch.zeros(_pad64(M), t.shape[1], device=t.device, dtype=t.dtype)
            z[:M].copy_(t)
            hit = self.padded[id(t)] = (t, z)
        return hit[1]

    def add(self, dY, X, want=True):
        if not want:
            return None
        out = torch.empty(dY.shape[1], X.shape[1], device=dY.device)
        self.jobs.append(dict(A=self._rows64(dY), B=self._rows64(X), out=out))
        return out

    def run(self):
        for i in range(0, len(self.jobs), hip.TN_MAX_GROUP):
            hip.gemm_tn_grouped(self.jobs[i:i + hip.TN_MAX_GROUP])


def _split_rows(dw, n):
    """the gradients of the two weights a GEMM ran concatenated along N: rows [:n] and [n:] of dw (None stays None)"""
    return (None, None) if dw is None else (dw[:n], dw[n:])


@functools.lru_cache(maxsize=None)
def _forward_args(cls):
    """{argument name of cls.forward behind ctx: its position}, read once per Function class"""
    return {name: i for i, name in enumerate(tuple(inspect.signature(cls.forward).parameters)[1:])}


@functools.lru_cache(maxsize=None)
def _need_table(cls, needs):
    return dict(zip(_forward_args(cls), needs))


def _needs(ctx, cls):
    """ctx.needs_input_grad by the name of the forward's argument: a table shared by every backward of the class with this pattern, to read only"""
    return _need_table(cls, ctx.needs_input_grad)


def _grads(ctx, cls, **named):
    """the return tuple of cls.backward: the gradients given by argument name, in the forward's order; None where none was given or needed.
    A name the forward does not have is a KeyError.  (A few look-ups per call: the steps of these layers are bound by the host.)"""
    position, need = _forward_args(cls), ctx.needs_input_grad
    out = [None] * len(need)
    for name, g in named.items():
        i = position[name]
        out[i] = g if need[i] else None
    return tuple(out)


# The parameters of one block / one gated layer, in the field order of the C structs: the only spelling of either list.
BLOCK_PARAM_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias",          # hip.BLOCK_FIELDS; below a
                     "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")  # transformer.Block / SimpleBlock
GATED_PARAM_NAMES = ("attn_layer.{0}.to_qkv.weight", "attn_layer.{0}.q_norm.weight", "attn_layer.{0}.q_norm.bias",    # hip.GATED_FIELDS; below a
                     "attn_layer.{0}.k_norm.weight", "attn_layer.{0}.k_norm.bias", "attn_layer.{0}.out_proj.weight",  # titok.ResidualAttentionBlock,
                     "ffd_layer.{0}.0.weight", "ffd_layer.{0}.0.bias", "ffd_layer.{0}.1.weight", "ffd_layer.{0}.3.weight")   # {0} = the layer
PARAMS_PER_BLOCK, PARAMS_PER_GATED_LAYER = len(hip.BLOCK_FIELDS), len(hip.GATED_FIELDS)
assert len(BLOCK_PARAM_NAMES) == PARAMS_PER_BLOCK and len(GATED_PARAM_NAMES) == PARAMS_PER_GATED_LAYER
_block_getter = operator.attrgetter(*BLOCK_PARAM_NAMES)


def block_params(blocks):
    """flat parameter list of an nn.ModuleList / nn.Sequential of transformer.Block in BLOCK_PARAM_NAMES order"""
    return [p for b in blocks for p in _block_getter(b)]


@functools.lru_cache(maxsize=None)
def _gated_getter(i):
    return operator.attrgetter(*(n.format(i) for n in GATED_PARAM_NAMES))


def gated_params(stack):
    """flat parameter list of a titok.ResidualAttentionBlock in GATED_PARAM_NAMES order, layer by layer"""
    return [p for i in range(stack.num_layer) for p in _gated_getter(i)(stack)]


class _Workspace:
    """a pooled workspace: its bytes, and the pack key (packs.pack_key) of the weight copies a gated stack left in them"""
    __slots__ = ("buf", "pack_key")

    def __init__(self, buf):
        self.buf, self.pack_key = buf, None


class _StackPool:
    """Host side of one stack engine (`prefix`_create / _workspace_bytes, its config and per-layer tensor structs): one handle per geometry,
    the ctypes arrays of a call, and the workspaces.  A workspace is zero-initialised (= `prefix`_init_workspace), stays with a forward until its
    backward has run, and is pooled again after that (or right behind an inference forward: stream order); its padded rows are still zero then."""

    def __init__(self, prefix, config, tensors, fields):
        self.prefix, self.config, self.tensors, self.fields = prefix, config, tensors, fields
        self.handles = {}      # geometry -> (handle, workspace bytes)
        self.free = {}         # (geometry, device) -> [_Workspace]

    def handle(self, key):
        h = self.handles.get(key)
        if h is None:
            cfg = self.config(*key)
            out = ctypes.c_void_p()
            hip.check(getattr(hip.lib(), self.prefix + "_create")(ctypes.byref(cfg), ctypes.byref(out)), self.prefix + "_create")
            h = self.handles[key] = (out, int(getattr(hip.lib(), self.prefix + "_workspace_bytes")(out)))
        return h

    def array(self, tensors, depth):
        arr = (self.tensors * depth)()
        for i in range(depth):
            for j, name in enumerate(self.fields):
                setattr(arr[i], name, tensors[i * len(self.fields) + j].data_ptr())
        return arr

    def take(self, key, dev):
        free = self.free.setdefault((key, str(dev)), [])
        return free.pop() if free else _Workspace(torch.zeros(self.handle(key)[1], dtype=torch.uint8, device=dev))

    def recycle(self, key, ws):
        self.free[(key, str(ws.buf.device))].append(ws)

    def after_forward(self, ctx, key, ws, params, tabs):
        if any(ctx.needs_input_grad):     # a backward may follow: the activations stay in ws until then
            ctx.key, ctx.ws, ctx.params, ctx.tabs = key, ws, params, tabs
        else:                             # inference: the workspace is free again behind this forward
            self.recycle(key, ws)

    def claim(self, ctx, who):
        """the workspace of ctx's forward, once: the caller recycles it behind its backward launch"""
        ws, ctx.ws = ctx.ws, None
        if ws is None:
            raise RuntimeError(f"{who}: second backward through the same forward (its workspace was recycled)")
        return ws


_BLOCKS = _StackPool("vt_stack", hip.StackConfig, hip.BlockTensors, hip.BLOCK_FIELDS)                 # geometry (B, L, D, H, depth)
_GATED = _StackPool("vt_gated_stack", hip.GatedStackConfig, hip.GatedLayerTensors, hip.GATED_FIELDS)  # geometry (B, L, D, H, depth, inner)
_stack, _block_array = _BLOCKS.handle, _BLOCKS.array      # for callers that drive the C entry points themselves (tests/test_simple_gpu.py)


class BlockStack(torch.autograd.Function):
    """depth x timm Block(dim, heads, mlp_ratio=4, qkv_bias=False) on x fp32 [B, L, D]; head_dim 64 or 32, any L.
    One vt_stack_forward_rotary / vt_stack_backward_rotary call each: the C++ engine enqueues the tokenizer's own block sequence
    (8 launches per block forward, 13 backward + one grouped weight-gradient launch per 4 blocks; reference: timm Block
    as built at models/transformer.py:18-25, 52-59).  Frozen parameters (requires_grad False everywhere: the
    generator-side pass through the discriminator) skip the weight-gradient GEMMs.
    cos = sin = None is that plain stack.  cos / sin given (fp32 [L, 32] device tables, titok.rope_tables; head_dim 64): rotary position
    embedding on q and k, depth x Block of `ResidualAttentionBlock1` (models/model_new/base/simpletransformer.py:74-87): the same
    launch sequence plus one vt_rope_rotate per block and direction.  The tables travel with the call, so both kinds share the
    handles and the workspace pool."""

    @staticmethod
    def forward(ctx, x, cos, sin, n_head, *params):
        hip.require_gpu(x, cos, sin, *params)
        assert x.dim() == 3 and x.dtype == torch.float32
        B, L, D = x.shape
        depth = len(params) // PARAMS_PER_BLOCK
        assert depth * PARAMS_PER_BLOCK == len(params) and D % n_head == 0
        if cos is not None:
            assert D == 64 * n_head
            assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.shape == (L, 32) == sin.shape
            cos, sin = cos.contiguous(), sin.contiguous()
        key = (B, L, D, n_head, depth)
        handle, _ = _BLOCKS.handle(key)
        params = tuple(p_.detach().float().contiguous() for p_ in params)
        ws = _BLOCKS.take(key, x.device)
        xin = x.contiguous()
        out = torch.empty_like(xin)
        hip.check(hip.lib().vt_stack_forward_rotary(handle, _BLOCKS.array(params, depth), hip.ptr(cos), hip.ptr(sin), hip.ptr(xin), hip.ptr(ws.buf),
                                                    hip.ptr(out), hip.stream()), "vt_stack_forward_rotary")
        _BLOCKS.after_forward(ctx, key, ws, params, (cos, sin))
        return out

    @staticmethod
    def backward(ctx, dy):
        ws = _BLOCKS.claim(ctx, "BlockStack")
        B, L, D, H, depth = ctx.key
        handle, _ = _BLOCKS.handle(ctx.key)
        need = ctx.needs_input_grad[4:]
        grads = [torch.empty_like(p_) for p_ in ctx.params]     # LayerNorm / bias gradients are always produced
        dx = torch.empty(B, L, D, device=dy.device, dtype=torch.float32)
        dyc = dy.contiguous().float()
        cos, sin = ctx.tabs
        hip.check(hip.lib().vt_stack_backward_rotary(handle, _BLOCKS.array(ctx.params, depth), hip.ptr(cos), hip.ptr(sin), hip.ptr(dyc), hip.ptr(ws.buf),
                                                     _BLOCKS.array(grads, depth), hip.ptr(dx), int(any(need)), hip.stream()), "vt_stack_backward_rotary")
        _BLOCKS.recycle(ctx.key, ws)
        return (dx, None, None, None, *[g if n else None for g, n in zip(grads, need)])


def block_stack(x, blocks, n_head):
    return BlockStack.apply(x, None, None, n_head, *block_params(blocks))


def rotary_block_stack(x, blocks, n_head, cos, sin):
    return BlockStack.apply(x, cos, sin, n_head, *block_params(blocks))


class GatedStack(torch.autograd.Function):
    """The stack of TiTok-style gated layers (models/model_new/base/transformer.py:66-91): depth x {x += Attn(x); x += ffd(x); x /= sqrt(i+1)}
    on x fp32 [B, L, D] (B * L % 64 == 0, D = 64 * heads): ONE vt_gated_stack_forward / _backward call each (11 launches per layer forward,
    17 backward, issued by the C++ engine).  params: GATED_PARAM_NAMES order per layer.  The workspace carries the saved activations and the
    bf16 operand copies of the weights; `pack_key` (packs.pack_key) identifies the weight versions a workspace was packed for."""

    @staticmethod
    def forward(ctx, x, cos, sin, n_head, pack_key, *params):
        hip.require_gpu(x, cos, sin, *params)
        assert x.dim() == 3
        B, L, D = x.shape
        depth = len(params) // PARAMS_PER_GATED_LAYER
        assert depth * PARAMS_PER_GATED_LAYER == len(params)
        inner = params[9].shape[1]
        key = (B, L, D, n_head, depth, inner)
        handle, _ = _GATED.handle(key)
        params = tuple(p_.detach().float().contiguous() for p_ in params)
        ws = _GATED.take(key, x.device)
        repack = ws.pack_key != pack_key
        ws.pack_key = pack_key
        xin = x.contiguous().float()
        out = torch.empty_like(xin)
        hip.check(hip.lib().vt_gated_stack_forward(handle, _GATED.array(params, depth), hip.ptr(cos), hip.ptr(sin), hip.ptr(xin), hip.ptr(ws.buf),
                                                   hip.ptr(out), int(repack), hip.stream()), "vt_gated_stack_forward")
        _GATED.after_forward(ctx, key, ws, params, (cos, sin))
        return out

    @staticmethod
    def backward(ctx, dy):
        ws = _GATED.claim(ctx, "GatedStack")
        B, L, D, H, depth, inner = ctx.key
        handle, _ = _GATED.handle(ctx.key)
        grads = [torch.empty_like(p_) for p_ in ctx.params]
        dx = torch.empty(B, L, D, device=dy.device, dtype=torch.float32)
        dyc = dy.contiguous().float()
        cos, sin = ctx.tabs
        hip.check(hip.lib().vt_gated_stack_backward(handle, _GATED.array(ctx.params, depth), hip.ptr(cos), hip.ptr(sin), hip.ptr(dyc), hip.ptr(ws.buf),
                                                    _GATED.array(grads, depth), hip.ptr(dx), hip.stream()), "vt_gated_stack_backward")
        _GATED.recycle(ctx.key, ws)
        need = ctx.needs_input_grad[5:]
        return (dx, None, None, None, None, *[g if n else None for g, n in zip(grads, need)])


# The patch ends: a Conv3d / ConvTranspose3d with kernel = stride = (pt, ph, pw) is a patch gather / scatter (csrc/vt_patch.hip) and one GEMM
# per temporal segment.  The per-segment pieces below are shared by PatchEmbed, ConvTransposePatch (one segment) and their Dual siblings (two);
# each Function keeps the order of its own library calls.
def _f32(t):
    return None if t is None else t.detach().float().contiguous()


def _conv_tokens(patches, wb, bias, pos, n, **into):
    """Conv3d forward of one segment: bf16 patch rows [B * n, Kp] x the packed weight -> tokens fp32 [B * n, D], rounded to bf16 like the conv
    under autocast, then + pos [n, D] (or None) in fp32 in the epilogue; into = omap=, out= to write the rows into a stream"""
    kw = dict(rowmod=_f32(pos.reshape(n, -1)), rowmod_period=n) if pos is not None else {}
    return hip.gemm_nt(patches, wb, hip.EPI_F32, bias=_f32(bias), round_bf16=True, **kw, **into)


def _convt_weight(weight):
    """ConvTranspose3d weight [D, C, pt, ph, pw] packed as the B operand [Kp, D] of the forward; -> (wb, wt = [D, Kp])"""
    return hip.pack_weight(weight.reshape(weight.shape[0], -1).t().contiguous())


def _convt_rows(x, wb, bias, taps):
    """ConvTranspose3d forward of one segment: bf16 tokens [M, D] -> patch rows fp32 [M, Kp] in (c, dt, dy, dx) order, each channel's bias on its
    taps = pt * ph * pw columns, rounded to bf16 like the conv under autocast"""
    return hip.gemm_nt(x, wb, hip.EPI_F32, bias=_f32(bias).repeat_interleave(taps).contiguous(), round_bf16=True)


def _convt_input_grad(drows, wt, **into):
    """d tokens [M, D] of one segment from the bf16 patch rows of d video, a bf16 gradient under autocast; into = omap=, out="""
    return hip.gemm_nt(drows, wt, hip.EPI_F32, round_bf16=True, **into)


def _convt_bias_grad(drows, C):
    """d bias [C] of one segment: the column sums of the patch rows of d video, summed over each channel's taps"""
    return hip.colsum(drows, rows=drows.shape[0]).reshape(C, -1).sum(dim=1)


def _shaped(dw, shape):
    return None if dw is None else dw.reshape(shape)


class PatchEmbed(torch.autograd.Function):
    """PatchEmbed3D.forward (models/embed.py:85-116): Conv3d(kernel = stride = (pt,p,p)) as patch gather + one GEMM,
    bf16-rounded like the conv under autocast, then (optionally) + pos_embed [N, D] in fp32, fused in the epilogue."""

    @staticmethod
    def forward(ctx, video, weight, bias, pos_embed):
        hip.require_gpu(video, weight, bias, pos_embed)
        D, C, pt, p, _ = weight.shape
        B = video.shape[0]
        video = video.contiguous().float()
        patches = hip.patchify(video, pt, p)                       # [B*N, Kp] bf16, (c,dt,dy,dx) inside a patch
        M = patches.shape[0]
        wb, wt = hip.pack_weight(weight)
        tok = _conv_tokens(patches, wb, bias, pos_embed, M // B)
        ctx.save_for_backward(patches, wt)
        ctx.geom = (B, C, video.shape[2], video.shape[3], pt, p, D)
        return tok.reshape(B, M // B, D)

    @staticmethod
    def backward(ctx, dtok):
        patches, wt = ctx.saved_tensors
        B, C, T, S, pt, p, D = ctx.geom
        M = patches.shape[0]
        need = _needs(ctx, PatchEmbed)
        dT = hip.cast_rows(dtok.contiguous().reshape(M, D))
        dvideo = dw = db = None
        if need["video"]:
            rows = hip.gemm_nt(dT, wt, hip.EPI_F32)                # [M, Kp] fp32 in patch order
            dvideo = hip.unpatchify(rows, B, C, T, S, pt, p)
        if need["weight"]:
            wg = _WeightGrads()
            dw = wg.add(dT, patches).reshape(D, C, pt, p, p)
            wg.run()
        if need["bias"]:
            db = hip.colsum(dT, rows=M)
        return _grads(ctx, PatchEmbed, video=dvideo, weight=dw, bias=db)


def _pad_cols(t2d, k_to):
    """bf16 copy of a 2-D tensor with the column count zero-padded to k_to (GEMM contraction dims are multiples of 64)"""
    r, k = t2d.shape
    out = _zeros(r, k_to, t2d.device)
    out[:, :k].copy_(t2d)
    return out


class Linear(torch.autograd.Function):
    """nn.Linear under autocast(bf16) for the small projections outside the block stacks (bottleneck in/out_linear,
    models/bottleneck.py:140-164): bf16 operands, fp32 accumulate, output rounded to bf16 (returned in an fp32 tensor)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        hip.require_gpu(x, weight, bias)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).float()
        M, K = x2.shape
        N = weight.shape[0]
        Kp_, Np_ = _pad64(K), _pad64(N)
        xb = _pad_cols(x2, Kp_)
        wb = _pad_cols(weight.detach(), Kp_)                        # [N, Kp]
        y = hip.gemm_nt(xb, wb, hip.EPI_F32, bias=bias, round_bf16=True, out=torch.empty(M, (N + 3) // 4 * 4, device=x.device))
        ctx.save_for_backward(xb, weight)
        ctx.geom = (shp, M, K, N, Np_)
        return y[:, :N].reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xb, weight = ctx.saved_tensors
        shp, M, K, N, Np_ = ctx.geom
        need = _needs(ctx, Linear)
        dyb = _pad_cols(dy.reshape(M, N), Np_)                      # grad of a bf16 output is bf16 under autocast
        dx = dw = db = None
        if need["x"]:
            wt = _pad_cols(weight.detach().t().contiguous(), Np_)   # [K, Np]: B operand of dX = dY . W
            dx = hip.gemm_nt(dyb, wt, hip.EPI_F32, out=torch.empty(M, (K + 3) // 4 * 4, device=dy.device))[:, :K].reshape(shp)
        if need["weight"]:
            wg = _WeightGrads()
            full = wg.add(dyb, xb)                                  # [Np, Kp]
            wg.run()
            dw = full[:N, :K].contiguous()
        if need["bias"]:
            db = hip.colsum(dyb, rows=M)[:N].contiguous()
        return _grads(ctx, Linear, x=dx, weight=dw, bias=db)


class VectorQuantize(torch.autograd.Function):
    """SimpleVectorQuantizer.forward (models/bottleneck.py:262-324).  Returns (regularized_z, indices, loss_q, loss_commit,
    loss_codebook, unregularized_z, emb); gradients flow through regularized_z (straight-through) and the three losses,
    exactly what autograd derives from :292-307; unregularized_z / emb are returned detached."""

    @staticmethod
    def forward(ctx, z, codebook, mode, l2_normalized, inv_tau, beta, codebook_w, seed):
        hip.require_gpu(z, codebook)
        shp = z.shape
        z2 = z.reshape(-1, shp[-1]).float().contiguous()
        o = hip.vq_forward(z2, codebook, mode, l2_normalized=l2_normalized, inv_tau=inv_tau, beta=beta, codebook_w=codebook_w, seed=seed)
        ctx.saved, ctx.cfg, ctx.shp = o, (beta, codebook_w, l2_normalized), shp
        L = o["losses"]
        idx, zn, emb = o["idx"].clone(), o["zn"].reshape(shp).clone(), o["E"].clone()
        ctx.mark_non_differentiable(idx, zn, emb)
        return o["rz"].reshape(shp), idx, L[0].clone(), L[1].clone(), L[2].clone(), zn, emb

    @staticmethod
    def backward(ctx, g_rz, _gi, g_q, g_c, g_cb, _gz, _ge):
        beta, cw, l2n = ctx.cfg
        o = ctx.saved
        dev = o["zn"].device
        gs = torch.stack([t if t is not None else torch.zeros((), device=dev) for t in (g_q, g_c, g_cb)]).float().contiguous()
        g2 = g_rz.reshape(o["zn"].shape).float().contiguous() if g_rz is not None else None
        dz, _, dW = hip.vq_backward(g2, gs, o, beta=beta, codebook_w=cw, l2_normalized=l2n, need_dW=ctx.needs_input_grad[1])
        return dz.reshape(ctx.shp), dW, None, None, None, None, None, None


class KLSample(torch.autograd.Function):
    """SummedKLDivergenceRegularizer.forward (models/bottleneck.py:356-371) on vt_kl_forward / vt_kl_backward: z [B, N, 2d] ->
    (sample, mean [B, N, d], loss_kl 0-dim, noise [B, N, d]); gradients flow through sample, mean and loss_kl into z, the noise is
    returned detached."""

    @staticmethod
    def forward(ctx, z, seed):
        hip.require_gpu(z)
        z = z.float().contiguous()
        mean, sample, noise, loss, _ = hip.kl_forward(z, seed)
        ctx.save_for_backward(z, noise)
        ctx.mark_non_differentiable(noise)
        return sample, mean, loss[0].clone(), noise

    @staticmethod
    def backward(ctx, g_sample, g_mean, g_loss, _gn):
        z, noise = ctx.saved_tensors
        gkl = g_loss.reshape(1) if g_loss is not None else None
        return hip.kl_backward(z, noise, g_sample, g_mean, gkl), None


def codebook_entries(indices, codebook, l2_normalized):
    """get_codebook_entry (bottleneck.py:327-344): rows of the (normalised) codebook; fp32 [*indices.shape, d]"""
    hip.require_gpu(indices, codebook)
    K, d = codebook.shape
    idx = indices.reshape(-1).to(torch.int64).contiguous()
    dev = codebook.device
    E, wn = torch.empty(K, d, device=dev), torch.empty(K, device=dev)
    ws = hip._ws(hip.lib().vt_vq_workspace_bytes(max(idx.numel(), 1), K, d), dev)
    hip.check(hip.lib().vt_vq_prep_codebook(hip.ptr(codebook), K, d, int(l2_normalized), hip.ptr(E), hip.ptr(wn), hip.ptr(ws), hip.stream()), "vt_vq_prep_codebook")
    out = torch.empty(idx.numel(), d, device=dev)
    hip.check(hip.lib().vt_vq_gather(hip.ptr(E), hip.ptr(idx), idx.numel(), K, d, hip.ptr(out), None, 0, hip.stream()), "vt_vq_gather")
    return out.reshape(*indices.shape, d)


class FiniteScalarQuantize(torch.autograd.Function):
    """FSQ.forward (models/model_new/quantizer/fsq.py:119-131): one launch per direction, straight-through gradient."""

    @staticmethod
    def forward(ctx, z, levels):
        zc = z.contiguous()
        codes, idx = hip.fsq_forward(zc, levels)
        ctx.save_for_backward(zc)
        ctx.levels = levels
        ctx.mark_non_differentiable(idx)
        return codes, idx

    @staticmethod
    def backward(ctx, dcodes, _didx):
        (z,) = ctx.saved_tensors
        return hip.fsq_backward(z, dcodes.contiguous().to(z.dtype), ctx.levels), None


class LayerNormRows(torch.autograd.Function):
    """nn.LayerNorm over the last dim on the LayerNorm kernels (fp32 in, statistics in fp32, bf16-rounded output returned in an
    fp32 tensor -- what the Linear that follows reads under autocast).  Widths of vt_layernorm_fwd (128 ... 1024)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        hip.require_gpu(x, weight, bias)
        shp = x.shape
        x2 = x.contiguous().reshape(-1, shp[-1]).float()
        y, mean, rstd = hip.layernorm_fwd(x2, weight, bias, eps)
        ctx.save_for_backward(x2, weight, mean, rstd)
        return y.float().reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, mean, rstd = ctx.saved_tensors
        dyb = hip.cast_rows(dy.contiguous().reshape(x2.shape).float())
        dx, _, dg, db, _ = hip.layernorm_bwd(dyb, x2, weight, mean, rstd, want_dxsum=False)
        return _grads(ctx, LayerNormRows, x=dx.reshape(dy.shape), weight=dg, bias=db)


class Unpatchify(torch.autograd.Function):
    """rows [B * N, C * pt * p * p] in (c, dt, dy, dx) column order -> video [B, C, T, S, S] (the scatter of larp_tokenizer.py:441-454
    once the head's rows are permuted to that order); backward = the patch gather."""

    @staticmethod
    def forward(ctx, rows, geom):
        B, C, T, S, pt, p = geom
        ctx.geom = geom
        return hip.unpatchify(rows.contiguous().float(), B, C, T, S, pt, p)

    @staticmethod
    def backward(ctx, dvideo):
        B, C, T, S, pt, p = ctx.geom
        return hip.patchify(dvideo.contiguous().float(), pt, p).float(), None


class ConvTransposePatch(torch.autograd.Function):
    """nn.ConvTranspose3d(width, C, kernel = stride = (pt, p, p)) on a token grid (blocks.py:116-147): one GEMM into patch
    rows (c, dt, dy, dx) + the LARP path's unpatchify scatter; bf16-rounded output like the conv under autocast."""

    @staticmethod
    def forward(ctx, tok, weight, bias, geom):
        hip.require_gpu(tok, weight, bias)
        B, C, T, S, pt, p = geom
        width = weight.shape[0]
        M = tok.shape[0] * tok.shape[1]
        if M % 64:
            raise hip.HipError("ConvTransposePatch: B * tokens must be a multiple of 64")
        xb = hip.cast_rows(tok.contiguous().reshape(M, width).float())
        wb, wt = _convt_weight(weight)
        rows = _convt_rows(xb, wb, bias, pt * p * p)
        ctx.save_for_backward(xb, wt)
        ctx.geom = geom
        return hip.unpatchify(rows, B, C, T, S, pt, p)

    @staticmethod
    def backward(ctx, dvideo):
        xb, wt = ctx.saved_tensors
        B, C, T, S, pt, p = ctx.geom
        need = _needs(ctx, ConvTransposePatch)
        drows = hip.patchify(dvideo.contiguous().float(), pt, p)              # bf16 [M, Kp], (c, dt, dy, dx) inside a patch
        M, width = xb.shape
        dtok = _convt_input_grad(drows, wt)                                    # [M, width]
        wg = _WeightGrads()
        dw = wg.add(xb, drows, need["weight"])
        wg.run()
        return _grads(ctx, ConvTransposePatch, tok=dtok.reshape(B, M // B, width), weight=_shaped(dw, (width, C, pt, p, p)),
                      bias=_convt_bias_grad(drows, C))


# ------------------------------------------------------------------------------------------------------------------------
# cross attention and model_design's CrossAttention layer (models/model_design/base/transformer.py:92-141)
# ------------------------------------------------------------------------------------------------------------------------
class CrossAttend(torch.autograd.Function):
    """softmax(q k^T / 8) v, head_dim 64, no mask, on vt_attention_cross_*: q a bf16 view [B * Lq, 64 H], k and v bf16 views [B * Lk, 64 H],
    each with a row stride of its own (column blocks of wider projections are read in place) -> o bf16 [B * Lq, 64 H]"""

    @staticmethod
    def forward(ctx, q, k, v, B, Lq, Lk, H):
        o, lse2 = hip.attention_cross_fwd(q, k, v, B, Lq, Lk, H)
        ctx.save_for_backward(q, k, v, o, lse2)
        ctx.geom = (B, Lq, Lk, H)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse2 = ctx.saved_tensors
        dq, dk, dv = hip.attention_cross_bwd(q, k, v, o, dO.contiguous().to(torch.bfloat16), lse2, *ctx.geom)
        return dq, dk, dv, None, None, None, None


class CrossAttentionLayer(torch.autograd.Function):
    """CrossAttention.forward (models/model_design/base/transformer.py:118-141) on x fp32 [B, Lq, D], context fp32 [B, Lk, Dc], D = 64 H,
    as nine launches: rmsnorm_any(x); ONE GEMM on [to_q ; to_gate] (N = 2D); rmsnorm_any(context); the to_kv GEMM; head RMSNorm of q and
    of k; vt_attention_cross_fwd with v read in place from the to_kv output; the gate from columns D..2D of the first GEMM; out_proj.
    Rounding points of autocast(bf16): bf16 Linear outputs, bf16 attention output and gate product, fp32 x / context and input gradients.
    pk_*: (bf16 [N, K], bf16 [K, N]) operand copies of [to_q ; to_gate], to_kv and out_proj (hip.pack_weight)."""

    @staticmethod
    def forward(ctx, x, context, norm_q_w, norm_kv_w, to_q_w, to_kv_w, to_gate_w, q_norm_w, k_norm_w, out_proj_w, H, eps, pk_qg, pk_kv, pk_o):
        hip.require_gpu(x, context, norm_q_w, norm_kv_w, to_q_w, to_kv_w, to_gate_w, q_norm_w, k_norm_w, out_proj_w)
        B, Lq, D = x.shape
        Lk, Dc = context.shape[1], context.shape[2]
        assert context.shape[0] == B and D == 64 * H and to_kv_w.shape == (2 * D, Dc)
        x2 = x.contiguous().reshape(B * Lq, D).float()
        c2 = context.contiguous().reshape(B * Lk, Dc).float()
        nq_w, nkv_w, qn_w, kn_w = (t.detach().float().contiguous() for t in (norm_q_w, norm_kv_w, q_norm_w, k_norm_w))
        xn, rstd_x = hip.rmsnorm_any_fwd(x2, nq_w, eps)
        qg = hip.gemm_nt(xn, pk_qg[0], hip.EPI_BF16)                    # [Mq, 2D] = [to_q xn | to_gate xn]
        cn, rstd_c = hip.rmsnorm_any_fwd(c2, nkv_w, eps)
        kv = hip.gemm_nt(cn, pk_kv[0], hip.EPI_BF16)                    # [Mk, 2D] = [k | v]
        qn = hip.head_rmsnorm_fwd(qg[:, :D], qn_w, eps, H)
        kn = hip.head_rmsnorm_fwd(kv[:, :D], kn_w, eps, H)
        o, lse2 = hip.attention_cross_fwd(qn, kn, kv[:, D:], B, Lq, Lk, H)
        og = hip.sigmoid_gate_cols_fwd(o, qg[:, D:])
        out = hip.gemm_nt(og, pk_o[0], hip.EPI_F32, round_bf16=True)
        ctx.save_for_backward(x2, c2, nq_w, nkv_w, qn_w, kn_w, rstd_x, rstd_c, xn, cn, qg, kv, qn, kn, o, lse2, og, pk_qg[1], pk_kv[1], pk_o[1])
        ctx.geom = (B, Lq, Lk, D, Dc, H, eps)
        return out.reshape(B, Lq, D)

    @staticmethod
    def backward(ctx, dout):
        x2, c2, nq_w, nkv_w, qn_w, kn_w, rstd_x, rstd_c, xn, cn, qg, kv, qn, kn, o, lse2, og, wqg_t, wkv_t, wo_t = ctx.saved_tensors
        B, Lq, Lk, D, Dc, H, eps = ctx.geom
        Mq, Mk = B * Lq, B * Lk
        dev = dout.device
        need = _needs(ctx, CrossAttentionLayer)
        gb = hip.cast_rows(dout.contiguous().reshape(Mq, D).float())
        dog = hip.gemm_nt(gb, wo_t, hip.EPI_BF16)
        dqg = torch.empty(Mq, 2 * D, device=dev, dtype=torch.bfloat16)   # gradient of [q | gate], every column written below
        dkv = torch.empty(Mk, 2 * D, device=dev, dtype=torch.bfloat16)   # gradient of [k | v]
        d_o = hip.sigmoid_gate_cols_bwd(dog, o, qg[:, D:], dqg[:, D:])
        dqn, _, _ = hip.attention_cross_bwd(qn, kn, kv[:, D:], o, d_o, lse2, B, Lq, Lk, H, dk=dkv[:, :D], dv=dkv[:, D:])
        _, dqn_w = hip.head_rmsnorm_bwd(dqn, qg[:, :D], qn_w, eps, H, dx=dqg[:, :D])
        _, dkn_w = hip.head_rmsnorm_bwd(dkv[:, :D], kv[:, :D], kn_w, eps, H, dx=dkv[:, :D])      # in place
        dxn = hip.gemm_nt(dqg, wqg_t, hip.EPI_BF16)
        dcn = hip.gemm_nt(dkv, wkv_t, hip.EPI_BF16)
        wg = _WeightGrads()
        dwq, dwg = _split_rows(wg.add(dqg, xn, need["to_q_w"] or need["to_gate_w"]), D)
        dwkv = wg.add(dkv, cn, need["to_kv_w"])
        dwo = wg.add(gb, og, need["out_proj_w"])
        wg.run()
        dx, _, dnq_w = hip.rmsnorm_any_bwd(dxn, x2, nq_w, rstd_x)
        dc, _, dnkv_w = hip.rmsnorm_any_bwd(dcn, c2, nkv_w, rstd_c)
        return _grads(ctx, CrossAttentionLayer, x=dx.reshape(B, Lq, D), context=dc.reshape(B, Lk, Dc), norm_q_w=dnq_w, norm_kv_w=dnkv_w, to_q_w=dwq,
                      to_kv_w=dwkv, to_gate_w=dwg, q_norm_w=dqn_w, k_norm_w=dkn_w, out_proj_w=dwo)


# ------------------------------------------------------------------------------------------------------------------------
# model_design's self-attention block and stack (models/model_design/base/transformer.py:30-85, 148-216)
# ------------------------------------------------------------------------------------------------------------------------
class ResidualScale(torch.autograd.Function):
    """x + res_scale * y (transformer.py:176-183) on vt_residual_scale_*: x fp32 [..., D], y fp32 of the same shape holding the bf16 values
    a layer returned, res_scale a 0-dim fp32 parameter read on the device.  torch forms res_scale * y in bf16 (the scale converted to bf16, one
    rounding of the product) and adds the fp32 x after; the gradient of the scale is the fp32 sum of bf16(dout) * y in a fixed order."""

    @staticmethod
    def forward(ctx, x, y, scale):
        hip.require_gpu(x, y, scale)
        D = x.shape[-1]
        x2 = x.contiguous().reshape(-1, D).float()
        y2 = y.contiguous().reshape(-1, D).float()
        s = scale.detach().float()
        out = hip.residual_scale_fwd(x2, y2, s)
        ctx.save_for_backward(y2, s)
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, dout):
        y2, s = ctx.saved_tensors
        d2 = dout.contiguous().reshape(y2.shape).float()
        dy, ds = hip.residual_scale_bwd(d2, y2, s, want_ds=_needs(ctx, ResidualScale)["scale"])
        return _grads(ctx, ResidualScale, x=dout, y=dy.reshape(dout.shape), scale=ds)


class RMSNormRows(torch.autograd.Function):
    """RMSNorm (transformer.py:18-27; models/norm.py:6-17) of rows that a bf16 Linear reads next: fp32 in, the bf16-rounded output returned in an
    fp32 tensor.  `family` names the pair of hip wrappers, i.e. the entry-point family of vt_rmsnorm.hip: "rmsnorm_any" (cond_adapter.0 of the
    design's decoder) or "rmsnorm" (the llama-abs widths only: the norms of larp_ar)."""

    @staticmethod
    def forward(ctx, x, weight, eps, family):
        hip.require_gpu(x, weight)
        x2 = x.contiguous().reshape(-1, x.shape[-1]).float()
        w = weight.detach().float().contiguous()
        y, rstd = getattr(hip, family + "_fwd")(x2, w, eps)
        ctx.save_for_backward(x2, w, rstd)
        ctx.family = family
        return y.float().reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rstd = ctx.saved_tensors
        dx, _, dw = getattr(hip, ctx.family + "_bwd")(hip.cast_rows(dy.contiguous().reshape(x2.shape).float()), x2, w, rstd)
        return _grads(ctx, RMSNormRows, x=dx.reshape(dy.shape), weight=dw)


class RMSNormF32(torch.autograd.Function):
    """final_norm of the stack (transformer.py:211, 216): RMSNorm of the fp32 residual stream with an fp32, unrounded output (vt_rmsnorm_any_f32_*)"""

    @staticmethod
    def forward(ctx, x, weight, eps):
        hip.require_gpu(x, weight)
        x2 = x.contiguous().reshape(-1, x.shape[-1]).float()
        w = weight.detach().float().contiguous()
        y, rstd = hip.rmsnorm_any_f32_fwd(x2, w, eps)
        ctx.save_for_backward(x2, w, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rstd = ctx.saved_tensors
        dx, dw = hip.rmsnorm_any_f32_bwd(dy.contiguous().reshape(x2.shape).float(), x2, w, rstd)
        return _grads(ctx, RMSNormF32, x=dx.reshape(dy.shape), weight=dw)


class SelfAttentionLayer(torch.autograd.Function):
    """x + res_scale * SelfAttention(x) (transformer.py:67-85, 176) on x fp32 [B, L, D], D = 64 H, as seven launches: rmsnorm_any(x); ONE GEMM on
    [to_qkv ; to_gate] (N = 4D, columns q | k | v | gate); vt_qkrms_rope_fwd (head RMSNorm and rotation of q and k, v copied, into the packed
    attention operand); vt_attention_fwd; the gate from columns 3D..4D; out_proj; vt_residual_scale_fwd.  Rounding points of autocast(bf16):
    bf16 Linear outputs, bf16 head norm, rotation, attention output and gate product, the residual product in bf16, fp32 x and dx.
    pk_*: (bf16 [N, K], bf16 [K, N]) operand copies of [to_qkv ; to_gate] and out_proj (hip.pack_weight)."""

    @staticmethod
    def forward(ctx, x, cos, sin, res_scale, norm_w, to_qkv_w, to_gate_w, q_norm_w, k_norm_w, out_proj_w, H, eps, pk_qkvg, pk_o):
        hip.require_gpu(x, cos, sin, res_scale, norm_w, to_qkv_w, to_gate_w, q_norm_w, k_norm_w, out_proj_w)
        B, L, D = x.shape
        assert D == 64 * H and to_qkv_w.shape == (3 * D, D) and cos.shape == (L, 32) == sin.shape
        M = B * L
        x2 = x.contiguous().reshape(M, D).float()
        n_w, qn_w, kn_w, s = (t.detach().float().contiguous() for t in (norm_w, q_norm_w, k_norm_w, res_scale))
        cos, sin = cos.contiguous(), sin.contiguous()
        xn, rstd = hip.rmsnorm_any_fwd(x2, n_w, eps)
        qkvg = hip.gemm_nt(xn, pk_qkvg[0], hip.EPI_BF16)                 # [M, 4D] = [q | k | v | gate]
        qkv = hip.qkrms_rope_fwd(qkvg, L, H, qn_w, kn_w, eps, cos, sin)
        o, lse2 = hip.attention_fwd(qkv, B, L, H)
        og = hip.sigmoid_gate_fwd(o, qkvg)
        y = hip.gemm_nt(og, pk_o[0], hip.EPI_F32, round_bf16=True)
        out = hip.residual_scale_fwd(x2, y, s)
        ctx.save_for_backward(x2, n_w, qn_w, kn_w, s, cos, sin, rstd, xn, qkvg, qkv, o, lse2, og, y, pk_qkvg[1], pk_o[1])
        ctx.geom = (B, L, D, H, eps)
        return out.reshape(B, L, D)

    @staticmethod
    def backward(ctx, dout):
        x2, n_w, qn_w, kn_w, s, cos, sin, rstd, xn, qkvg, qkv, o, lse2, og, y, wqkvg_t, wo_t = ctx.saved_tensors
        B, L, D, H, eps = ctx.geom
        M = B * L
        need = _needs(ctx, SelfAttentionLayer)
        d2 = dout.contiguous().reshape(M, D).float()
        dy, ds = hip.residual_scale_bwd(d2, y, s, want_ds=need["res_scale"])
        gb = hip.cast_rows(dy)                                           # exact: dy holds bf16 values
        dog = hip.gemm_nt(gb, wo_t, hip.EPI_BF16)
        dqkvg = torch.empty(M, 4 * D, device=dout.device, dtype=torch.bfloat16)  # gradient of [q | k | v | gate], every column written below
        d_o = hip.sigmoid_gate_bwd(dog, o, qkvg, dqkvg)
        dqkv = hip.attention_bwd(qkv, o, d_o, lse2, B, L, H)
        dqn_w, dkn_w = hip.qkrms_rope_bwd(qkvg, dqkv, L, H, qn_w, kn_w, eps, cos, sin, dqkvg, want_dw=need["q_norm_w"] or need["k_norm_w"])
        dxn = hip.gemm_nt(dqkvg, wqkvg_t, hip.EPI_BF16)                  # the gradients from to_qkv and to_gate summed in fp32, rounded once
        wg = _WeightGrads()
        dwqkv, dwg = _split_rows(wg.add(dqkvg, xn, need["to_qkv_w"] or need["to_gate_w"]), 3 * D)
        dwo = wg.add(gb, og, need["out_proj_w"])
        wg.run()
        dx, _, dn_w = hip.rmsnorm_any_bwd(dxn, x2, n_w, rstd, dres=d2)   # + the residual path's gradient
        return _grads(ctx, SelfAttentionLayer, x=dx.reshape(B, L, D), res_scale=ds, norm_w=dn_w, to_qkv_w=dwqkv, to_gate_w=dwg, q_norm_w=dqn_w,
                      k_norm_w=dkn_w, out_proj_w=dwo)


class FeedForwardLayer(torch.autograd.Function):
    """x + res_scale * ffn(x) with ffn = make_ffn (transformer.py:30-39, 183): rmsnorm_any(x); the fc1 GEMM (N = 2 inner); vt_geglu_fwd into an
    operand whose row stride is padded to a multiple of 64 (inner is 1376 at width 512); the fc2 GEMM; vt_residual_scale_fwd.
    pk_1: operand copies of ffn.1; pk_2: of ffn.3 with the contraction dim padded to that multiple (pack_weight(k_pad=))."""

    @staticmethod
    def forward(ctx, x, res_scale, norm_w, fc1_w, fc2_w, eps, pk_1, pk_2):
        hip.require_gpu(x, res_scale, norm_w, fc1_w, fc2_w)
        shp = x.shape
        D = shp[-1]
        inner = fc2_w.shape[1]
        assert fc1_w.shape == (2 * inner, D) and fc2_w.shape[0] == D
        x2 = x.contiguous().reshape(-1, D).float()
        n_w, s = norm_w.detach().float().contiguous(), res_scale.detach().float()
        xn, rstd = hip.rmsnorm_any_fwd(x2, n_w, eps)
        h = hip.gemm_nt(xn, pk_1[0], hip.EPI_BF16)                      # [M, 2 inner] = [x | gate]
        a = hip.geglu_fwd(h, lda=_pad64(inner))
        y = hip.gemm_nt(a, pk_2[0], hip.EPI_F32, round_bf16=True)
        out = hip.residual_scale_fwd(x2, y, s)
        ctx.save_for_backward(x2, n_w, s, rstd, xn, h, a, y, pk_1[1], pk_2[1])
        ctx.inner = inner
        return out.reshape(shp)

    @staticmethod
    def backward(ctx, dout):
        x2, n_w, s, rstd, xn, h, a, y, w1_t, w2_t = ctx.saved_tensors
        M, D = x2.shape
        need = _needs(ctx, FeedForwardLayer)
        d2 = dout.contiguous().reshape(M, D).float()
        dy, ds = hip.residual_scale_bwd(d2, y, s, want_ds=need["res_scale"])
        gb = hip.cast_rows(dy)
        da = hip.gemm_nt(gb, w2_t, hip.EPI_BF16)                        # [M, pad64(inner)]
        dh = hip.geglu_bwd(da, h)
        dxn = hip.gemm_nt(dh, w1_t, hip.EPI_BF16)
        wg = _WeightGrads()
        dw1 = wg.add(dh, xn, need["fc1_w"])
        dw2p = wg.add(gb, a, need["fc2_w"])                             # [D, pad64(inner)]
        wg.run()
        dw2 = dw2p[:, :ctx.inner].contiguous() if need["fc2_w"] else None
        dx, _, dn_w = hip.rmsnorm_any_bwd(dxn, x2, n_w, rstd, dres=d2)
        return _grads(ctx, FeedForwardLayer, x=dx.reshape(dout.shape), res_scale=ds, norm_w=dn_w, fc1_w=dw1, fc2_w=dw2)


# ------------------------------------------------------------------------------------------------------------------------
# packed variable-length attention with grouped KV heads and model_titok's Attn layer (models/model_titok/base/transformer.py:32-62)
# ------------------------------------------------------------------------------------------------------------------------
class VarlenAttend(torch.autograd.Function):
    """flash_attn_varlen_func(q, k, v, cu_seqlens, cu_seqlens, ...) on vt_attention_varlen_*: head_dim 64, no mask, scale 1/8.  q a bf16 view
    [M, 64 Hq], k and v bf16 views [M, 64 Hkv] with a row stride each (the column blocks of one projection are read in place), sequence b =
    rows cu_seqlens[b] .. cu_seqlens[b+1]-1, query head h on KV head h // (Hq // Hkv) -> o bf16 [M, 64 Hq].  cu_seqlens: a list, or a CPU or
    device int tensor (a device tensor costs one synchronisation per call, forward and backward share the read)."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, Hq, Hkv):
        cu = hip.cu_seqlens_list(cu_seqlens)                             # the one conversion: backward reuses the list
        o, lse2 = hip.attention_varlen_fwd(q, k, v, cu, Hq, Hkv)
        ctx.save_for_backward(q, k, v, o, lse2)
        ctx.geom = (cu, Hq, Hkv)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse2 = ctx.saved_tensors
        dq, dk, dv = hip.attention_varlen_bwd(q, k, v, o, dO.contiguous().to(torch.bfloat16), lse2, *ctx.geom)
        return dq, dk, dv, None, None, None


class VarlenAttentionLayer(torch.autograd.Function):
    """Attn.forward (models/model_titok/base/transformer.py:46-62) on a packed batch x fp32 [M, D], D = 64 Hq, as five launches: LayerNorm(x);
    the to_qkv GEMM (N = D + 128 Hkv, columns q | k | v); vt_qknorm_rope_gqa_fwd (per-head LayerNorm and rotation of q and k by table row m, v
    copied); vt_attention_varlen_fwd on the three column blocks in place; out_proj.  Rounding points of autocast(bf16): bf16 Linear outputs,
    bf16 head norm and rotation, bf16 attention output, fp32 x and dx.  cos / sin: fp32 [M, 32] device tables (varlen.rope_freqs); cu: the
    sequence boundaries as a host list.  pk_*: (bf16 [N, K], bf16 [K, N]) operand copies of to_qkv and out_proj (packs.get)."""

    @staticmethod
    def forward(ctx, x, cos, sin, cu, pre_w, pre_b, to_qkv_w, q_w, q_b, k_w, k_b, out_proj_w, Hq, Hkv, eps, pk_qkv, pk_o):
        hip.require_gpu(x, cos, sin, pre_w, pre_b, to_qkv_w, q_w, q_b, k_w, k_b, out_proj_w)
        M, D = x.shape
        G = 64 * Hkv
        assert D == 64 * Hq and to_qkv_w.shape == (D + 2 * G, D) and cos.shape == (M, 32) == sin.shape
        x2 = x.contiguous().float()
        pw, pb, qw, qb, kw, kb = (t.detach().float().contiguous() for t in (pre_w, pre_b, q_w, q_b, k_w, k_b))
        cos, sin = cos.contiguous(), sin.contiguous()
        xn, mean, rstd = hip.layernorm_fwd(x2, pw, pb, eps)
        qkv = hip.gemm_nt(xn, pk_qkv[0], hip.EPI_BF16)                   # [M, D + 2G] = [q | k | v]
        qkr = hip.qknorm_rope_gqa_fwd(qkv, Hq, Hkv, qw, qb, kw, kb, eps, cos, sin)
        o, lse2 = hip.attention_varlen_fwd(qkr[:, :D], qkr[:, D:D + G], qkr[:, D + G:], cu, Hq, Hkv)
        out = hip.gemm_nt(o, pk_o[0], hip.EPI_F32, round_bf16=True)
        ctx.save_for_backward(x2, pw, qw, kw, cos, sin, mean, rstd, xn, qkv, qkr, o, lse2, pk_qkv[1], pk_o[1])
        ctx.geom = (list(cu), Hq, Hkv, eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, pw, qw, kw, cos, sin, mean, rstd, xn, qkv, qkr, o, lse2, wqkv_t, wo_t = ctx.saved_tensors
        cu, Hq, Hkv, eps = ctx.geom
        M, D = x2.shape
        G = 64 * Hkv
        need = _needs(ctx, VarlenAttentionLayer)
        gb = hip.cast_rows(dout.contiguous().float())
        d_o = hip.gemm_nt(gb, wo_t, hip.EPI_BF16)
        dqkr = torch.empty(M, D + 2 * G, device=dout.device, dtype=torch.bfloat16)  # gradient of the rotated [q | k | v], every column written below
        hip.attention_varlen_bwd(qkr[:, :D], qkr[:, D:D + G], qkr[:, D + G:], o, d_o, lse2, cu, Hq, Hkv, dq=dqkr[:, :D], dk=dqkr[:, D:D + G],
                                 dv=dqkr[:, D + G:])
        dqkv, (dq_w, dq_b, dk_w, dk_b) = hip.qknorm_rope_gqa_bwd(qkv, dqkr, Hq, Hkv, qw, kw, eps, cos, sin)
        dxn = hip.gemm_nt(dqkv, wqkv_t, hip.EPI_BF16)
        wg = _WeightGrads()
        dwqkv = wg.add(dqkv, xn, need["to_qkv_w"])
        dwo = wg.add(gb, o, need["out_proj_w"])
        wg.run()
        dx, _, dg, db, _ = hip.layernorm_bwd(dxn, x2, pw, mean, rstd, want_dxsum=False, want_dxb=False)
        return _grads(ctx, VarlenAttentionLayer, x=dx, pre_w=dg, pre_b=db, to_qkv_w=dwqkv, q_w=dq_w, q_b=dq_b, k_w=dk_w, k_b=dk_b, out_proj_w=dwo)


# ------------------------------------------------------------------------------------------------------------------------
# the packed `titok` model (models/model_titok/base/blocks.py:82-222): clips of different sizes, [lead | tail] sequences, its blocks
# ------------------------------------------------------------------------------------------------------------------------
class PatchRowsClips(torch.autograd.Function):
    """A list of fp32 clips [C, T_b, H_b, W_b] -> bf16 patch rows [sum_b G_b, C pt p p], clip after clip (the rearrange + cat of
    blocks.py:128-129, rounded as the Linear that follows reads it under autocast): ONE vt_patchify_clips launch; backward = ONE
    vt_unpatchify_clips launch.  (The clips are a variable argument list, so the gradients go back by position, as BlockStack's do.)"""

    @staticmethod
    def forward(ctx, pt, p, *clips):
        clips = [v.contiguous().float() for v in clips]
        ctx.geom = (pt, p, clips[0].shape[0] if clips else 0, [tuple(v.shape[1:]) for v in clips])
        return hip.patchify_clips(clips, pt, p)

    @staticmethod
    def backward(ctx, drows):
        pt, p, C, sizes = ctx.geom
        dclips = hip.unpatchify_clips(drows.contiguous().float(), sizes, C, pt, p)
        return (None, None, *[g if n else None for g, n in zip(dclips, ctx.needs_input_grad[2:])])


class UnpatchifyClips(torch.autograd.Function):
    """fp32 rows [sum_b G_b, C pt p p] in (c, dt, dy, dx) column order -> a tuple of fp32 clips [C, T_b, H_b, W_b], sizes = ((T_b, H_b, W_b), ...)
    (the split + rearrange of blocks.py:212-220): ONE vt_unpatchify_clips launch; backward = ONE vt_patchify_clips launch over the list of
    d clips (a clip without a gradient counts as zeros)."""

    @staticmethod
    def forward(ctx, rows, sizes, C, pt, p):
        ctx.geom = (tuple(tuple(int(v) for v in s) for s in sizes), C, pt, p)
        return tuple(hip.unpatchify_clips(rows.contiguous().float(), ctx.geom[0], C, pt, p))

    @staticmethod
    def backward(ctx, *dclips):
        sizes, C, pt, p = ctx.geom
        dev = next(g for g in dclips if g is not None).device
        full = [g.contiguous().float() if g is not None else torch.zeros(C, *s, device=dev) for g, s in zip(dclips, sizes)]
        return _grads(ctx, UnpatchifyClips, rows=hip.patchify_clips(full, pt, p).float())


class PackedScatter(torch.autograd.Function):
    """The packed residual stream fp32 [M, D] of blocks.py:132-135 / :197-200: sequence b = rows cu[b] .. cu[b+1]-1 = [lead[b] lead rows |
    tail rows]; the `which` segments (hip.PACKED_LEAD / PACKED_TAIL) take the rows of the compact src, the other segments every row = vec
    (mask_token [1, D]).  Backward: d src = PackedGather of the same segments, d vec = vt_packed_segment_colsum of the other ones."""

    @staticmethod
    def forward(ctx, src, vec, cu, lead, which):
        ctx.geom = (hip.cu_seqlens_list(cu), [int(v) for v in lead], which, vec.shape)
        return hip.packed_scatter(src.contiguous().float(), ctx.geom[0], ctx.geom[1], which, vec=vec.detach().contiguous().float())

    @staticmethod
    def backward(ctx, dout):
        cu, lead, which, vshape = ctx.geom
        need = _needs(ctx, PackedScatter)
        d = dout.contiguous().float()
        dsrc = hip.packed_gather(d, cu, lead, which) if need["src"] else None
        dvec = hip.packed_segment_colsum(d, cu, lead, 1 - which).reshape(vshape) if need["vec"] else None
        return _grads(ctx, PackedScatter, src=dsrc, vec=dvec)


class PackedGather(torch.autograd.Function):
    """The `which` segments' rows of a packed fp32 [M, D], compact (blocks.py:140-142: the latent rows; :207-209: the grid rows).
    Backward: PackedScatter with zeros in the other segments."""

    @staticmethod
    def forward(ctx, packed, cu, lead, which):
        ctx.geom = (hip.cu_seqlens_list(cu), [int(v) for v in lead], which)
        return hip.packed_gather(packed.contiguous().float(), *ctx.geom)

    @staticmethod
    def backward(ctx, dout):
        cu, lead, which = ctx.geom
        return _grads(ctx, PackedGather, packed=hip.packed_scatter(dout.contiguous().float(), cu, lead, which))


class VarlenAttentionResidualLayer(torch.autograd.Function):
    """x + Attn(x) (models/model_titok/base/transformer.py:83): VarlenAttentionLayer's five launches with the residual in the out_proj GEMM's
    epilogue, which rounds the product to bf16 first and adds the fp32 x second -- bit for bit x + VarlenAttentionLayer(x).  Same arguments in
    the same order, so the backward IS VarlenAttentionLayer's (it reads ctx only), plus dout on the residual path."""

    @staticmethod
    def forward(ctx, x, cos, sin, cu, pre_w, pre_b, to_qkv_w, q_w, q_b, k_w, k_b, out_proj_w, Hq, Hkv, eps, pk_qkv, pk_o):
        hip.require_gpu(x, cos, sin, pre_w, pre_b, to_qkv_w, q_w, q_b, k_w, k_b, out_proj_w)
        M, D = x.shape
        G = 64 * Hkv
        assert D == 64 * Hq and to_qkv_w.shape == (D + 2 * G, D) and cos.shape == (M, 32) == sin.shape
        x2 = x.contiguous().float()
        pw, pb, qw, qb, kw, kb = (t.detach().float().contiguous() for t in (pre_w, pre_b, q_w, q_b, k_w, k_b))
        cos, sin = cos.contiguous(), sin.contiguous()
        xn, mean, rstd = hip.layernorm_fwd(x2, pw, pb, eps)
        qkv = hip.gemm_nt(xn, pk_qkv[0], hip.EPI_BF16)
        qkr = hip.qknorm_rope_gqa_fwd(qkv, Hq, Hkv, qw, qb, kw, kb, eps, cos, sin)
        o, lse2 = hip.attention_varlen_fwd(qkr[:, :D], qkr[:, D:D + G], qkr[:, D + G:], cu, Hq, Hkv)
        out = hip.gemm_nt(o, pk_o[0], hip.EPI_F32, residual=x2, round_bf16=True)
        ctx.save_for_backward(x2, pw, qw, kw, cos, sin, mean, rstd, xn, qkv, qkr, o, lse2, pk_qkv[1], pk_o[1])
        ctx.geom = (list(cu), Hq, Hkv, eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        grads = VarlenAttentionLayer.backward(ctx, dout)
        return (grads[0] + dout if grads[0] is not None else None, *grads[1:])


class VarlenFeedForwardLayer(torch.autograd.Function):
    """ffd(x) of models/model_titok/base/transformer.py:20-30 on x fp32 [M, D], and with residual=True x + ffd(x) (:84): LayerNorm(x); the first
    Linear (N = 2 inner, columns x | gate); vt_geglu_fwd into an operand whose row stride is padded to a multiple of 64 (inner is 352 at width
    128, 1376 at 512); the second Linear, whose epilogue rounds to bf16 first and adds the fp32 x second -- bit for bit x + ffd(x).  No gate and
    no stream rescale.  pk_1: operand copies of the first Linear; pk_2: of the second with the contraction dim padded (packs.get(k_pad=))."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, fc1_w, fc2_w, eps, residual, pk_1, pk_2):
        hip.require_gpu(x, ln_w, ln_b, fc1_w, fc2_w)
        M, D = x.shape
        inner = fc2_w.shape[1]
        assert fc1_w.shape == (2 * inner, D) and fc2_w.shape[0] == D
        x2 = x.contiguous().float()
        w, b = ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous()
        xn, mean, rstd = hip.layernorm_fwd(x2, w, b, eps)
        h = hip.gemm_nt(xn, pk_1[0], hip.EPI_BF16)                      # [M, 2 inner] = [x | gate]
        a = hip.geglu_fwd(h, lda=_pad64(inner))
        out = hip.gemm_nt(a, pk_2[0], hip.EPI_F32, residual=x2 if residual else None, round_bf16=True)
        ctx.save_for_backward(x2, w, mean, rstd, xn, h, a, pk_1[1], pk_2[1])
        ctx.geom = (inner, residual)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, w, mean, rstd, xn, h, a, w1_t, w2_t = ctx.saved_tensors
        inner, residual = ctx.geom
        need = _needs(ctx, VarlenFeedForwardLayer)
        d2 = dout.contiguous().float()
        gb = hip.cast_rows(d2)
        da = hip.gemm_nt(gb, w2_t, hip.EPI_BF16)                        # [M, pad64(inner)]
        dh = hip.geglu_bwd(da, h)
        dxn = hip.gemm_nt(dh, w1_t, hip.EPI_BF16)
        wg = _WeightGrads()
        dw1 = wg.add(dh, xn, need["fc1_w"])
        dw2p = wg.add(gb, a, need["fc2_w"])                             # [D, pad64(inner)]
        wg.run()
        dw2 = dw2p[:, :inner].contiguous() if need["fc2_w"] else None
        dx, _, dg, db, _ = hip.layernorm_bwd(dxn, x2, w, mean, rstd, dres=d2 if residual else None, want_dxsum=False, want_dxb=False)
        return _grads(ctx, VarlenFeedForwardLayer, x=dx, ln_w=dg, ln_b=db, fc1_w=dw1, fc2_w=dw2)


# ------------------------------------------------------------------------------------------------------------------------
# `autoencoder_dualpatch` (models/model_dualpatch/base/blocks.py:12-258): a clip cut along time into two segments with a patch size each
# ------------------------------------------------------------------------------------------------------------------------
def _dual_maps(lead, n0, n1, L):
    """the row maps of the two patch segments in a [B, L, D] stream [lead rows | n0 first-segment rows | n1 rest rows]"""
    return hip.RowMap(n0, L, lead), hip.RowMap(n1, L, lead + n0)


class DualPatchEmbed(torch.autograd.Function):
    """Encoder.forward up to the layer stack (blocks.py:99-120): frames [0, T0) through Conv3d(kernel = stride = (pt0, ph, pw)) + pos0, frames
    [T0, T) through Conv3d((pt1, ph, pw)) + pos1, behind `lead` rows of lead_table (latent_queries, broadcast over the batch) -> the residual
    stream fp32 [B, lead + N0 + N1, D].  ONE vt_patchify_dual, two GEMMs whose epilogues round the conv output to bf16, add the fp32 position
    table and write their rows into the stream through an output row map, ONE vt_assemble_rows for the lead rows: no slice copy of the video and
    no torch.cat.  w0 [D, C, pt0, ph, pw], w1 [D, C, pt1, ph, pw], pos0 [1, N0, D], pos1 [1, N1, D], lead_table [1, lead, D]; T0 follows from N0.
    Backward: vt_cast_rows per segment through the same maps, both weight gradients in one grouped launch, vt_colsum for the biases,
    vt_batch_sum through a map for the three tables, and for d video two input-gradient GEMMs + ONE vt_unpatchify_dual."""

    @staticmethod
    def forward(ctx, video, w0, b0, pos0, w1, b1, pos1, lead, lead_table):
        hip.require_gpu(video, w0, b0, pos0, w1, b1, pos1, lead_table)
        D, C, pt0, ph, pw = w0.shape
        pt1 = w1.shape[2]
        B, _, T, H, W = video.shape
        assert video.shape[1] == C and w1.shape == (D, C, pt1, ph, pw) and H % ph == 0 and W % pw == 0
        n0 = pos0.numel() // D
        T0 = n0 // ((H // ph) * (W // pw)) * pt0
        n1 = hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)[1]
        assert hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)[0] == n0 and pos1.numel() == n1 * D and lead_table.numel() == lead * D
        L = lead + n0 + n1
        video = video.contiguous().float()
        rows0, rows1 = hip.patchify_dual(video, T0, pt0, pt1, ph, pw)          # bf16, (c, dt, dy, dx) inside a patch
        (wb0, wt0), (wb1, wt1) = hip.pack_weight(w0), hip.pack_weight(w1)
        out = torch.empty(B, L, D, device=video.device)
        o2 = out.view(B * L, D)
        m0, m1 = _dual_maps(lead, n0, n1, L)
        _conv_tokens(rows0, wb0, b0, pos0, n0, omap=m0, out=o2)
        _conv_tokens(rows1, wb1, b1, pos1, n1, omap=m1, out=o2)
        hip.assemble_rows(o2, L, 0, B, lead, table=_f32(lead_table.reshape(lead, D)))
        ctx.save_for_backward(rows0, rows1, wt0, wt1)
        ctx.geom = (B, C, T, H, W, T0, pt0, pt1, ph, pw, D, lead, n0, n1)
        ctx.shapes = (w0.shape, w1.shape, pos0.shape, pos1.shape, lead_table.shape)
        return out

    @staticmethod
    def backward(ctx, dtok):
        rows0, rows1, wt0, wt1 = ctx.saved_tensors
        B, C, T, H, W, T0, pt0, pt1, ph, pw, D, lead, n0, n1 = ctx.geom
        L = lead + n0 + n1
        need = _needs(ctx, DualPatchEmbed)
        d2 = dtok.contiguous().float().view(B * L, D)
        m0, m1 = _dual_maps(lead, n0, n1, L)
        dT0 = hip.cast_rows(d2, rows=B * n0, rmap=m0)                          # the conv outputs are bf16 under autocast: so are their gradients
        dT1 = hip.cast_rows(d2, rows=B * n1, rmap=m1)
        dvideo = None
        if need["video"]:
            dvideo = hip.unpatchify_dual(hip.gemm_nt(dT0, wt0, hip.EPI_F32), hip.gemm_nt(dT1, wt1, hip.EPI_F32), B, C, T, H, W, T0, pt0, pt1, ph, pw)
        wg = _WeightGrads()
        dw0, dw1 = wg.add(dT0, rows0, need["w0"]), wg.add(dT1, rows1, need["w1"])
        wg.run()
        sw0, sw1, sp0, sp1, slt = ctx.shapes
        return _grads(ctx, DualPatchEmbed, video=dvideo, w0=_shaped(dw0, sw0), w1=_shaped(dw1, sw1),
                      b0=hip.colsum(dT0, rows=B * n0) if need["b0"] else None, b1=hip.colsum(dT1, rows=B * n1) if need["b1"] else None,
                      pos0=hip.batch_sum(d2, B, n0, rmap=m0).reshape(sp0) if need["pos0"] else None,
                      pos1=hip.batch_sum(d2, B, n1, rmap=m1).reshape(sp1) if need["pos1"] else None,
                      lead_table=hip.batch_sum(d2, B, lead, rmap=hip.RowMap(lead, L, 0)).reshape(slt) if need["lead_table"] else None)


class DualConvTransposePatch(torch.autograd.Function):
    """Decoder.forward behind the layer stack (blocks.py:234-257): rows [lead, lead + N0) of every sequence of `stream` fp32 [B, L, D] through
    ConvTranspose3d(D, C, kernel = stride = (pt0, ph, pw)) into frames [0, T0), the N1 rows behind them through ConvTranspose3d((pt1, ph, pw))
    into frames [T0, T): vt_cast_rows per segment through a row map, two GEMMs into patch rows (c, dt, dy, dx) rounded to bf16 like the convs
    under autocast, ONE vt_unpatchify_dual (no torch.cat of two videos).  geom = (B, C, T, H, W, T0, pt0, pt1, ph, pw).
    Backward: ONE vt_patchify_dual of d video (bf16 rows, as ConvTransposePatch), two input-gradient GEMMs written into d stream through
    the row maps, vt_zero_rows for the lead rows (nothing reads the stack's latent rows), grouped weight gradients, vt_colsum for the biases."""

    @staticmethod
    def forward(ctx, stream, lead, w0, b0, w1, b1, geom):
        hip.require_gpu(stream, w0, b0, w1, b1)
        B, C, T, H, W, T0, pt0, pt1, ph, pw = geom
        D = w0.shape[0]
        n0, n1 = hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)
        L = lead + n0 + n1
        assert stream.shape == (B, L, D) and w0.shape == (D, C, pt0, ph, pw) and w1.shape == (D, C, pt1, ph, pw)
        s2 = stream.contiguous().float().view(B * L, D)
        m0, m1 = _dual_maps(lead, n0, n1, L)
        x0, x1 = hip.cast_rows(s2, rows=B * n0, rmap=m0), hip.cast_rows(s2, rows=B * n1, rmap=m1)
        (wb0, wt0), (wb1, wt1) = _convt_weight(w0), _convt_weight(w1)
        r0, r1 = _convt_rows(x0, wb0, b0, pt0 * ph * pw), _convt_rows(x1, wb1, b1, pt1 * ph * pw)
        ctx.save_for_backward(x0, x1, wt0, wt1)
        ctx.geom, ctx.lead = geom, lead
        return hip.unpatchify_dual(r0, r1, B, C, T, H, W, T0, pt0, pt1, ph, pw)

    @staticmethod
    def backward(ctx, dvideo):
        x0, x1, wt0, wt1 = ctx.saved_tensors
        B, C, T, H, W, T0, pt0, pt1, ph, pw = ctx.geom
        lead, D = ctx.lead, x0.shape[1]
        n0, n1 = hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)
        L = lead + n0 + n1
        need = _needs(ctx, DualConvTransposePatch)
        dr0, dr1 = hip.patchify_dual(dvideo.contiguous().float(), T0, pt0, pt1, ph, pw)      # bf16 [B * N, Kp]
        dstream = None
        if need["stream"]:
            dstream = torch.empty(B, L, D, device=dvideo.device)
            d2 = dstream.view(B * L, D)
            m0, m1 = _dual_maps(lead, n0, n1, L)
            _convt_input_grad(dr0, wt0, omap=m0, out=d2)
            _convt_input_grad(dr1, wt1, omap=m1, out=d2)
            if lead:
                hip.zero_rows(d2, rows=B * lead, rmap=hip.RowMap(lead, L, 0))
        wg = _WeightGrads()
        dw0, dw1 = wg.add(x0, dr0, need["w0"]), wg.add(x1, dr1, need["w1"])
        wg.run()
        return _grads(ctx, DualConvTransposePatch, stream=dstream, w0=_shaped(dw0, (D, C, pt0, ph, pw)), w1=_shaped(dw1, (D, C, pt1, ph, pw)),
                      b0=_convt_bias_grad(dr0, C) if need["b0"] else None, b1=_convt_bias_grad(dr1, C) if need["b1"] else None)


class DualDecoderStream(torch.autograd.Function):
    """The decoder's sequence (blocks.py:222-229): [x + latent_pos | first_patch_queries | rest_patch_queries] as fp32 [B, n + N0 + N1, D] by three
    vt_assemble_rows calls (x: the proj_in output fp32 [B, n, D]; the tables [1, rows, D], broadcast over the batch), no torch.cat.
    Backward: d x is the first n rows of every sequence, the tables' gradients are vt_batch_sum through a row map."""

    @staticmethod
    def forward(ctx, x, latent_pos, q0, q1):
        hip.require_gpu(x, latent_pos, q0, q1)
        B, n, D = x.shape
        n0, n1 = q0.numel() // D, q1.numel() // D
        L = n + n0 + n1
        assert latent_pos.numel() == n * D
        out = torch.empty(B, L, D, device=x.device)
        o2 = out.view(B * L, D)
        tab = [t.detach().reshape(-1, D).float().contiguous() for t in (latent_pos, q0, q1)]
        hip.assemble_rows(o2, L, 0, B, n, src=x.contiguous().float().view(B * n, D), table=tab[0])
        hip.assemble_rows(o2, L, n, B, n0, table=tab[1])
        hip.assemble_rows(o2, L, n + n0, B, n1, table=tab[2])
        ctx.geom = (B, n, n0, n1, D)
        ctx.shapes = (latent_pos.shape, q0.shape, q1.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, n, n0, n1, D = ctx.geom
        L = n + n0 + n1
        need = _needs(ctx, DualDecoderStream)
        d = dout.contiguous().float()
        d2 = d.view(B * L, D)
        s_lp, s_q0, s_q1 = ctx.shapes
        return _grads(ctx, DualDecoderStream, x=d[:, :n],
                      latent_pos=hip.batch_sum(d2, B, n, rmap=hip.RowMap(n, L, 0)).reshape(s_lp) if need["latent_pos"] else None,
                      q0=hip.batch_sum(d2, B, n0, rmap=hip.RowMap(n0, L, n)).reshape(s_q0) if need["q0"] else None,
                      q1=hip.batch_sum(d2, B, n1, rmap=hip.RowMap(n1, L, n + n0)).reshape(s_q1) if need["q1"] else None)


# ---- the 3D ResNet ends of autoencoder_cnnvit -------------------------------------------------------------------------------------------------
def _pad16(c):
    return (c + 15) // 16 * 16


def _cl(x):
    """logical [B, C, T, H, W] -> the bf16 [B, T, H, W, C] the kernels read: a view where x is bf16 channels_last_3d already, one copy otherwise"""
    if x is None:
        return None
    assert x.dim() == 5
    return x.to(torch.bfloat16).permute(0, 2, 3, 4, 1).contiguous()


def _logical(x_cl):
    """bf16 [B, T, H, W, C] -> the logical [B, C, T, H, W] view of the same memory (channels_last_3d)"""
    return x_cl.permute(0, 4, 1, 2, 3)


class Conv3x3x3(torch.autograd.Function):
    """nn.Conv3d(kernel 3, padding 1, stride (1,1,1) / (1,2,2) / (2,2,2)) under autocast(bf16) on channels-last activations (cnnvit.py:21-28,
    86, 95, 115, 172): out = bf16(acc + bias), and with `residual` bf16(float(bf16(acc + bias)) + float(residual)), the two roundings autocast gives
    `x + conv2(h)`.  `owner`, `name`: the module and attribute path of the nn.Conv3d, for the pack registry.  A 3-channel end runs at 16 channels:
    the input's pad channels are zero (VideoToChannelsLast), the output's are bf16(0 + 0)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, owner, name):
        hip.require_gpu(x, weight, bias, residual)
        xc = _cl(x)
        cout, cin = weight.shape[:2]
        cout_abi, cin_abi = _pad16(cout), xc.shape[-1]
        assert cin_abi == _pad16(cin), f"Conv3x3x3: the input has {xc.shape[-1]} channels, the weight {cin}"
        b = bias.detach().float()
        if cout_abi != cout:
            b = torch.nn.functional.pad(b, (0, cout_abi - cout))
        out = hip.conv3d_fwd(xc, packs.conv3d(owner, name, cout_abi, cin_abi), b.contiguous(), cout_abi, stride, residual=_cl(residual))
        ctx.save_for_backward(xc)
        ctx.conv = (stride, owner, name, cout, cin, cout_abi, cin_abi)
        return _logical(out)

    @staticmethod
    def backward(ctx, dy):
        xc, = ctx.saved_tensors
        stride, owner, name, cout, cin, cout_abi, cin_abi = ctx.conv
        need = _needs(ctx, Conv3x3x3)
        dyc = _cl(dy)                                               # the gradient of a bf16 output is bf16 under autocast
        dx = dw = db = None
        if need["x"]:
            dx = _logical(hip.conv3d_dgrad(dyc, packs.conv3d(owner, name, cout_abi, cin_abi, for_dgrad=True), tuple(xc.shape[1:4]), cin_abi, stride))
        if need["weight"]:
            dw = hip.conv3d_wgrad(xc, dyc, stride, cout, cin)
        if need["bias"]:
            db = hip.colsum(dyc.view(-1, cout_abi))[:cout].contiguous()
        return _grads(ctx, Conv3x3x3, x=dx, weight=dw, bias=db, residual=dy)


class GroupNormSwish(torch.autograd.Function):
    """nn.GroupNorm(G, C, eps) and, with swish, x * sigmoid(x) behind it (cnnvit.py:5-10): statistics and the activation in fp32 from the bf16
    input, rounded to bf16 once."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, swish):
        hip.require_gpu(x, weight, bias)
        xc = _cl(x)
        w, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        y, mean, rstd = hip.groupnorm_fwd(xc, w, b, eps, groups, swish)
        ctx.save_for_backward(xc, w, b, mean, rstd)
        ctx.gn = (groups, swish)
        return _logical(y)

    @staticmethod
    def backward(ctx, dy):
        xc, w, b, mean, rstd = ctx.saved_tensors
        dx, dg, db = hip.groupnorm_bwd(_cl(dy), xc, w, b, mean, rstd, *ctx.gn)
        return _grads(ctx, GroupNormSwish, x=_logical(dx), weight=dg, bias=db)


class UpsampleNearest(torch.autograd.Function):
    """F.interpolate(x, scale_factor=(2,2,2) or (1,2,2), mode='nearest') (cnnvit.py:99); the backward adds a position's children in fp32"""

    @staticmethod
    def forward(ctx, x, scale):
        hip.require_gpu(x)
        ctx.scale = tuple(int(s) for s in scale)
        return _logical(hip.upsample_nearest_fwd(_cl(x), ctx.scale))

    @staticmethod
    def backward(ctx, dy):
        return _logical(hip.upsample_nearest_bwd(_cl(dy), ctx.scale)), None


class VideoToChannelsLast(torch.autograd.Function):
    """fp32 video [B, C, T, H, W] -> the logical [B, 16k, T, H, W] bf16 channels-last activation, channels C.. zero (the autocast cast in front
    of conv_in); the video's gradient is computed only when the video requires one"""

    @staticmethod
    def forward(ctx, video):
        hip.require_gpu(video)
        ctx.C = video.shape[1]
        return _logical(hip.video_to_channels_last(video.float().contiguous(), _pad16(ctx.C)))

    @staticmethod
    def backward(ctx, dy):
        return hip.channels_last_to_video(_cl(dy), ctx.C)


class ChannelsLastToVideo(torch.autograd.Function):
    """the first C channels of a logical [B, 16k, T, H, W] bf16 activation -> fp32 [B, C, T, H, W] holding the bf16 values (as pred_frames elsewhere)"""

    @staticmethod
    def forward(ctx, x, C):
        hip.require_gpu(x)
        ctx.cpad = x.shape[1]
        return hip.channels_last_to_video(_cl(x), C)

    @staticmethod
    def backward(ctx, dvideo):
        return _logical(hip.video_to_channels_last(dvideo.float().contiguous(), ctx.cpad)), None
