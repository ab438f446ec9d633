"""`autoencoder_stat` (models/model_stat/autoencoder.py:8-152, base/blocks.py:11-154; what cfgs/larp_tokenizer_stat.yaml names): the
adaptive-length FSQ tokenizer.  A probability head scores each of the 1280 latent tokens; training keeps a token with a Bernoulli
draw and a straight-through gradient, evaluation keeps the tokens whose probability is above 0.5, and the dropped tokens are zeroed
before FSQ.

Same module tree and state-dict keys as the reference (`encoder.proj_in` = Linear(3*4*8*8, 768), `encoder.mask_token`,
`encoder.prob_head.net.{0,2}`, `encoder.model_layers.*`, `encoder.proj_out`, `decoder.proj_in`, `decoder.mask_token`,
`decoder.model_layers.*`, `decoder.proj_out` = Linear(768, 3*4*8*8); `quantize` has no entries), same constructor keywords (every
size keyword is accepted and ignored: the reference hard-codes 16x128x128 clips, (4, 8, 8) patches, model size 'base', 1280 latent
tokens and FSQ levels [8,8,8,5,5,5]; the private `_geometry=` dict(in_grid, patch_size, tokens, model_size) is for small tests), same
`encode(data, current_epoch=0) -> (codes, {'indices', 'mask', 'probs', 'stage'})`, `decode(x)`, `forward(x, current_epoch=0) ->
{'pred_frames', 'probs', 'mask', 'stage'}`, `get_stage`, `get_mask_with_ste`.

The layer stacks, FSQ constants and rotary tables are the FSQ family's (titok.py).  The two layouts that differ from it:
  * patchify is a Linear over `b c (t pt) (h ph) (w pw) -> b (t h w) (pt ph pw c)` (channel-last inside a patch): the weight is
    viewed as [768, pt, ph, pw, c] and permuted to the Conv3d layout, then functional.PatchEmbed runs it;
  * unpatchify is a Linear(768, 3*4*8*8) with a per-element bias and the inverse rearrange: the rows and bias of `proj_out` are
    permuted to (c, pt, ph, pw) order, then functional.Linear + functional.Unpatchify run it.
The permutes are autograd ops on the weights (their gradients permute back).

The token gate is one autograd Function, `StatGate`: fc1 of the head as a vt_gemm_nt with the GELU epilogue, then
vt_stat_gate_forward (fc2 + sigmoid + mask + FSQ of the masked latents, one row pass); backward = vt_stat_gate_backward (FSQ's
straight-through gradient, the mask's STE, sigmoid', fc2's gradients, gelu') and the existing GEMMs for fc1's weight gradient, its
bias (column sum) and the gradient into the stack, which carries the 0.1 of `x.detach() + 0.1 * (x - x.detach())` (blocks.py:89).

Mixed precision follows the autocast(bf16) rounding points of the FSQ family: bf16 GEMM operands with fp32 accumulation; every
Linear output rounded to bf16 (proj_in, proj_out, fc1 = u and gelu(u) in bf16, the logit of fc2); the sigmoid runs on the bf16
logit and its output is rounded to bf16 like a bf16 tensor op; FSQ runs in fp32 with autocast off as in the reference; the mask is
exactly 0 or 1.  GPU tensors only; B * 1280 (B * tokens) must be a multiple of 64.
"""
import math

import torch
from torch import nn

from . import hip
from .fsq import FSQ
from .functional import Linear as LinearFn, PatchEmbed as PatchEmbedFn, Unpatchify as UnpatchifyFn, _grads, _needs, _WeightGrads
from .registry import register
from .titok import ResidualAttentionBlock, _RopeMixin, get_model_dims, init_weights, rope_tables


def _bf16_rows(x):
    """bf16 [M, W] copy of an fp32 [B, n, W] tensor that is either contiguous or the first n rows of each batch item of a
    contiguous [B, L, W] tensor (the encoder keeps h[:, :n]); the slice is read in place through a row map"""
    B, n, W = x.shape
    if x.is_contiguous():
        return hip.cast_rows(x.float(), rows=B * n)
    if x.dtype == torch.float32 and x.stride(2) == 1 and x.stride(1) == W and x.stride(0) % W == 0:
        return hip.cast_rows(x, rows=B * n, rmap=hip.RowMap(n, x.stride(0) // W, 0))
    return hip.cast_rows(x.contiguous().float(), rows=B * n)


class StatGate(torch.autograd.Function):
    """x [B, n, W] fp32 (the stack's latent rows), z [B, n, d] fp32 or None (proj_out's output) -> codes [B, n, d] (None without z),
    probs [B, n], mask [B, n], indices int32 [B, n] (None without z).  probs = ProbPredictor(x) (blocks.py:11-24), mask by `mode`
    (hip.STAT_*), codes / indices = FSQ(z * mask).  The gradient into x is scaled by `x_grad_scale`."""

    @staticmethod
    def forward(ctx, x, z, w1, b1, w2, b2, levels, mode, seed, mask_in, x_grad_scale):
        hip.require_gpu(x, z, w1, b1, w2, b2, mask_in)
        B, n, W = x.shape
        M = B * n
        if M % 64:
            raise hip.HipError(f"StatGate: B * tokens = {M} must be a multiple of 64")
        xb = _bf16_rows(x)
        w1b, w1t = hip.pack_weight(w1.detach())
        u, g = hip.gemm_nt(xb, w1b, hip.EPI_BF16_GELU, bias=b1.detach().float().contiguous())
        w2f = w2.detach().reshape(-1).float().contiguous()
        b2f = b2.detach().reshape(1).float().contiguous()
        z2 = z.detach().reshape(M, -1).float().contiguous() if z is not None else None
        mi = mask_in.detach().reshape(M).float().contiguous() if mask_in is not None else None
        probs, mask, codes, idx = hip.stat_gate_forward(g, w2f, b2f, z2, levels if z is not None else None, mode, seed, mi)
        ste = mode in (hip.STAT_SAMPLE, hip.STAT_FORCED)
        ctx.save_for_backward(xb, w1t, u, g, z2, mask, probs, w2f)
        ctx.cfg = (x.shape, None if z is None else z.shape, levels if z is not None else None, ste, float(x_grad_scale))
        outs = [codes.reshape(B, n, -1) if codes is not None else None, probs.reshape(B, n), mask.reshape(B, n),
                idx.reshape(B, n) if idx is not None else None]
        const = [outs[3]] + ([] if ste else [outs[2]])     # a thresholded / all-ones mask is a constant (autoencoder.py:98,110)
        ctx.mark_non_differentiable(*[t for t in const if t is not None])
        return tuple(outs)

    @staticmethod
    def backward(ctx, dcodes, dprobs, dmask, _didx):
        xb, w1t, u, g, z2, mask, probs, w2f = ctx.saved_tensors
        xshape, zshape, levels, ste, scale = ctx.cfg
        M, W = g.shape
        dc = None
        if z2 is not None:
            dc = dcodes.reshape(z2.shape).float().contiguous() if dcodes is not None else torch.zeros_like(z2)
        dp = dprobs.reshape(M).float().contiguous() if dprobs is not None else None
        dm = dmask.reshape(M).float().contiguous() if (dmask is not None and ste) else None
        dU, dz, dw2, db2 = hip.stat_gate_backward(dc, dp, dm, z2, mask, probs, u, g, w2f, levels, ste)
        need = _needs(ctx, StatGate)
        dx = db1 = None
        if need["x"]:
            dx = hip.gemm_nt(dU, w1t, hip.EPI_F32, out_scale=scale if scale != 1.0 else 0.0).reshape(xshape)
        wg = _WeightGrads()
        dw1 = wg.add(dU, xb, need["w1"])
        wg.run()
        if need["b1"]:
            db1 = hip.colsum(dU, rows=M)
        return _grads(ctx, StatGate, x=dx, z=dz.reshape(zshape) if dz is not None else None, w1=dw1, b1=db1, w2=dw2.reshape(1, W), b2=db2)


class ProbPredictor(nn.Module):
    """blocks.py:11-24: Linear(W, W) -> GELU -> Linear(W, 1) -> Sigmoid (keys net.0.*, net.2.*); runs as StatGate"""

    def __init__(self, embed_dim):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU(), nn.Linear(embed_dim, 1))
        self.sigmoid = nn.Sigmoid()

    def gate(self, x, z=None, levels=None, mode=hip.STAT_ONES, seed=0, mask_in=None, x_grad_scale=1.0):
        fc1, fc2 = self.net[0], self.net[2]
        return StatGate.apply(x, z, fc1.weight, fc1.bias, fc2.weight, fc2.bias, levels, mode, seed, mask_in, x_grad_scale)

    def forward(self, x):
        """x [B, n, W] -> probs [B, n, 1]"""
        return self.gate(x)[1].unsqueeze(-1)


class Encoder(nn.Module, _RopeMixin):
    """blocks.py:40-94: Linear patchify, `out_tokens` scalar mask tokens in FRONT of the patch tokens, layers, first out_tokens rows
    -> (proj_out, prob_head with the gradient into the stack scaled by 0.1)"""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=3, out_channels=5, in_grid=(32, 256, 256), out_tokens=2048):
        super().__init__()
        self.patch_size, self.token_size, self.in_channels, self.out_tokens = tuple(patch_size), out_channels, in_channels, out_tokens
        self.grid = [x // y for x, y in zip(in_grid, patch_size)]
        self.width, self.num_layers, self.heads, mlp_ratio = get_model_dims(model_size)
        assert patch_size[1] == patch_size[2] and in_grid[1] == in_grid[2], "square frames and patches (the reference's only geometry)"
        self.proj_in = nn.Linear(in_features=in_channels * math.prod(patch_size), out_features=self.width)
        self.mask_token = nn.Parameter(self.width ** -0.5 * torch.randn(1, 1, 1))
        self.freqs = rope_tables(out_tokens, self.grid, head_dim=self.width // self.heads)
        self._freqs_dev = None
        self.prob_head = ProbPredictor(self.width)
        self.model_layers = ResidualAttentionBlock(self.width, self.heads, mlp_ratio, self.num_layers)
        self.proj_out = nn.Linear(self.width, self.token_size, bias=True)
        self.apply(init_weights)

    def conv_weight(self):
        """proj_in.weight [W, pt*ph*pw*c] viewed as [W, pt, ph, pw, c] and permuted to the Conv3d layout [W, c, pt, ph, pw]"""
        pt, ph, pw = self.patch_size
        return self.proj_in.weight.view(self.width, pt, ph, pw, self.in_channels).permute(0, 4, 1, 2, 3)

    def features(self, x):
        """-> (z = proj_out(latents) [B, n, d], latents [B, n, W]): everything of forward() but the probability head"""
        B = x.shape[0]
        tok = PatchEmbedFn.apply(x, self.conv_weight(), self.proj_in.bias, None)
        h = torch.cat([self.mask_token.expand(B, self.out_tokens, self.width), tok], dim=1)
        h = self.model_layers(h, freqs=self._freqs(x.device))
        lat = h[:, :self.out_tokens]
        return LinearFn.apply(lat, self.proj_out.weight, self.proj_out.bias), lat

    def forward(self, x):
        z, lat = self.features(x)
        return z, self.prob_head.gate(lat, x_grad_scale=0.1)[1]


class Decoder(nn.Module, _RopeMixin):
    """blocks.py:96-154: Linear(token_size, W), grid_size scalar mask tokens BEHIND the latents, layers, last grid_size rows ->
    Linear(W, C*pt*ph*pw) and the inverse rearrange"""

    def __init__(self, model_size="tiny", patch_size=(4, 8, 8), in_channels=5, out_channels=3, in_tokens=2048, out_grid=(32, 256, 256)):
        super().__init__()
        self.patch_size, self.token_size, self.in_channels, self.in_tokens = tuple(patch_size), in_channels, out_channels, in_tokens
        self.out_grid = tuple(out_grid)
        self.grid = [x // y for x, y in zip(out_grid, patch_size)]
        self.grid_size = math.prod(self.grid)
        self.width, self.num_layers, self.heads, mlp_ratio = get_model_dims(model_size)
        assert patch_size[1] == patch_size[2] and out_grid[1] == out_grid[2], "square frames and patches (the reference's only geometry)"
        self.proj_in = nn.Linear(self.token_size, self.width, bias=True)
        self.mask_token = nn.Parameter(self.width ** -0.5 * torch.randn(1, 1, 1))
        self.freqs = rope_tables(in_tokens, self.grid, head_dim=self.width // self.heads)
        self._freqs_dev = None
        self.model_layers = ResidualAttentionBlock(self.width, self.heads, mlp_ratio, self.num_layers)
        self.proj_out = nn.Linear(in_features=self.width, out_features=out_channels * math.prod(patch_size))
        self.apply(init_weights)

    def row_weights(self):
        """proj_out's rows and bias permuted from (pt, ph, pw, c) to the (c, pt, ph, pw) order of the unpatchify scatter"""
        pt, ph, pw = self.patch_size
        C = self.in_channels
        w = self.proj_out.weight.view(pt, ph, pw, C, self.width).permute(3, 0, 1, 2, 4).reshape(C * pt * ph * pw, self.width)
        b = self.proj_out.bias.view(pt, ph, pw, C).permute(3, 0, 1, 2).reshape(-1)
        return w, b

    def forward(self, x):
        B = x.shape[0]
        h = LinearFn.apply(x, self.proj_in.weight, self.proj_in.bias)
        h = torch.cat([h, self.mask_token.expand(B, self.grid_size, self.width)], dim=1)
        h = self.model_layers(h, freqs=self._freqs(x.device))
        w, b = self.row_weights()
        rows = LinearFn.apply(h[:, self.in_tokens:], w, b)
        geom = (B, self.in_channels, self.out_grid[0], self.out_grid[1], self.patch_size[0], self.patch_size[1])
        return UnpatchifyFn.apply(rows.reshape(B * self.grid_size, -1), geom)


@register("autoencoder_stat")
class AutoEncoderStat(nn.Module):
    """autoencoder.py:8-152.  `bottleneck` and `prior_model` are accepted and unused, as every size keyword."""
    LEVELS = [8, 8, 8, 5, 5, 5]
    output_format = "bcthw"

    def __init__(self, bottleneck=None, prior_model=None, num_latent_tokens=1024, input_size=128, frame_num=16, temporal_patch_size=4,
                 patch_size=8, decoder_temporal_patch_size=4, decoder_patch_size=8, in_channels=3, transformer_name="transformer_encoder_parallel",
                 encoder_name=None, decoder_name=None, encoder_hidden_size=768, decoder_hidden_size=768, encoder_num_heads=12, decoder_num_heads=12,
                 encoder_depth=6, decoder_depth=6, latent_pe_scale_factor=10000, query_init_std=0.02, encoder_query_gaussian_init=True,
                 learned_decoder_latent_pe=False, _geometry=None, **kwargs):
        super().__init__()
        g = dict(in_grid=[16, 128, 128], patch_size=[4, 8, 8], tokens=1280, model_size="base")
        g.update(_geometry or {})
        token_size = len(self.LEVELS)
        self.encoder = Encoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=3, out_channels=token_size,
                               in_grid=g["in_grid"], out_tokens=g["tokens"])
        self.quantize = FSQ(levels=self.LEVELS)
        self.decoder = Decoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=token_size, out_channels=3,
                               in_tokens=g["tokens"], out_grid=g["in_grid"])
        self.prior_model = None

    def _seed(self):
        """per-call seed of the Bernoulli draw: torch's seed and a call counter, as SimpleVectorQuantizer.forward"""
        self._calls = getattr(self, "_calls", 0) + 1
        return (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._calls) & 0xFFFFFFFFFFFFFFFF

    def get_mask_with_ste(self, probs):
        """autoencoder.py:69-88 on a given probability tensor (a small [B, N] op outside the hot path; encode() draws its mask
        inside the fused gate instead, from a counter-hash uniform)"""
        if self.training:
            mask = torch.bernoulli(probs.detach())
            return (mask - probs).detach() + probs
        return (probs > 0.5).to(probs)

    def get_stage(self, current_epoch):
        """autoencoder.py:90-96: 'random_drop' is unreachable there (both tests are `< 0`) and is not built"""
        return "vanilla" if current_epoch < 0 else "adaptive"

    def _mode(self, stage):
        if self.training:
            return hip.STAT_SAMPLE if stage == "adaptive" else hip.STAT_ONES
        return hip.STAT_THRESHOLD if stage == "adaptive" else hip.STAT_ONES

    def encode(self, data, current_epoch=0, **kwargs):
        z, lat = self.encoder.features(data)
        stage = self.get_stage(current_epoch)
        mode = self._mode(stage)
        seed = self._seed() if mode == hip.STAT_SAMPLE else 0
        codes, probs, mask, idx = self.encoder.prob_head.gate(lat, z, self.quantize.levels, mode, seed, x_grad_scale=0.1)
        return codes, {"indices": idx, "mask": mask, "probs": probs, "stage": stage}

    def decode(self, x):
        return self.decoder(x)

    def forward(self, x, current_epoch=0):
        x_q, out = self.encode(x, current_epoch=current_epoch)
        return {"pred_frames": self.decode(x_q), "probs": out["probs"], "mask": out["mask"], "stage": out["stage"]}
