"""The reference's `autoencoder_dualpatch` (models/model_dualpatch/autoencoder.py:8-84; Encoder / Decoder of base/blocks.py:12-258) on the
MI355X kernels: an FSQ tokenizer whose clip is cut along time into a first segment, patchified with a (1, 8, 8) Conv3d, and a rest segment,
patchified with a (3, 8, 8) Conv3d, each with a learned position table of its own; the decoder ends in two ConvTranspose3d whose outputs are
concatenated along T.

Same module tree and state-dict keys as the reference (`encoder.first_patch_embed`, `encoder.rest_patch_embed`, `encoder.first_pos_embed`,
`encoder.rest_pos_embed`, `encoder.latent_queries`, `encoder.model_layers.{attn_layer,ffd_layer}.{i}.*`, `encoder.proj_out`; `decoder.proj_in`,
`decoder.latent_pos_embed`, `decoder.first_patch_queries`, `decoder.rest_patch_queries`, `decoder.model_layers.*`, `decoder.first_unpatch`,
`decoder.rest_unpatch`; `quantize` has no entries), the same constructor keywords and defaults, the same init.

The ends run on the two-segment entry points of csrc/vt_patch.hip (functional.DualPatchEmbed / DualConvTransposePatch / DualDecoderStream): one patchify launch for both
segments, GEMMs that write straight into the residual stream, one unpatchify launch for both segments.  The layer stack is the gated
LayerNorm-per-head stack of titok.ResidualAttentionBlock (base/transformer.py:58-81 of this family is that stack WITHOUT a rotary embedding)
with identity rotary tables: cos = 1, sin = 0 changes no value (x * 1 + y * (+-0) == x), so no second instantiation of the qk-norm kernel
and no new stack entry points exist.  Mixed precision = autocast(bf16) as the reference trains.  GPU tensors only; B * L must
be a multiple of 64, width one of the gated engine's 256 / 512 / 768 / 1024.
"""
import torch
from torch import nn

from .fsq import FSQ
from .functional import DualConvTransposePatch, DualDecoderStream, DualPatchEmbed, Linear as LinearFn
from .registry import register
from .titok import ResidualAttentionBlock, get_model_dims, init_weights


class _IdentityRotary:
    """cos = 1, sin = 0 as fp32 [L, 32] device tables, made once per device: the stack engine's rotation with them is the identity"""

    def _freqs(self, device, L):
        tabs = self.__dict__.get("_freqs_dev")
        if tabs is None or tabs[0].device != device or tabs[0].shape[0] != L:
            tabs = (torch.ones(L, 32, device=device), torch.zeros(L, 32, device=device))
            self.__dict__["_freqs_dev"] = tabs
        return tabs


class _DualGrid:
    """the token geometry both ends share (blocks.py:35-49, 157-170): ONE first-segment temporal token of first_frame_temporal_patch frames"""

    def _set_grid(self, spatial_patch_size, first_frame_temporal_patch, rest_temporal_patch, num_frames, spatial_size):
        self.spatial_patch_size, self.spatial_size = tuple(spatial_patch_size), tuple(spatial_size)
        self.first_frame_temporal_patch, self.rest_temporal_patch, self.num_frames = first_frame_temporal_patch, rest_temporal_patch, num_frames
        ph, pw = self.spatial_patch_size
        self.spatial_grid = (self.spatial_size[0] // ph, self.spatial_size[1] // pw)
        nh, nw = self.spatial_grid
        self.first_temporal_grid = 1
        self.first_num_tokens = nh * nw
        self.rest_frame_count = num_frames - first_frame_temporal_patch
        assert self.rest_frame_count > 0 and self.rest_frame_count % rest_temporal_patch == 0
        self.rest_temporal_grid = self.rest_frame_count // rest_temporal_patch
        self.rest_num_tokens = self.rest_temporal_grid * nh * nw
        self.total_patch_tokens = self.first_num_tokens + self.rest_num_tokens


class DualPatchEncoder(nn.Module, _IdentityRotary, _DualGrid):
    """`Encoder` (blocks.py:12-128): [latent_queries | first-frame patch tokens + first_pos_embed | rest patch tokens + rest_pos_embed] through the
    layer stack, first out_tokens rows -> Linear(width, token_size).  `_dims` = (width, layers, heads, mlp_ratio) replaces
    get_model_dims(model_size) for small tests."""

    def __init__(self, model_size="small_thin", spatial_patch_size=(8, 8), first_frame_temporal_patch=1, rest_temporal_patch=3, in_channels=3,
                 out_channels=6, num_frames=16, spatial_size=(128, 128), out_tokens=1024, _dims=None):
        super().__init__()
        self._set_grid(spatial_patch_size, first_frame_temporal_patch, rest_temporal_patch, num_frames, spatial_size)
        self.token_size, self.in_channels, self.out_tokens = out_channels, in_channels, out_tokens
        ph, pw = self.spatial_patch_size
        self.width, self.num_layers, self.heads, mlp_ratio = _dims if _dims is not None else get_model_dims(model_size)
        scale = self.width ** -0.5
        k0, k1 = (first_frame_temporal_patch, ph, pw), (rest_temporal_patch, ph, pw)
        self.first_patch_embed = nn.Conv3d(in_channels, self.width, kernel_size=k0, stride=k0, bias=True)
        self.rest_patch_embed = nn.Conv3d(in_channels, self.width, kernel_size=k1, stride=k1, bias=True)
        self.first_pos_embed = nn.Parameter(scale * torch.randn(1, self.first_num_tokens, self.width))
        self.rest_pos_embed = nn.Parameter(scale * torch.randn(1, self.rest_num_tokens, self.width))
        self.latent_queries = nn.Parameter(scale * torch.randn(1, out_tokens, self.width))
        self.model_layers = ResidualAttentionBlock(self.width, self.heads, mlp_ratio, self.num_layers)
        self.proj_out = nn.Linear(self.width, self.token_size, bias=True)
        self.apply(init_weights)

    def stream(self, x):
        """the residual stream in front of the layer stack, fp32 [B, out_tokens + N0 + N1, width]"""
        return DualPatchEmbed.apply(x, self.first_patch_embed.weight, self.first_patch_embed.bias, self.first_pos_embed, self.rest_patch_embed.weight,
                                    self.rest_patch_embed.bias, self.rest_pos_embed, self.out_tokens, self.latent_queries)

    def forward(self, x):
        assert tuple(x.shape[2:]) == (self.num_frames,) + self.spatial_size, "the position tables are built for one clip size"
        h = self.stream(x)
        h = self.model_layers(h, freqs=self._freqs(h.device, h.shape[1]))[:, :self.out_tokens]
        return LinearFn.apply(h, self.proj_out.weight, self.proj_out.bias)


class DualPatchDecoder(nn.Module, _IdentityRotary, _DualGrid):
    """`Decoder` (blocks.py:134-258): [proj_in(x) + latent_pos_embed | first_patch_queries | rest_patch_queries] through the layer stack, the rows
    behind the in_tokens latents -> first_unpatch / rest_unpatch (ConvTranspose3d), concatenated along T.  The pair keeps torch's default init:
    init_weights names nn.Conv3d, which ConvTranspose3d is not."""

    def __init__(self, model_size="small_thin", spatial_patch_size=(8, 8), first_frame_temporal_patch=1, rest_temporal_patch=3, in_channels=6,
                 out_channels=3, in_tokens=1024, num_frames=16, spatial_size=(128, 128), _dims=None):
        super().__init__()
        self._set_grid(spatial_patch_size, first_frame_temporal_patch, rest_temporal_patch, num_frames, spatial_size)
        self.token_size, self.out_channels, self.in_tokens = in_channels, out_channels, in_tokens
        ph, pw = self.spatial_patch_size
        self.width, self.num_layers, self.heads, mlp_ratio = _dims if _dims is not None else get_model_dims(model_size)
        scale = self.width ** -0.5
        self.proj_in = nn.Linear(self.token_size, self.width, bias=True)
        self.latent_pos_embed = nn.Parameter(scale * torch.randn(1, in_tokens, self.width))
        self.first_patch_queries = nn.Parameter(scale * torch.randn(1, self.first_num_tokens, self.width))
        self.rest_patch_queries = nn.Parameter(scale * torch.randn(1, self.rest_num_tokens, self.width))
        self.model_layers = ResidualAttentionBlock(self.width, self.heads, mlp_ratio, self.num_layers)
        k0, k1 = (first_frame_temporal_patch, ph, pw), (rest_temporal_patch, ph, pw)
        self.first_unpatch = nn.ConvTranspose3d(self.width, out_channels, kernel_size=k0, stride=k0, bias=True)
        self.rest_unpatch = nn.ConvTranspose3d(self.width, out_channels, kernel_size=k1, stride=k1, bias=True)
        self.apply(init_weights)

    def forward(self, x):
        B = x.shape[0]
        h = LinearFn.apply(x, self.proj_in.weight, self.proj_in.bias)
        h = DualDecoderStream.apply(h, self.latent_pos_embed, self.first_patch_queries, self.rest_patch_queries)
        h = self.model_layers(h, freqs=self._freqs(h.device, h.shape[1]))
        geom = (B, self.out_channels, self.num_frames, self.spatial_size[0], self.spatial_size[1], self.first_frame_temporal_patch,
                self.first_frame_temporal_patch, self.rest_temporal_patch, self.spatial_patch_size[0], self.spatial_patch_size[1])
        return DualConvTransposePatch.apply(h, self.in_tokens, self.first_unpatch.weight, self.first_unpatch.bias, self.rest_unpatch.weight,
                                            self.rest_unpatch.bias, geom)


@register("autoencoder_dualpatch")
class AutoEncoderDualPatch(nn.Module):
    """autoencoder.py:8-84: every constructor keyword of the reference is accepted and ignored (it builds Encoder() and Decoder() with their
    defaults: small_thin, 16 x 128 x 128 clips, 1024 latent tokens, FSQ [8, 8, 8, 5, 5, 5]).  `_geometry` = dict(dims, spatial_patch_size,
    first_frame_temporal_patch, rest_temporal_patch, num_frames, spatial_size, tokens), any subset, overrides the geometry for small tests.

    `autoencoder_first_token` / `autoencoder_first_token_res` of the same reference file are NOT registered: their constructors pass
    patch_size= / in_grid= to this Encoder, which takes neither -- a TypeError in the reference itself."""
    LEVELS = [8, 8, 8, 5, 5, 5]
    output_format = "bcthw"

    def __init__(self, bottleneck=None, prior_model=None, _geometry=None, **kwargs):
        super().__init__()
        g = dict(_geometry or {})
        tokens = g.pop("tokens", 1024)
        if "dims" in g:
            g["_dims"] = g.pop("dims")
        token_size = len(self.LEVELS)
        self.encoder = DualPatchEncoder(out_channels=token_size, out_tokens=tokens, **g)
        self.quantize = FSQ(levels=self.LEVELS)
        self.decoder = DualPatchDecoder(in_channels=token_size, in_tokens=tokens, **g)
        self.prior_model = None

    def encode(self, data, **kwargs):
        return self.quantize(self.encoder(data))

    def decode(self, x):
        return self.decoder(x)

    def decode_indices(self, indices):
        return self.decoder(self.quantize.indices_to_codes(indices))

    def forward(self, x):
        x_q, _ = self.encode(x)
        return {"pred_frames": self.decode(x_q)}
