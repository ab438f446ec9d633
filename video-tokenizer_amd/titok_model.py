"""The reference's `titok` registry entry (models/model_titok/titok.py): TiTokEncoder -> FSQ([8, 8, 8, 5, 5, 5]) -> TiTokDecoder on clips of
variable size, packed from the encoder's input to the decoder's output (varlen.py; the data movement is csrc/vt_packed.hip).

As in the reference every constructor keyword is accepted and ignored and the geometry is hard-coded: `base` encoder and decoder (width 768,
12 + 12 layers, 12 query heads over 4 KV heads), patch (4, 8, 8), token size 6, no prior model.  `_geometry` = dict(dims=(width, layers,
[Hq, Hkv], mlp_ratio), patch_size=(pt, p, p)) overrides it for small tests.  The state-dict keys are the reference's."""
import torch
import torch.nn as nn

from .fsq import FSQ
from .registry import register
from .varlen import TiTokDecoder, TiTokEncoder, init_weights


@register("titok")
class TiTok(nn.Module):
    TOKENS, LEVELS = 1024, [8, 8, 8, 5, 5, 5]

    def __init__(self, bottleneck=None, prior_model=None, _geometry=None, **kwargs):
        super().__init__()
        g = dict(dims=None, patch_size=[4, 8, 8])
        g.update(_geometry or {})
        in_grid = [16, 128, 128]
        token_size = len(self.LEVELS)
        self.encoder = TiTokEncoder(model_size="base", patch_size=g["patch_size"], in_channels=3, out_channels=token_size, max_grid=in_grid,
                                    max_tokens=self.TOKENS, _dims=g["dims"])
        self.quantize = FSQ(levels=self.LEVELS)
        self.decoder = TiTokDecoder(model_size="base", patch_size=g["patch_size"], in_channels=token_size, out_channels=3, max_grid=in_grid,
                                    max_tokens=self.TOKENS, _dims=g["dims"])
        self.prior_model = None
        self.apply(init_weights)

    def encode(self, x, token_counts):
        """x: a list of clips [3, T_b, H_b, W_b] -> (x_q [sum token_counts, 6], {'indices': one int32 [token_counts[b]] per clip})"""
        x = self.encoder(x, token_counts)
        x_q, x_dict = self.quantize(x)
        x_dict["indices"] = torch.split(x_dict["indices"], [int(n) for n in token_counts], dim=0)
        return x_q, x_dict

    def decode(self, x, token_counts, grids):
        """x [sum token_counts, 6], grids[b] = (T_b, H_b, W_b) in pixels -> a list of clips [3, T_b, H_b, W_b]"""
        return self.decoder(x, token_counts, grids)

    def decode_indices(self, indices, grids):
        """indices: one index tensor per clip (encode's split), or a [B, n] tensor"""
        token_counts = [int(x.shape[0]) for x in indices]
        flat = torch.cat([x.reshape(-1) for x in indices], dim=0)
        x_q = self.quantize.indices_to_codes(flat).to(next(self.decoder.parameters()).dtype)
        return self.decode(x_q, token_counts, grids)

    def forward(self, x):
        x = list(x)
        sizes = {tuple(vid.shape[1:]) for vid in x}
        if len(sizes) > 1:
            raise ValueError(f"TiTok.forward stacks its outputs, so its clips must have one size; got {sorted(sizes)}.  For clips of different sizes "
                             "call encode(x, token_counts) and decode(x_q, token_counts, grids), which return one clip each")
        token_counts = [self.TOKENS for _ in x]
        grids = [tuple(vid.shape[1:]) for vid in x]
        x_q, _ = self.encode(x, token_counts)
        return {"pred_frames": torch.stack(self.decode(x_q, token_counts, grids), dim=0)}
