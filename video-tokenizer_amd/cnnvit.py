"""The 3D ResNet ends of the reference's `autoencoder_cnnvit` (models/model_cnnvit/base/cnnvit.py) on the MI355X kernels: ResnetBlock3D,
AttnBlock3D, Downsample3D, Upsample3D, Encoder_cnn and Decoder_cnn, class for class.

Same constructor keywords and defaults, module tree, state-dict keys and shapes as the reference, and torch's default init (the outer model
applies its own `init_weights`).  Every parameter lives in the nn.Conv3d / nn.GroupNorm the reference has at that place; the forwards run on
csrc/vt_conv3d.hip and csrc/vt_groupnorm.hip through functional.Conv3x3x3, GroupNormSwish and UpsampleNearest, the 1x1x1 convolutions
(nin_shortcut, q, k, v, proj_out) as vt_gemm_nt on the [B T H W, C] view through functional.Linear.

Modules take and return logical [B, C, T, H, W] tensors; between layers these are bf16 in torch.channels_last_3d, i.e. [B, T, H, W, C] in
memory, so `rearrange(x, 'b c t h w -> b (t h w) c')` at the boundary to the token stack is a view.  Encoder_cnn takes the fp32 video (its 3
channels are zero-padded to 16 by the layout pass and the weight pack), Decoder_cnn returns fp32 holding bf16 values.  Rounding points = the
reference under autocast(bf16): convolution outputs and residual sums are bf16, GroupNorm and swish are computed in fp32 from bf16 and rounded
once, activation gradients are bf16, parameter gradients fp32.

AttnBlock3D's attention core is one head of dimension C over T H W positions; the library's attention kernels are head-dim 64 only, so the core
runs F.scaled_dot_product_attention on the GPU as torch glue (default scale C^-1/2 = the reference's; in fp32 from the bf16 q, k, v and
rounded to bf16 once: it is 1 GFLOP at four clips of the default size), as does the residual add behind proj_out.  GPU tensors only;
dropout > 0 raises; channel counts must be multiples of 16 (3 at the video ends) and of 16 groups.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .functional import ChannelsLastToVideo, Conv3x3x3, GroupNormSwish, Linear as LinearFn, UpsampleNearest, VideoToChannelsLast, _cl, _logical


def Normalize(in_channels, num_groups=16):
    return nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


def _no_dropout(dropout):
    if dropout > 0:
        raise NotImplementedError(f"dropout={dropout}: the HIP ends have no dropout (the reference's default is 0.0)")


def _norm(norm, x, swish):
    return GroupNormSwish.apply(x, norm.weight, norm.bias, norm.num_groups, norm.eps, int(swish))


def _conv(owner, name, x, residual=None):
    conv = owner.get_submodule(name)
    return Conv3x3x3.apply(x, conv.weight, conv.bias, residual, tuple(conv.stride), owner, name)


def _conv1(conv, x):
    """a 1x1x1 nn.Conv3d as a GEMM on the [B T H W, C] view; bf16 in, bf16 out (functional.Linear rounds to bf16 and returns fp32)"""
    xc = _cl(x)
    y = LinearFn.apply(xc.reshape(-1, xc.shape[-1]), conv.weight.reshape(conv.out_channels, conv.in_channels), conv.bias)
    return _logical(y.to(torch.bfloat16).reshape(*xc.shape[:-1], conv.out_channels))


class ResnetBlock3D(nn.Module):
    def __init__(self, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, norm_type='group'):
        super().__init__()
        _no_dropout(dropout)
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv3d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv3d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = nn.Conv3d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = nn.Conv3d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        h = _conv(self, "conv1", _norm(self.norm1, x, True))
        h = _norm(self.norm2, h, True)
        if self.in_channels != self.out_channels:
            x = _conv(self, "conv_shortcut", x) if self.use_conv_shortcut else _conv1(self.nin_shortcut, x)
        return _conv(self, "conv2", h, residual=x)                  # x + conv2(h), both roundings, in the convolution's epilogue


class AttnBlock3D(nn.Module):
    def __init__(self, in_channels, norm_type='group'):
        super().__init__()
        self.norm = Normalize(in_channels)
        self.q = nn.Conv3d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv3d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv3d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv3d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        h = _norm(self.norm, x, False)
        B, C, T, H, W = h.shape
        q, k, v = (_cl(_conv1(m, h)).reshape(B, 1, T * H * W, C).float() for m in (self.q, self.k, self.v))
        o = F.scaled_dot_product_attention(q, k, v)                 # one head of dimension C: torch glue, in fp32 from the bf16 q, k, v
        o = _logical(o.to(torch.bfloat16).reshape(B, T, H, W, C))   # ... and rounded once, like GroupNorm and swish
        return x + _conv1(self.proj_out, o)


class Downsample3D(nn.Module):
    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1)

    def forward(self, x):
        return _conv(self, "conv", x)


class Upsample3D(nn.Module):
    def __init__(self, in_channels, scale_factor):
        super().__init__()
        self.scale_factor = scale_factor
        self.conv = nn.Conv3d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        return _conv(self, "conv", UpsampleNearest.apply(x, tuple(self.scale_factor)))


class Encoder_cnn(nn.Module):
    def __init__(self, in_channels=3, ch=16, ch_mult=(1, 2, 4, 4), num_res_blocks=2, norm_type='group', dropout=0.0, z_channels=256, use_attn=True):
        super().__init__()
        _no_dropout(dropout)
        self.ch = ch
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.use_attn = use_attn
        self.conv_in = nn.Conv3d(in_channels, ch, kernel_size=3, stride=1, padding=1)
        prev_out_dim = ch
        self.conv_blocks = nn.ModuleList()
        downsample_strides = [(1, 2, 2), (2, 2, 2), (2, 2, 2)]
        for i_level in range(self.num_resolutions):
            conv_block = nn.Module()
            res_block = nn.ModuleList()
            if self.use_attn:
                attn_block = nn.ModuleList()
            block_in = prev_out_dim
            block_out = ch * ch_mult[i_level]
            for _ in range(self.num_res_blocks):
                res_block.append(ResnetBlock3D(block_in, block_out, dropout=dropout, norm_type=norm_type))
                block_in = block_out
                if self.use_attn and i_level == self.num_resolutions - 1:
                    attn_block.append(AttnBlock3D(block_in, norm_type))
            conv_block.res = res_block
            if self.use_attn:
                conv_block.attn = attn_block
            if i_level != self.num_resolutions - 1:
                conv_block.downsample = Downsample3D(block_in, block_in, stride=downsample_strides[i_level])
                prev_out_dim = block_in
            self.conv_blocks.append(conv_block)
        self.mid = nn.ModuleList()
        self.mid.append(ResnetBlock3D(block_in, block_in, dropout=dropout, norm_type=norm_type))
        if self.use_attn:
            self.mid.append(AttnBlock3D(block_in, norm_type=norm_type))
        self.mid.append(ResnetBlock3D(block_in, block_in, dropout=dropout, norm_type=norm_type))
        self.norm_out = Normalize(block_in, num_groups=16)
        self.conv_out = nn.Conv3d(block_in, z_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        """x: the fp32 video [B, C, T, H, W] -> logical [B, z_channels, T', H', W'] bf16 channels_last_3d"""
        h = _conv(self, "conv_in", VideoToChannelsLast.apply(x))
        for i_level, block in enumerate(self.conv_blocks):
            for i_block in range(self.num_res_blocks):
                h = block.res[i_block](h)
                if self.use_attn and len(block.attn) > 0:
                    h = block.attn[i_block](h)
            if i_level != self.num_resolutions - 1:
                h = block.downsample(h)
        for mid_block in self.mid:
            h = mid_block(h)
        return _conv(self, "conv_out", _norm(self.norm_out, h, True))


class Decoder_cnn(nn.Module):
    def __init__(self, z_channels=256, ch=16, ch_mult=(1, 2, 4, 4), num_res_blocks=2, norm_type="group", dropout=0.0, out_channels=3, use_attn=True):
        super().__init__()
        _no_dropout(dropout)
        self.ch = ch
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.use_attn = use_attn
        self.out_channels = out_channels
        block_in = ch * ch_mult[self.num_resolutions - 1]
        self.conv_in = nn.Conv3d(z_channels, block_in, kernel_size=3, stride=1, padding=1)
        self.mid = nn.ModuleList()
        self.mid.append(ResnetBlock3D(block_in, block_in, dropout=dropout, norm_type=norm_type))
        if self.use_attn:
            self.mid.append(AttnBlock3D(block_in, norm_type=norm_type))
        self.mid.append(ResnetBlock3D(block_in, block_in, dropout=dropout, norm_type=norm_type))
        upsample_scales = [(2, 2, 2), (2, 2, 2), (1, 2, 2)]
        self.conv_blocks = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            conv_block = nn.Module()
            res_block = nn.ModuleList()
            if self.use_attn:
                attn_block = nn.ModuleList()
            block_out = ch * ch_mult[i_level]
            for _ in range(self.num_res_blocks + 1):
                res_block.append(ResnetBlock3D(block_in, block_out, dropout=dropout, norm_type=norm_type))
                block_in = block_out
                if self.use_attn and i_level == self.num_resolutions - 1:
                    attn_block.append(AttnBlock3D(block_in, norm_type))
            conv_block.res = res_block
            if self.use_attn:
                conv_block.attn = attn_block
            if i_level != 0:
                conv_block.upsample = Upsample3D(block_in, scale_factor=upsample_scales[self.num_resolutions - 1 - i_level])
            self.conv_blocks.append(conv_block)
        self.norm_out = Normalize(block_in, num_groups=16)
        self.conv_out = nn.Conv3d(block_in, out_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, z):
        """z: logical [B, z_channels, T', H', W'] (any float dtype and layout) -> fp32 [B, out_channels, T, H, W] holding bf16 values"""
        h = _conv(self, "conv_in", z)
        for mid_block in self.mid:
            h = mid_block(h)
        for i_level, block in enumerate(self.conv_blocks):
            for i_block in range(self.num_res_blocks + 1):
                h = block.res[i_block](h)
                if self.use_attn and len(block.attn) > 0:
                    h = block.attn[i_block](h)
            if i_level != self.num_resolutions - 1:
                h = block.upsample(h)
        h = _conv(self, "conv_out", _norm(self.norm_out, h, True))
        return ChannelsLastToVideo.apply(h, self.out_channels)
