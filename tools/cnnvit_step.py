"""Forward + backward time of the `autoencoder_cnnvit` ends (cnnvit.py: Encoder_cnn -> Decoder_cnn, ch=32, ch_mult=(1,2,4,4), z_channels=1024)
at 4 clips of 16x128x128, and the three convolution products at the four pyramid levels.

Prints ONE JSON line and writes it to --out (default profiles/cnnvit_step.json):
  * ms per forward + backward of the HIP ends and, alternating with it in every round, of the same modules (the same parameters) evaluated in
    stock torch ops under autocast(bf16) with channels_last_3d tensors: F.group_norm, F.silu, F.conv3d, F.interpolate, F.scaled_dot_product_attention.
    That evaluation lives in THIS TOOL ONLY -- it is the yardstick, not a product path.  Device events behind a synchronised warm-up; median
    [min, max] over --rounds rounds of --steps steps;
  * the 3x3x3 convolution flops of one step (forward + input gradient + weight gradient) and the rate they are done at;
  * per level (32 ch at 16x128x128, 64 at 16x64x64, 128 at 8x32x32, 128 at 4x16x16; 4 clips): ms and TFLOP/s of vt_conv3d_fwd, vt_conv3d_dgrad and
    vt_conv3d_wgrad, and the bytes each must move at least (input + output once), as a rate.
Progress goes to stderr.

  python tools/cnnvit_step.py --steps 3 --warmup 2 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import video_tokenizer_amd as vt  # noqa: E402
from video_tokenizer_amd import cnnvit, hip  # noqa: E402

CL = torch.channels_last_3d
FLOPS = [0]


# ---- the yardstick: the same module tree in stock torch ops ------------------------------------------------------------------------------------
def t_conv(conv, x):
    y = F.conv3d(x, conv.weight, conv.bias, stride=conv.stride, padding=conv.padding)
    if conv.kernel_size == (3, 3, 3):
        FLOPS[0] += 2 * 27 * conv.in_channels * conv.out_channels * y.numel() // conv.out_channels
    return y


def t_norm(norm, x, swish):
    y = F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)
    return F.silu(y) if swish else y


def t_res(m, x):
    h = t_conv(m.conv1, t_norm(m.norm1, x, True))
    h = t_conv(m.conv2, t_norm(m.norm2, h, True))
    if m.in_channels != m.out_channels:
        x = t_conv(m.conv_shortcut if m.use_conv_shortcut else m.nin_shortcut, x)
    return x + h


def t_attn(m, x):
    h = t_norm(m.norm, x, False)
    B, C, T, H, W = h.shape
    q, k, v = (t_conv(c, h).reshape(B, 1, C, T * H * W).transpose(2, 3) for c in (m.q, m.k, m.v))
    o = F.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(B, C, T, H, W)
    return x + t_conv(m.proj_out, o)


def t_any(m, x):
    return t_attn(m, x) if isinstance(m, cnnvit.AttnBlock3D) else t_res(m, x)


def t_levels(m, h, n_blocks, last):
    for i, block in enumerate(m.conv_blocks):
        for j in range(n_blocks):
            h = t_res(block.res[j], h)
            if m.use_attn and len(block.attn) > 0:
                h = t_attn(block.attn[j], h)
        if i != m.num_resolutions - 1:
            h = t_conv(block.downsample.conv, h) if last == "down" else t_conv(block.upsample.conv, F.interpolate(h, scale_factor=block.upsample.scale_factor, mode="nearest"))
    return h


def t_encoder(m, x):
    h = t_levels(m, t_conv(m.conv_in, x), m.num_res_blocks, "down")
    for b in m.mid:
        h = t_any(b, h)
    return t_conv(m.conv_out, t_norm(m.norm_out, h, True))


def t_decoder(m, z):
    h = t_conv(m.conv_in, z)
    for b in m.mid:
        h = t_any(b, h)
    h = t_levels(m, h, m.num_res_blocks + 1, "up")
    return t_conv(m.conv_out, t_norm(m.norm_out, h, True))


# ---- timing ----------------------------------------------------------------------------------------------------------------------------------
def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(samples):
    return {"ms_per_step": round(statistics.median(samples), 4), "ms_min": round(min(samples), 4), "ms_max": round(max(samples), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnnvit_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    kw = dict(ch=32, ch_mult=(1, 2, 4, 4), z_channels=1024)
    enc, dec = vt.Encoder_cnn(**kw).cuda(), vt.Decoder_cnn(**kw).cuda()
    params = list(enc.parameters()) + list(dec.parameters())
    video = torch.rand(a.clips, 3, 16, 128, 128, device="cuda") * 2 - 1
    cot = torch.randn(a.clips, 3, 16, 128, 128, device="cuda")

    def clear():
        for p in params:
            p.grad = None

    def hip_step():
        clear()
        dec(enc(video)).backward(cot)

    video_cl = video.contiguous(memory_format=CL)

    def torch_step():
        clear()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = t_decoder(dec, t_encoder(enc, video_cl))
        y.float().backward(cot)

    sides = {"hip": hip_step} if a.no_torch else {"hip": hip_step, "torch_autocast_bf16_channels_last_3d": torch_step}
    for name, fn in sides.items():
        print(f"warm-up {name}", file=sys.stderr)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
    if not a.no_torch:
        FLOPS[0] = 0
        torch_step()
        torch.cuda.synchronize()
    conv_flops = 3 * FLOPS[0]                                              # forward + input gradient + weight gradient (conv_in's input gradient included)
    samples = {k: [] for k in sides}
    for r in range(a.rounds):
        for name, fn in sides.items():
            samples[name].append(timed(fn, a.steps))
            print(f"round {r} {name}: {samples[name][-1]:.3f} ms", file=sys.stderr)
    res = {"metric": "autoencoder_cnnvit ends (Encoder_cnn + Decoder_cnn, ch=32, z=1024) ms per fwd+bwd step", "device": torch.cuda.get_device_name(0),
           "clips": a.clips, "clip": [16, 128, 128], "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    for name in sides:
        res[name] = summary(samples[name])
    if not a.no_torch:
        res["torch_over_hip"] = round(res["torch_autocast_bf16_channels_last_3d"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
        res["conv3x3x3_gflop_per_step"] = round(conv_flops / 1e9, 1)
        res["hip_conv_tflops_over_whole_step"] = round(conv_flops / res["hip"]["ms_per_step"] / 1e9, 1)

    # the three products at the four pyramid levels
    levels = []
    for C, (T, H, W) in ((32, (16, 128, 128)), (64, (16, 64, 64)), (128, (8, 32, 32)), (128, (4, 16, 16))):
        x = torch.randn(a.clips, T, H, W, C, device="cuda").to(torch.bfloat16)
        dy = torch.randn_like(x)
        w = torch.randn(C, C, 3, 3, 3, device="cuda") / (27 * C) ** 0.5
        bias = torch.zeros(C, device="cuda")
        wp, wd = hip.conv3d_pack_weight(w, C, C), hip.conv3d_pack_weight(w, C, C, for_dgrad=True)
        out, dw = torch.empty_like(x), torch.empty_like(w)
        flops, nbytes = 2 * 27 * C * C * x.numel() // C, 2 * x.numel() * 2
        row = {"channels": C, "clip": [T, H, W], "gflop": round(flops / 1e9, 2), "activation_mb": round(x.numel() * 2 / 2 ** 20, 1)}
        for name, fn in (("fwd", lambda: hip.conv3d_fwd(x, wp, bias, C, out=out)), ("dgrad", lambda: hip.conv3d_dgrad(dy, wd, (T, H, W), C, dx=out)),
                         ("wgrad", lambda: hip.conv3d_wgrad(x, dy, dw=dw))):
            fn()
            torch.cuda.synchronize()
            ms = statistics.median(timed(fn, 3) for _ in range(3))
            row[name] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1), "min_traffic_gb_per_s": round(nbytes / ms / 1e6, 1)}
        levels.append(row)
        print(json.dumps(row), file=sys.stderr)
    res["conv_products"] = levels
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
