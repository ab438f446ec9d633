"""Training-step time of `autoencoder_convpatchify_simplytransformer` (rotary block stacks on vt_stack_forward_rotary / _backward_rotary).

Prints ONE JSON line: ms per forward + backward and clips/s at the model's hard-coded geometry (16x128x128 clips, 1024 patch + 1024 latent
tokens, 12 + 12 blocks of width 768) for each --clips, timed with device events behind a synchronised warm-up, median of --rounds rounds.
With --torch every round also times the same model written in stock torch ops under autocast(bf16) on the same device, the two legs
alternating: nn.Linear / nn.LayerNorm, F.scaled_dot_product_attention, the complex-multiply rotary, FSQ as elementwise ops, and the two
kernel = stride convolutions as a patch reshape around a Linear (the same arithmetic; the library convolutions spend minutes searching
for an algorithm the first time they see these shapes on a fresh machine).  That model lives in THIS TOOL ONLY -- it is the yardstick,
not a product path.  Progress goes to stderr.  Also the rotary kernel's bytes per
call (q and k read and written, the two tables) for reading a kernel trace.

  python tools/simple_step.py --clips 4 --steps 5 --warmup 2 --rounds 3 --torch
For the kernel trace, a short run of its own under the profiler:
  rocprofv3 --kernel-trace --stats -d <dir> -o simple -- python tools/simple_step.py --clips 4 --steps 3 --warmup 2 --rounds 1
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import video_tokenizer_amd as vt  # noqa: E402
from oracle import inputs as gen  # noqa: E402

NAME = "autoencoder_convpatchify_simplytransformer"
WIDTH, HEADS, DEPTH, TOKENS, GRID, PATCH, LEVELS = 768, 12, 12, 1024, [4, 16, 16], (4, 8, 8), (8, 8, 8, 5, 5, 5)


# ---------------------------------------------------------------------------------------------- the stock-torch yardstick
class TorchBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(WIDTH), nn.LayerNorm(WIDTH)
        self.qkv, self.proj = nn.Linear(WIDTH, 3 * WIDTH, bias=False), nn.Linear(WIDTH, WIDTH)
        self.fc1, self.fc2 = nn.Linear(WIDTH, 4 * WIDTH), nn.Linear(4 * WIDTH, WIDTH)

    @staticmethod
    def rotary(x, freqs):
        with torch.autocast("cuda", enabled=False):
            xc = torch.view_as_complex(x.float().reshape(*x.shape[:-1], -1, 2))
            return torch.view_as_real(xc * freqs.unsqueeze(-2)).flatten(-2).type_as(x)

    def forward(self, x, freqs):
        B, N, C = x.shape
        q, k, v = self.qkv(self.norm1(x)).reshape(B, N, 3, HEADS, C // HEADS).unbind(2)
        q, k = self.rotary(q, freqs), self.rotary(k, freqs)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2))
        x = x + self.proj(o.transpose(1, 2).reshape(B, N, C))
        return x + self.fc2(F.gelu(self.fc1(self.norm2(x))))


class TorchModel(nn.Module):
    def __init__(self, freqs):
        super().__init__()
        self.register_buffer("freqs", freqs, persistent=False)
        self.enc_in = nn.Linear(3 * PATCH[0] * PATCH[1] * PATCH[2], WIDTH)          # Conv3d(3, WIDTH, PATCH, stride PATCH) on patch rows
        self.enc_mask, self.dec_mask = nn.Parameter(torch.randn(1, 1, 1) * WIDTH ** -0.5), nn.Parameter(torch.randn(1, 1, 1) * WIDTH ** -0.5)
        self.enc, self.dec = nn.ModuleList(TorchBlock() for _ in range(DEPTH)), nn.ModuleList(TorchBlock() for _ in range(DEPTH))
        self.enc_norm, self.dec_norm = nn.LayerNorm(WIDTH), nn.LayerNorm(WIDTH)
        self.enc_out, self.dec_in = nn.Linear(WIDTH, len(LEVELS)), nn.Linear(len(LEVELS), WIDTH)
        self.dec_out = nn.Linear(WIDTH, 3 * PATCH[0] * PATCH[1] * PATCH[2])         # ConvTranspose3d(WIDTH, 3, PATCH, stride PATCH)

    def fsq(self, z):
        lv = torch.tensor(LEVELS, device=z.device, dtype=torch.float32)
        half_l = (lv - 1) * (1 + 1e-3) / 2
        offset = torch.where(lv.remainder(2) == 0, 0.5, 0.0)
        bounded = (z.float() + (offset / half_l).atanh()).tanh() * half_l - offset
        return (bounded + (bounded.round() - bounded).detach()) / torch.floor(lv / 2)

    def forward(self, video):
        B = video.shape[0]
        (pt, ph, pw), (gt, gh, gw) = PATCH, GRID
        rows = video.reshape(B, 3, gt, pt, gh, ph, gw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, gt * gh * gw, -1)
        x = self.enc_in(rows)
        x = torch.cat([self.enc_mask.expand(B, TOKENS, WIDTH).to(x.dtype), x], dim=1)
        for b in self.enc:
            x = b(x, self.freqs)
        codes = self.fsq(self.enc_out(self.enc_norm(x)[:, :TOKENS]))
        y = self.dec_in(codes)
        y = torch.cat([y, self.dec_mask.expand(B, GRID[0] * GRID[1] * GRID[2], WIDTH).to(y.dtype)], dim=1)
        for b in self.dec:
            y = b(y, self.freqs)
        y = self.dec_norm(y)[:, TOKENS:]
        out = self.dec_out(y).reshape(B, gt, gh, gw, 3, pt, ph, pw).permute(0, 4, 1, 5, 2, 6, 3, 7)
        return out.reshape(B, 3, gt * pt, gh * ph, gw * pw)


# ---------------------------------------------------------------------------------------------- timing
def timed(step, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def note(msg):
    print(f"[simple_step] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[4])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg; the legs alternate inside a round")
    ap.add_argument("--torch", action="store_true", help="also time the stock-torch model under autocast(bf16), alternating with the HIP model")
    a = ap.parse_args()
    torch.manual_seed(0)
    model = vt.make({"name": NAME, "args": {"bottleneck": None, "prior_model": None}}).cuda().train()
    ref = None
    if a.torch:
        cos, sin = vt.titok.rope_tables(TOKENS, GRID)
        ref = TorchModel(torch.complex(cos, sin)).cuda().train()
    note("models built")
    res = {"metric": f"{NAME} ms per fwd+bwd step (16x128x128 clips)", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "legs": []}
    for clips in a.clips:
        video = torch.from_numpy(gen.video_clips(clips, 16, 128, 60 + clips)).cuda()

        def hip_step():
            model.zero_grad(set_to_none=True)
            model(video)["pred_frames"].square().mean().backward()

        def torch_step():
            ref.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = ref(video)
            out.float().square().mean().backward()

        legs = [("hip", hip_step)] + ([("torch_autocast_bf16", torch_step)] if ref is not None else [])
        for name, fn in legs:
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            note(f"{clips} clips: {name} warmed up")
        times = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in legs:
                times[name].append(timed(fn, a.steps))
            note(f"{clips} clips: round {r} " + ", ".join(f"{n} {t[-1]:.1f} ms" for n, t in times.items()))
        M, D = clips * (TOKENS + GRID[0] * GRID[1] * GRID[2]), WIDTH
        leg = {"clips": clips, "rope_bytes_per_call": 2 * M * 2 * D * 2 + 2 * (M // clips) * 32 * 4, "rope_calls_per_step": 4 * DEPTH}
        for name, ts in times.items():
            med = statistics.median(ts)
            leg[name] = {"ms_per_step": round(med, 3), "clips_per_s": round(clips * 1000.0 / med, 2), "ms_min": round(min(ts), 3),
                         "ms_max": round(max(ts), 3)}
        if ref is not None:
            leg["torch_over_hip"] = round(statistics.median(times["torch_autocast_bf16"]) / statistics.median(times["hip"]), 3)
        res["legs"].append(leg)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
