"""Training-step time of `autoencoder_dualpatch` (dualpatch.py: first-frame (1, 8, 8) and rest (3, 8, 8) patches in one pass, the gated layer stack).

Prints ONE JSON line and writes it to --out (default profiles/dualpatch_step.json):
  * ms per forward + backward and clips/s at the model's hard-coded geometry (16x128x128 clips, 1024 latent + 256 first-frame + 1280 rest tokens,
    5 + 5 layers of width 768) for each --clips, timed with device events behind a synchronised warm-up, median and range of --rounds rounds;
  * with --torch, alternating with it in every round, the same model written in stock torch ops under autocast(bf16) on the same device:
    nn.Conv3d / nn.ConvTranspose3d on the temporal slices, nn.Linear, nn.LayerNorm, F.scaled_dot_product_attention, FSQ as elementwise ops,
    torch.cat for the stream and the output.  That model lives in THIS TOOL ONLY -- it is the yardstick, not a product path;
  * each copy kernel against the composition it replaces, alternating in one process, at each --clips: vt_patchify_dual against two
    .contiguous() slice copies + two vt_patchify calls; vt_unpatchify_dual against two vt_unpatchify calls + torch.cat along T.
Progress goes to stderr.

  python tools/dualpatch_step.py --clips 4 --steps 3 --warmup 2 --rounds 3 --torch
"""
import argparse
import json
import math
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

NAME = "autoencoder_dualpatch"
WIDTH, HEADS, DEPTH, TOKENS, LEVELS, MLP = 768, 12, 5, 1024, (8, 8, 8, 5, 5, 5), 2.0
T, S, T0, PT0, PT1, P = 16, 128, 1, 1, 3, 8
N0, N1 = (S // P) ** 2, (T - T0) // PT1 * (S // P) ** 2


# ---------------------------------------------------------------------------------------------- the stock-torch yardstick
class TLayer(nn.Module):
    def __init__(self):
        super().__init__()
        inner = vt.titok.ffd_inner_dim(WIDTH, MLP)
        self.to_qkv, self.out_proj = nn.Linear(WIDTH, 4 * WIDTH, bias=False), nn.Linear(WIDTH, WIDTH, bias=False)
        self.q_norm, self.k_norm, self.ln = nn.LayerNorm(64), nn.LayerNorm(64), nn.LayerNorm(WIDTH)
        self.fc1, self.fc2 = nn.Linear(WIDTH, 2 * inner, bias=False), nn.Linear(inner, WIDTH, bias=False)

    def forward(self, x, i):
        q, k, v, gate = self.to_qkv(x).chunk(4, dim=-1)
        q, k, v = (t.unflatten(-1, (HEADS, 64)) for t in (q, k, v))
        q, k = self.q_norm(q).to(v.dtype), self.k_norm(k).to(v.dtype)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).flatten(-2)
        x = x + self.out_proj(o * torch.sigmoid(gate))
        a, g = self.fc1(self.ln(x)).chunk(2, dim=-1)
        return (x + self.fc2(F.gelu(g) * a)) * (1 / math.sqrt(i + 1))


class TorchModel(nn.Module):
    def __init__(self):
        super().__init__()
        table = lambda n: nn.Parameter(torch.randn(1, n, WIDTH) * WIDTH ** -0.5)   # noqa: E731
        self.embed0, self.embed1 = nn.Conv3d(3, WIDTH, (PT0, P, P), (PT0, P, P)), nn.Conv3d(3, WIDTH, (PT1, P, P), (PT1, P, P))
        self.pos0, self.pos1, self.latents = table(N0), table(N1), table(TOKENS)
        self.enc, self.dec = nn.ModuleList(TLayer() for _ in range(DEPTH)), nn.ModuleList(TLayer() for _ in range(DEPTH))
        self.enc_out, self.dec_in = nn.Linear(WIDTH, len(LEVELS)), nn.Linear(len(LEVELS), WIDTH)
        self.latent_pos, self.q0, self.q1 = table(TOKENS), table(N0), table(N1)
        self.un0, self.un1 = nn.ConvTranspose3d(WIDTH, 3, (PT0, P, P), (PT0, P, P)), nn.ConvTranspose3d(WIDTH, 3, (PT1, P, P), (PT1, P, P))

    def fsq(self, z):
        lv = torch.tensor(LEVELS, device=z.device, dtype=torch.float32)
        half_l = (lv - 1) * (1 + 1e-3) / 2
        offset = torch.where(lv.remainder(2) == 0, 0.5, 0.0)
        bounded = (z.float() + (offset / half_l).atanh()).tanh() * half_l - offset
        return (bounded + (bounded.round() - bounded).detach()) / torch.floor(lv / 2)

    def forward(self, video):
        B, g = video.shape[0], S // P
        f0 = self.embed0(video[:, :, :T0]).flatten(2).transpose(1, 2) + self.pos0
        f1 = self.embed1(video[:, :, T0:]).flatten(2).transpose(1, 2) + self.pos1
        x = torch.cat([self.latents.expand(B, -1, -1), f0, f1], dim=1)
        for i, layer in enumerate(self.enc):
            x = layer(x, i)
        codes = self.fsq(self.enc_out(x[:, :TOKENS]))
        y = torch.cat([self.dec_in(codes) + self.latent_pos, self.q0.expand(B, -1, -1), self.q1.expand(B, -1, -1)], dim=1)
        for i, layer in enumerate(self.dec):
            y = layer(y, i)
        y0 = y[:, TOKENS:TOKENS + N0].transpose(1, 2).reshape(B, WIDTH, T0 // PT0, g, g)
        y1 = y[:, TOKENS + N0:].transpose(1, 2).reshape(B, WIDTH, (T - T0) // PT1, g, g)
        return torch.cat([self.un0(y0), self.un1(y1)], dim=2)


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
    print(f"[dualpatch_step] {msg}", file=sys.stderr, flush=True)


def alternate(legs, warmup, steps, rounds, what):
    for name, fn in legs:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        note(f"{what}: {name} warmed up")
    times = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, fn in legs:
            times[name].append(timed(fn, steps))
        note(f"{what}: round {r} " + ", ".join(f"{n} {t[-1]:.4f} ms" for n, t in times.items()))
    return {name: {"ms": round(statistics.median(ts), 5), "ms_min": round(min(ts), 5), "ms_max": round(max(ts), 5)} for name, ts in times.items()}


def copy_kernel_legs(clips, steps, warmup, rounds):
    """each two-segment copy kernel against the composition of slice copies, one-segment kernels and torch.cat it replaces; outputs are allocated
    inside every leg, as the Functions do"""
    hip = vt.hip
    B = clips
    video = torch.from_numpy(gen.video_clips(B, T, S, 70 + clips)).cuda()
    r0 = torch.from_numpy(gen.normal((B * N0, 3 * PT0 * P * P), 71)).cuda()
    r1 = torch.from_numpy(gen.normal((B * N1, 3 * PT1 * P * P), 72)).cuda()

    def dual_patchify():
        hip.patchify_dual(video, T0, PT0, PT1, P, P)

    def composed_patchify():
        hip.patchify(video[:, :, :T0].contiguous(), PT0, P)
        hip.patchify(video[:, :, T0:].contiguous(), PT1, P)

    def dual_unpatchify():
        hip.unpatchify_dual(r0, r1, B, 3, T, S, S, T0, PT0, PT1, P, P)

    def composed_unpatchify():
        torch.cat([hip.unpatchify(r0, B, 3, T0, S, PT0, P), hip.unpatchify(r1, B, 3, T - T0, S, PT1, P)], dim=2)

    res = {"clips": clips, "video_bytes": video.numel() * 4}
    res["patchify"] = alternate([("dual", dual_patchify), ("composed", composed_patchify)], warmup + 3, 50 * steps, rounds, f"{clips} clips patchify")
    res["unpatchify"] = alternate([("dual", dual_unpatchify), ("composed", composed_unpatchify)], warmup + 3, 50 * steps, rounds, f"{clips} clips unpatchify")
    for d in ("patchify", "unpatchify"):
        res[d]["composed_over_dual"] = round(res[d]["composed"]["ms"] / res[d]["dual"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[4])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg; the legs alternate inside a round")
    ap.add_argument("--torch", action="store_true", help="also time the stock-torch model under autocast(bf16), alternating with the HIP model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dualpatch_step.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    model = vt.make({"name": NAME, "args": {"bottleneck": None, "prior_model": None}}).cuda().train()
    ref = TorchModel().cuda().train() if a.torch else None
    note("models built")
    res = {"metric": f"{NAME} ms per fwd+bwd step (16x128x128 clips)", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "legs": [], "copy_kernels": []}
    for clips in a.clips:
        video = torch.from_numpy(gen.video_clips(clips, T, S, 60 + clips)).cuda()

        def hip_step():
            model.zero_grad(set_to_none=True)
            model(video)["pred_frames"].square().mean().backward()

        def torch_step():
            ref.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = ref(video)
            out.float().square().mean().backward()

        legs = [("hip", hip_step)] + ([("torch_autocast_bf16", torch_step)] if ref is not None else [])
        t = alternate(legs, a.warmup, a.steps, a.rounds, f"{clips} clips step")
        leg = {"clips": clips}
        for name, v in t.items():
            leg[name] = {"ms_per_step": v["ms"], "clips_per_s": round(clips * 1000.0 / v["ms"], 2), "ms_min": v["ms_min"], "ms_max": v["ms_max"]}
        if ref is not None:
            leg["torch_over_hip"] = round(t["torch_autocast_bf16"]["ms"] / t["hip"]["ms"], 3)
        res["legs"].append(leg)
        res["copy_kernels"].append(copy_kernel_legs(clips, a.steps, a.warmup, a.rounds))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
