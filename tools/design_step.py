"""Training-step time of `autoencoder_design` (design.py: rotary RMS-norm blocks with learned residual scales, cross attention in the decoder).

Prints ONE JSON line and writes it to --out (default profiles/design_step.json):
  * ms per forward + backward and clips/s at the model's hard-coded geometry (16x128x128 clips, 1024 + 1024 tokens in the encoder and the
    decoder, 256 + 256 in the first-frame encoder, 8 + 4 + 8 blocks of width 512) for each --clips, timed with device events behind a
    synchronised warm-up, median of --rounds rounds;
  * with --torch, alternating with it in every round, the same model written in stock torch ops under autocast(bf16) on the same device:
    nn.Linear, F.scaled_dot_product_attention, the complex-multiply rotary, RMSNorm and FSQ as elementwise ops, the kernel = stride convolutions
    as a patch reshape around a Linear.  That model lives in THIS TOOL ONLY -- it is the yardstick, not a product path;
  * the fused q/k pass (vt_qkrms_rope_fwd / _bwd) against the chain of existing passes it replaces (vt_head_rmsnorm_* of q and of k, a copy of
    v, vt_rope_rotate), alternating in one process, at the row count of the encoder for each --clips.
Progress goes to stderr.

  python tools/design_step.py --clips 4 --steps 5 --warmup 2 --rounds 3 --torch
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

NAME = "autoencoder_design"
WIDTH, HEADS, DEPTH, TOKENS, COND, GRID, PATCH, LEVELS, MLP = 512, 8, 8, 1024, 256, [4, 16, 16], (4, 8, 8), (8, 8, 8, 5, 5, 5), 4


# ---------------------------------------------------------------------------------------------- the stock-torch yardstick
class TRMSNorm(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return (x * x.float().pow(2).mean(-1, keepdim=True).add(1e-6).rsqrt()).to(x.dtype) * self.weight


def rotary(x, freqs):
    with torch.autocast("cuda", enabled=False):
        xc = torch.view_as_complex(x.float().reshape(*x.shape[:-1], -1, 2))
        return torch.view_as_real(xc * freqs.unsqueeze(-2)).flatten(-2).type_as(x)


class TAttention(nn.Module):
    def __init__(self, cross):
        super().__init__()
        self.cross = cross
        self.norm, self.q_norm, self.k_norm = TRMSNorm(WIDTH), TRMSNorm(64), TRMSNorm(64)
        self.to_gate, self.out_proj = nn.Linear(WIDTH, WIDTH, bias=False), nn.Linear(WIDTH, WIDTH, bias=False)
        if cross:
            self.norm_kv, self.to_q, self.to_kv = TRMSNorm(WIDTH), nn.Linear(WIDTH, WIDTH, bias=False), nn.Linear(WIDTH, 2 * WIDTH, bias=False)
        else:
            self.to_qkv = nn.Linear(WIDTH, 3 * WIDTH, bias=False)

    def forward(self, x, freqs, context=None):
        xn = self.norm(x)
        gate = self.to_gate(xn)
        if self.cross:
            q, (k, v) = self.to_q(xn), self.to_kv(self.norm_kv(context)).chunk(2, dim=-1)
        else:
            q, k, v = self.to_qkv(xn).chunk(3, dim=-1)
        q, k, v = (t.unflatten(-1, (HEADS, 64)) for t in (q, k, v))
        q, k = self.q_norm(q).to(v.dtype), self.k_norm(k).to(v.dtype)
        if not self.cross:
            q, k = rotary(q, freqs), rotary(k, freqs)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).flatten(-2)
        return self.out_proj(o * torch.sigmoid(gate))


class TBlock(nn.Module):
    def __init__(self, cross, i):
        super().__init__()
        inner = vt.design.ffn_inner_dim(WIDTH, MLP)
        self.sa, self.ca = TAttention(False), (TAttention(True) if cross else None)
        self.ffn_norm, self.fc1, self.fc2 = TRMSNorm(WIDTH), nn.Linear(WIDTH, 2 * inner, bias=False), nn.Linear(inner, WIDTH, bias=False)
        self.scales = nn.ParameterList([nn.Parameter(torch.tensor(1.0 / math.sqrt(2 * i + 1))) for _ in range(3 if cross else 2)])

    def forward(self, x, freqs, context=None):
        x = x + self.scales[0] * self.sa(x, freqs)
        if self.ca is not None:
            x = x + self.scales[2] * self.ca(x, None, context)
        a, g = self.fc1(self.ffn_norm(x)).chunk(2, dim=-1)
        return x + self.scales[1] * self.fc2(F.gelu(g) * a)


class TStack(nn.Module):
    def __init__(self, depth, cross):
        super().__init__()
        self.layers, self.final = nn.ModuleList(TBlock(cross, i) for i in range(depth)), TRMSNorm(WIDTH)

    def forward(self, x, freqs, context=None):
        for b in self.layers:
            x = b(x, freqs, context)
        return self.final(x)


class TorchModel(nn.Module):
    def __init__(self, freqs_main, freqs_first):
        super().__init__()
        self.register_buffer("freqs_main", freqs_main, persistent=False)
        self.register_buffer("freqs_first", freqs_first, persistent=False)
        kp = 3 * PATCH[0] * PATCH[1] * PATCH[2]
        self.enc_in, self.first_in = nn.Linear(kp, WIDTH), nn.Linear(kp // PATCH[0], WIDTH)      # the two kernel = stride convolutions on patch rows
        self.enc_q, self.first_q = nn.Parameter(torch.randn(1, TOKENS, WIDTH) * WIDTH ** -0.5), nn.Parameter(torch.randn(1, COND, WIDTH) * WIDTH ** -0.5)
        self.dec_q = nn.Parameter(torch.randn(1, GRID[0] * GRID[1] * GRID[2], WIDTH) * WIDTH ** -0.5)
        self.enc, self.first, self.dec = TStack(DEPTH, False), TStack(max(DEPTH // 2, 2), False), TStack(DEPTH, True)
        self.enc_out, self.first_out = nn.Linear(WIDTH, len(LEVELS)), nn.Linear(WIDTH, len(LEVELS))
        self.dec_in, self.dec_cond = nn.Linear(len(LEVELS), WIDTH), nn.Linear(len(LEVELS), WIDTH)
        self.ad_norm, self.ad1, self.ad2 = TRMSNorm(WIDTH), nn.Linear(WIDTH, WIDTH, bias=False), nn.Linear(WIDTH, WIDTH, bias=False)
        self.dec_out = nn.Linear(WIDTH, kp)

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
        first = video[:, :, 0].reshape(B, 3, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, -1)
        x = self.enc(torch.cat([self.enc_q.expand(B, -1, -1), self.enc_in(rows)], dim=1), self.freqs_main)
        f = self.first(torch.cat([self.first_q.expand(B, -1, -1), self.first_in(first)], dim=1), self.freqs_first)
        main_q, first_q = self.fsq(self.enc_out(x[:, :TOKENS])), self.fsq(self.first_out(f[:, :COND]))
        c = self.dec_cond(first_q)
        context = c + self.ad2(F.silu(self.ad1(self.ad_norm(c))))
        y = self.dec(torch.cat([self.dec_in(main_q), self.dec_q.expand(B, -1, -1)], dim=1), self.freqs_main, context)
        out = self.dec_out(y[:, TOKENS:]).reshape(B, gt, gh, gw, pt, ph, pw, 3).permute(0, 7, 1, 4, 2, 5, 3, 6)
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
    print(f"[design_step] {msg}", file=sys.stderr, flush=True)


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
        note(f"{what}: round {r} " + ", ".join(f"{n} {t[-1]:.3f} ms" for n, t in times.items()))
    return {name: {"ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)} for name, ts in times.items()}


def qk_pass_legs(clips, steps, warmup, rounds):
    """the fused q/k pass against the chain of passes it replaces, forward and backward, on the encoder's [clips * 2048, 4 * 512] projection"""
    hip = vt.hip
    L, H, D = TOKENS + GRID[0] * GRID[1] * GRID[2], HEADS, WIDTH
    M = clips * L
    qkvg = torch.from_numpy(gen.normal((M, 4 * D), 11)).cuda().to(torch.bfloat16)
    dqkv = torch.from_numpy(gen.normal((M, 3 * D), 12)).cuda().to(torch.bfloat16)
    w = torch.ones(64, device="cuda")
    cos, sin = (t.cuda() for t in vt.titok.rope_tables(TOKENS, GRID))
    out, dqkvg, rot = torch.empty(M, 3 * D, device="cuda", dtype=torch.bfloat16), torch.empty_like(qkvg), torch.empty_like(dqkv)

    def fused_fwd():
        hip.qkrms_rope_fwd(qkvg, L, H, w, w, 1e-6, cos, sin, out=out)

    def chain_fwd():
        hip.check(hip.lib().vt_head_rmsnorm_fwd(hip.ptr(qkvg), 4 * D, hip.ptr(w), 1e-6, M, H, hip.ptr(out), 3 * D, hip.stream()), "q")
        hip.check(hip.lib().vt_head_rmsnorm_fwd(hip.ptr(qkvg[:, D:]), 4 * D, hip.ptr(w), 1e-6, M, H, hip.ptr(out[:, D:]), 3 * D, hip.stream()), "k")
        out[:, 2 * D:].copy_(qkvg[:, 2 * D:3 * D])
        hip.rope_rotate(out, L, H, cos, sin)

    def fused_bwd():
        hip.qkrms_rope_bwd(qkvg, dqkv, L, H, w, w, 1e-6, cos, sin, dqkvg)

    def chain_bwd():
        rot.copy_(dqkv)
        hip.rope_rotate(rot, L, H, cos, sin, conjugate=True)
        hip.head_rmsnorm_bwd(rot[:, :D], qkvg[:, :D], w, 1e-6, H, dx=dqkvg[:, :D])
        hip.head_rmsnorm_bwd(rot[:, D:2 * D], qkvg[:, D:2 * D], w, 1e-6, H, dx=dqkvg[:, D:2 * D])
        dqkvg[:, 2 * D:3 * D].copy_(rot[:, 2 * D:])

    res = {"rows": M, "width_in": 4 * D}
    res["fwd"] = alternate([("fused", fused_fwd), ("chain", chain_fwd)], warmup + 3, 20 * steps, rounds, f"{clips} clips q/k fwd")
    res["bwd"] = alternate([("fused", fused_bwd), ("chain", chain_bwd)], warmup + 3, 20 * steps, rounds, f"{clips} clips q/k bwd")
    for d in ("fwd", "bwd"):
        res[d]["chain_over_fused"] = round(res[d]["chain"]["ms"] / res[d]["fused"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[4])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg; the legs alternate inside a round")
    ap.add_argument("--torch", action="store_true", help="also time the stock-torch model under autocast(bf16), alternating with the HIP model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "design_step.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    model = vt.make({"name": NAME, "args": {"bottleneck": None, "prior_model": None}}).cuda().train()
    ref = None
    if a.torch:
        fm, ff = vt.titok.rope_tables(TOKENS, GRID), vt.titok.rope_tables(COND, [1] + GRID[1:])
        ref = TorchModel(torch.complex(*fm), torch.complex(*ff)).cuda().train()
    note("models built")
    res = {"metric": f"{NAME} ms per fwd+bwd step (16x128x128 clips)", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "legs": [], "qk_pass": []}
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
        t = alternate(legs, a.warmup, a.steps, a.rounds, f"{clips} clips step")
        leg = {"clips": clips}
        for name, v in t.items():
            leg[name] = {"ms_per_step": v["ms"], "clips_per_s": round(clips * 1000.0 / v["ms"], 2), "ms_min": v["ms_min"], "ms_max": v["ms_max"]}
        if ref is not None:
            leg["torch_over_hip"] = round(t["torch_autocast_bf16"]["ms"] / t["hip"]["ms"], 3)
        res["legs"].append(leg)
        res["qk_pass"].append(dict(clips=clips, **qk_pass_legs(clips, a.steps, a.warmup, a.rounds)))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
