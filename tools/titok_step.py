"""Training-step time of `titok` (titok_model.py: clips of variable size packed through a grouped-query encoder, FSQ and decoder).

Prints ONE JSON line and writes it to --out (default profiles/titok_step.json):
  * ms per forward + backward and clips/s of the base model (width 768, 12 + 12 layers, 12 query heads over 4 KV heads) for two workloads,
    timed with device events behind a synchronised warm-up, median of --rounds rounds:
      uniform: 4 clips of 16x128x128 with 1024 tokens each;
      mixed:   16x128x128, 8x64x96, 4x128x64, 16x32x32 with 1024 / 256 / 128 / 64 tokens;
  * with --torch, alternating with it in every round, the same model written in stock torch ops under autocast(bf16) on the same device:
    nn.Linear, nn.LayerNorm, per-sequence F.scaled_dot_product_attention with `repeat_interleave`d K / V, the complex-multiply rotary, the
    torch.cat / split packing of the reference, FSQ as elementwise ops.  That model lives in THIS TOOL ONLY -- it is the yardstick, not a
    product path;
  * the one-launch vt_patchify_clips / vt_unpatchify_clips and vt_packed_scatter / vt_packed_gather against their per-clip torch
    constructions (rearrange + cat + cast; split + cat), sides alternating, for both workloads.
Progress goes to stderr.

  python tools/titok_step.py --steps 3 --warmup 2 --rounds 3 --torch
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

PATCH, LEVELS = (4, 8, 8), (8, 8, 8, 5, 5, 5)
WORKLOADS = {
    "uniform": ([(16, 128, 128)] * 4, [1024] * 4),
    "mixed": ([(16, 128, 128), (8, 64, 96), (4, 128, 64), (16, 32, 32)], [1024, 256, 128, 64]),
}


# ---------------------------------------------------------------------------------------------- the stock-torch yardstick
def rotary(x, freqs):
    with torch.autocast("cuda", enabled=False):
        xc = torch.view_as_complex(x.float().reshape(*x.shape[:-1], -1, 2))
        return torch.view_as_real(xc * freqs.unsqueeze(-2)).flatten(-2).type_as(x)


def patch_rows(vid):
    C, T, H, W = vid.shape
    pt, ph, pw = PATCH
    return vid.reshape(C, T // pt, pt, H // ph, ph, W // pw, pw).permute(1, 3, 5, 0, 2, 4, 6).reshape(-1, C * pt * ph * pw)


def unpatch_rows(rows, size, C=3):
    T, H, W = size
    pt, ph, pw = PATCH
    return rows.reshape(T // pt, H // ph, W // pw, C, pt, ph, pw).permute(3, 0, 4, 1, 5, 2, 6).reshape(C, T, H, W)


class TLayer(nn.Module):
    def __init__(self, D, Hq, Hkv, ratio):
        super().__init__()
        self.D, self.Hq, self.Hkv = D, Hq, Hkv
        inner = vt.varlen.ffd(D, ratio)[4].in_features
        self.pre_ln, self.q_norm, self.k_norm, self.ln = nn.LayerNorm(D), nn.LayerNorm(64), nn.LayerNorm(64), nn.LayerNorm(D)
        self.to_qkv, self.out_proj = nn.Linear(D, D + 128 * Hkv, bias=False), nn.Linear(D, D, bias=False)
        self.fc1, self.fc2 = nn.Linear(D, 2 * inner, bias=False), nn.Linear(inner, D, bias=False)

    def forward(self, x, freqs, lens):
        G = 64 * self.Hkv
        q, k, v = self.to_qkv(self.pre_ln(x)).split([self.D, G, G], dim=-1)
        q, k, v = q.unflatten(-1, (self.Hq, 64)), k.unflatten(-1, (self.Hkv, 64)), v.unflatten(-1, (self.Hkv, 64))
        q, k = rotary(self.q_norm(q).to(v), freqs), rotary(self.k_norm(k).to(v), freqs)
        g, out = self.Hq // self.Hkv, []
        for qs, ks, vs in zip(q.split(lens, 0), k.split(lens, 0), v.split(lens, 0)):
            ks, vs = ks.repeat_interleave(g, dim=1), vs.repeat_interleave(g, dim=1)
            out.append(F.scaled_dot_product_attention(qs.transpose(0, 1), ks.transpose(0, 1), vs.transpose(0, 1)).transpose(0, 1))
        x = x + self.out_proj(torch.cat(out, 0).flatten(-2))
        a, gate = self.fc1(self.ln(x)).chunk(2, dim=-1)
        return x + self.fc2(F.gelu(gate) * a)


class TorchModel(nn.Module):
    def __init__(self):
        super().__init__()
        D, depth, (Hq, Hkv), ratio = vt.varlen.get_model_dims("base")
        kp = 3 * math.prod(PATCH)
        self.enc_mask, self.dec_mask = nn.Parameter(torch.randn(1, D) * D ** -0.5), nn.Parameter(torch.randn(1, D) * D ** -0.5)
        self.enc_in, self.enc_post, self.enc_out = nn.Linear(kp, D), nn.LayerNorm(D), nn.Linear(D, len(LEVELS))
        self.dec_in, self.dec_pre, self.dec_out = nn.Linear(len(LEVELS), D), nn.LayerNorm(D), nn.Linear(D, kp)
        self.enc = nn.ModuleList(TLayer(D, Hq, Hkv, ratio) for _ in range(depth))
        self.dec = nn.ModuleList(TLayer(D, Hq, Hkv, ratio) for _ in range(depth))

    def fsq(self, z):
        lv = torch.tensor(LEVELS, device=z.device, dtype=torch.float32)
        half_l = (lv - 1) * (1 + 1e-3) / 2
        offset = torch.where(lv.remainder(2) == 0, 0.5, 0.0)
        bounded = (z.float() + (offset / half_l).atanh()).tanh() * half_l - offset
        return (bounded + (bounded.round() - bounded).detach()) / torch.floor(lv / 2)

    def forward(self, clips, counts, freqs):
        sizes = [tuple(v.shape[1:]) for v in clips]
        gs = [math.prod(d // q for d, q in zip(s, PATCH)) for s in sizes]
        lens = [g + n for g, n in zip(gs, counts)]
        tok = self.enc_in(torch.cat([patch_rows(v) for v in clips], 0)).split(gs, 0)
        x = torch.cat([t for n, rows in zip(counts, tok) for t in (self.enc_mask.repeat(n, 1), rows)], 0)
        for layer in self.enc:
            x = layer(x, freqs, lens)
        z = self.enc_out(self.enc_post(torch.cat([seq[:n] for n, seq in zip(counts, x.split(lens, 0))], 0)))
        tok = self.dec_in(self.fsq(z)).split(counts, 0)
        x = self.dec_pre(torch.cat([t for g, rows in zip(gs, tok) for t in (rows, self.dec_mask.repeat(g, 1))], 0))
        for layer in self.dec:
            x = layer(x, freqs, lens)
        rows = self.dec_out(torch.cat([seq[n:] for n, seq in zip(counts, x.split(lens, 0))], 0))
        return [unpatch_rows(r, s) for r, s in zip(rows.split(gs, 0), sizes)]


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
    print(f"[titok_step] {msg}", file=sys.stderr, flush=True)


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
    return {name: {"ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)} for name, ts in times.items()}


def movement_legs(clips, counts, steps, warmup, rounds, what):
    """the one-launch data movement against the per-clip torch constructions of the reference, at the workload's sizes and width 768"""
    hip = vt.hip
    D = 768
    sizes = [tuple(v.shape[1:]) for v in clips]
    gs = [math.prod(d // q for d, q in zip(s, PATCH)) for s in sizes]
    lens = [g + n for g, n in zip(gs, counts)]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    rows32 = torch.from_numpy(gen.normal((sum(gs), 3 * math.prod(PATCH)), 31)).cuda()
    tok = torch.from_numpy(gen.normal((sum(gs), D), 32)).cuda()
    packed = torch.from_numpy(gen.normal((cu[-1], D), 33)).cuda()
    mask = torch.from_numpy(gen.normal((1, D), 34)).cuda()
    legs = {
        "patchify": [("hip", lambda: hip.patchify_clips(clips, PATCH[0], PATCH[1])),
                     ("torch", lambda: torch.cat([patch_rows(v) for v in clips], 0).to(torch.bfloat16))],
        "unpatchify": [("hip", lambda: hip.unpatchify_clips(rows32, sizes, 3, PATCH[0], PATCH[1])),
                       ("torch", lambda: [unpatch_rows(r, s).contiguous() for r, s in zip(rows32.split(gs, 0), sizes)])],
        "scatter": [("hip", lambda: hip.packed_scatter(tok, cu, counts, hip.PACKED_TAIL, vec=mask)),
                    ("torch", lambda: torch.cat([t for n, r in zip(counts, tok.split(gs, 0)) for t in (mask.repeat(n, 1), r)], 0))],
        "gather": [("hip", lambda: hip.packed_gather(packed, cu, counts, hip.PACKED_LEAD)),
                   ("torch", lambda: torch.cat([seq[:n] for n, seq in zip(counts, packed.split(lens, 0))], 0))],
    }
    res = {}
    for name, pair in legs.items():
        t = alternate(pair, warmup + 3, 20 * steps, rounds, f"{what} {name}")
        res[name] = dict(t, torch_over_hip=round(t["torch"]["ms"] / t["hip"]["ms"], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg; the legs alternate inside a round")
    ap.add_argument("--torch", action="store_true", help="also time the stock-torch model under autocast(bf16), alternating with the HIP model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "titok_step.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    model = vt.make({"name": "titok", "args": {"bottleneck": None, "prior_model": None}}).cuda().train()
    ref = TorchModel().cuda().train() if a.torch else None
    note("models built")
    res = {"metric": "titok (base) ms per fwd+bwd step", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "legs": [], "movement": []}
    for name in a.workloads:
        sizes, counts = WORKLOADS[name]
        clips = [torch.from_numpy(gen.uniform((3,) + s, 70 + i)).cuda() for i, s in enumerate(sizes)]
        grids = vt.hip.clip_grids(sizes, PATCH[0], PATCH[1])
        freqs = vt.varlen.rope_freqs(grids, counts)[0].cuda() if ref is not None else None

        def hip_step():
            model.zero_grad(set_to_none=True)
            x_q, _ = model.encode(clips, counts)
            sum(p.square().mean() for p in model.decode(x_q, counts, sizes)).backward()

        def torch_step():
            ref.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = ref(clips, counts, freqs)
            sum(p.float().square().mean() for p in out).backward()

        legs = [("hip", hip_step)] + ([("torch_autocast_bf16", torch_step)] if ref is not None else [])
        t = alternate(legs, a.warmup, a.steps, a.rounds, f"{name} step")
        leg = {"workload": name, "clips": [list(s) for s in sizes], "tokens": counts, "rows": sum(math.prod(g) + n for g, n in zip(grids, counts))}
        for n, v in t.items():
            leg[n] = {"ms_per_step": v["ms"], "clips_per_s": round(len(sizes) * 1000.0 / v["ms"], 2), "ms_min": v["ms_min"], "ms_max": v["ms_max"]}
        if ref is not None:
            leg["torch_over_hip"] = round(t["torch_autocast_bf16"]["ms"] / t["hip"]["ms"], 3)
        res["legs"].append(leg)
        res["movement"].append(dict(workload=name, **movement_legs(clips, counts, a.steps, a.warmup, a.rounds, name)))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
