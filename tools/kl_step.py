"""Training-step time of LARPTokenizer with the KL bottleneck ('skl', csrc/vt_kl.hip) against the same model with VQ, config B.

Prints ONE JSON line (and writes it to --out):
  * for each --clips: ms per forward + backward step of the KL model and of the VQ model (config B geometry: 16x128x128, 12 + 12
    blocks, 1024 latents, d = 24; train mode, deterministic VQ search), the two interleaved round by round in ONE process, median of
    --rounds rounds of --steps steps each;
  * the two KL kernels' HBM-bytes bounds at the given clips (bytes they must move / 6.3 TB/s, the measured copy rate).
With --stats CSV (the kernel_stats.csv of a rocprofv3 run of this tool, or tools/rocpd_top.py's CSV of its database), the in-step average time of each KL kernel and its
fraction of the bytes bound are added, and the rows of the CSV are copied to <out>_kernel_stats.csv.

  python tools/kl_step.py --clips 1 2 8 --steps 10 --rounds 5 --out profiles/kl_step.json
  rocprofv3 --kernel-trace --stats -d <dir> -o kl -- python tools/kl_step.py --clips 8 --steps 3 --rounds 1 --vq 0
  python tools/rocpd_top.py <dir>/kl_results.db 60 > profiles/kl_step_kernel_stats.csv
  python tools/kl_step.py --clips 8 --rounds 0 --stats profiles/kl_step_kernel_stats.csv --out profiles/kl_step.json
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import video_tokenizer_amd as vt  # noqa: E402
from oracle import inputs as gen  # noqa: E402
from oracle import larp_oracle as O  # noqa: E402
from video_tokenizer_amd.config import model_spec  # noqa: E402

COPY_BPS = 6.3e12
KL_KERNELS = ("kl_fwd_kernel", "kl_loss_kernel", "kl_bwd_kernel")


def build(kl):
    cfg = O.make_cfg("B")
    spec = model_spec(cfg, False)
    if kl:
        spec["args"]["bottleneck"]["args"]["regularizer"]["name"] = "skl"
    torch.manual_seed(0)
    return vt.make(spec).cuda().train(), cfg


def make_step(model, video, kl):
    def one():
        model.zero_grad(set_to_none=True)
        out = model(video)
        aux = out["loss_kl"] * 1e-6 if kl else out["loss_q"]
        (out["pred_frames"].square().mean() + aux).backward()
    return one


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def kernel_bytes(clips, Nq=1024, d=24, ldp=64):
    M = clips * Nq
    fwd = M * 2 * d * 4 + 3 * M * d * 4 + M * ldp * 2 + 2 * 1024 * 4      # z; mean, sample, noise; bf16 sample row; loss partials
    bwd = M * 2 * d * 4 + 2 * M * d * 4 + M * ldp * 2                      # z; dL/dsample, noise; bf16 dz row
    return {"kl_fwd_kernel": fwd, "kl_bwd_kernel": bwd}


def read_stats(path, clips):
    """rocprofv3 --stats kernel_stats.csv -> {kernel: average ns} for the KL kernels (and every row, for the record)"""
    rows = list(csv.DictReader(open(path)))
    avg = {}
    for r in rows:
        name = r.get("Name") or r.get("name") or ""
        for k in KL_KERNELS:
            if k in name:       # rocprofv3's kernel_stats.csv (AverageNs) or tools/rocpd_top.py's CSV of its database (avg_us)
                avg[k] = float(r["AverageNs"]) if "AverageNs" in r else float(r["avg_us"]) * 1000.0
    bounds = kernel_bytes(clips)
    out = {}
    for k, ns in avg.items():
        e = {"in_step_avg_us": round(ns / 1000.0, 2)}
        if k in bounds:
            e["bytes"] = bounds[k]
            e["hbm_bound_us"] = round(bounds[k] / COPY_BPS * 1e6, 2)
            e["fraction_of_bound"] = round(bounds[k] / COPY_BPS * 1e9 / ns, 3)
        out[k] = e
    return out, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved KL / VQ rounds per clips count (0: no timing)")
    ap.add_argument("--vq", type=int, default=1, help="0: KL model only (the rocprofv3 leg)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "LARPTokenizer config B fwd+bwd ms/step, KL ('skl') vs VQ, interleaved", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "legs": []}
    if a.rounds > 0:
        kl_model, cfg = build(True)
        vq_model = build(False)[0] if a.vq else None
        for clips in a.clips:
            video = torch.from_numpy(gen.video_clips(clips, cfg["frame_num"], cfg["input_size"], 40 + clips)).cuda()
            fk = make_step(kl_model, video, True)
            fv = make_step(vq_model, video, False) if vq_model is not None else None
            for _ in range(a.warmup):
                fk()
                if fv:
                    fv()
            torch.cuda.synchronize()
            tk, tv = [], []
            for _ in range(a.rounds):
                tk.append(timed(fk, a.steps))
                if fv:
                    tv.append(timed(fv, a.steps))
            leg = {"clips": clips, "kl_ms_per_step": round(statistics.median(tk), 3), "kl_clips_per_s": round(clips * 1000.0 / statistics.median(tk), 2),
                   "kl_rounds_ms": [round(t, 3) for t in tk]}
            if tv:
                leg.update({"vq_ms_per_step": round(statistics.median(tv), 3), "vq_clips_per_s": round(clips * 1000.0 / statistics.median(tv), 2),
                            "vq_rounds_ms": [round(t, 3) for t in tv], "kl_over_vq": round(statistics.median(tk) / statistics.median(tv), 4)})
            res["legs"].append(leg)
    res["kl_kernel_bytes_bound"] = {str(c): {k: {"bytes": b, "hbm_bound_us": round(b / COPY_BPS * 1e6, 2)} for k, b in kernel_bytes(c).items()}
                                    for c in a.clips}
    if a.stats:
        res["kl_kernels_in_step"], rows = read_stats(a.stats, max(a.clips))
        if a.out:
            with open(os.path.splitext(a.out)[0] + "_kernel_stats.csv", "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=list(rows[0]))
                w.writeheader()
                w.writerows(rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        if os.path.exists(a.out) and a.rounds == 0 and a.stats:   # a --stats-only pass adds to the timing record instead of replacing it
            prev = json.load(open(a.out))
            prev["kl_kernels_in_step"] = res["kl_kernels_in_step"]
            line = json.dumps(prev)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
