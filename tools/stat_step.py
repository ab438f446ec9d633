"""Training-step throughput of `autoencoder_stat` and the cost of its fused token gate (csrc/vt_stat.hip).

Prints ONE JSON line:
  * clips/s of forward + backward (train mode, 'adaptive' stage: sampled mask with its STE) at 16x128x128 for each --clips;
  * an interleaved A/B at M = 8 x 1280 rows, W = 768, in the same process: the fused gate (vt_stat_gate_forward + _backward) against
    a torch-ops gate that lives in THIS TOOL ONLY (fc2 as a matmul, sigmoid, bernoulli, the STE, the mask multiply and FSQ as torch
    elementwise ops, backward by autograd).  Both start from the same fc1 output (u, gelu(u)); median of --ab-reps rounds each;
  * each gate kernel's HBM-bytes bound: the bytes it must move / 6.3 TB/s (the measured copy rate).

  python tools/stat_step.py --clips 1 2 8 --steps 10 --warmup 3
For the kernel trace, run a short 8-clip leg under rocprofv3 in a separate process:
  rocprofv3 --kernel-trace --stats -d <dir> -o stat -- python tools/stat_step.py --clips 8 --steps 3 --warmup 2 --ab-reps 0
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import video_tokenizer_amd as vt  # noqa: E402
from oracle import inputs as gen  # noqa: E402

COPY_BPS = 6.3e12
LEVELS = (8, 8, 8, 5, 5, 5)
ARGS = {"bottleneck": None, "prior_model": None, "input_size": 128, "frame_num": 16}


def step_rate(model, clips, steps, warmup):
    video = torch.from_numpy(gen.video_clips(clips, 16, 128, 40 + clips)).cuda()

    def one():
        model.zero_grad(set_to_none=True)
        out = model(video, current_epoch=0)
        (out["pred_frames"].square().mean() + out["probs"].mean() + 0.1 * out["mask"].mean()).backward()

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        one()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return {"clips": clips, "ms_per_step": round(ms, 3), "clips_per_s": round(clips * 1000.0 / ms, 2)}


def torch_fsq(z):
    """FSQ (models/model_new/quantizer/fsq.py:76-107) as torch elementwise ops -- the A/B's yardstick, not a product path"""
    lv = torch.tensor(LEVELS, device=z.device, dtype=torch.float32)
    half_l = (lv - 1) * (1 + 1e-3) / 2
    offset = torch.where(lv.remainder(2) == 0, 0.5, 0.0)
    shift = (offset / half_l).atanh()
    bounded = (z + shift).tanh() * half_l - offset
    q = bounded + (bounded.round() - bounded).detach()
    hw = torch.floor(lv / 2)
    codes = q / hw
    basis = torch.cumprod(torch.tensor((1,) + LEVELS[:-1], device=z.device, dtype=torch.float32), 0)
    idx = ((codes * hw + hw) * basis).sum(-1).to(torch.int32)
    return codes, idx


def gate_ab(reps, M=8 * 1280, W=768):
    dev = "cuda"
    H = vt.hip
    u = torch.from_numpy(gen.normal((M, W), 50, 1.0)).to(torch.bfloat16).to(dev)
    g = torch.nn.functional.gelu(u.float()).to(torch.bfloat16)
    w2 = (torch.from_numpy(gen.normal((W,), 51, 0.05))).to(dev)
    b2 = torch.zeros(1, device=dev)
    z = torch.from_numpy(gen.normal((M, 6), 52, 1.5)).to(dev)
    dcodes = torch.from_numpy(gen.normal((M, 6), 53)).to(dev)
    dprobs = torch.from_numpy(gen.normal((M,), 54)).to(dev)

    def fused():
        probs, mask, codes, idx = H.stat_gate_forward(g, w2, b2, z, LEVELS, H.STAT_SAMPLE, seed=7)
        H.stat_gate_backward(dcodes, dprobs, None, z, mask, probs, u, g, w2, LEVELS, True)

    def torch_ops():
        uu = u.float().requires_grad_(True)
        gg = torch.nn.functional.gelu(uu).to(torch.bfloat16)
        w = w2.clone().requires_grad_(True)
        zz = z.clone().requires_grad_(True)
        logit = (gg.float() @ w + b2).to(torch.bfloat16).float()
        p = torch.sigmoid(logit).to(torch.bfloat16).float()
        m = torch.bernoulli(p.detach())
        m = (m - p).detach() + p
        codes, _ = torch_fsq(zz * m[:, None])
        torch.autograd.backward([codes, p], [dcodes, dprobs])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0

    for _ in range(3):
        fused()
        torch_ops()
    torch.cuda.synchronize()
    tf, tt = [], []
    for _ in range(reps):
        tf.append(timed(fused))
        tt.append(timed(torch_ops))
    fwd_bytes = M * W * 2 + M * 6 * 4 * 2 + M * 4 * 3 + W * 4
    bwd_bytes = 3 * M * W * 2 + M * 6 * 4 * 3 + M * 4 * 3 + 512 * (W + 1) * 4 * 2
    return {"rows": M, "width": W, "reps": reps, "fused_fwd_bwd_us_median": round(statistics.median(tf), 2),
            "torch_ops_fwd_bwd_us_median": round(statistics.median(tt), 2),
            "speedup": round(statistics.median(tt) / statistics.median(tf), 2),
            "fwd_bytes": fwd_bytes, "fwd_hbm_bound_us": round(fwd_bytes / COPY_BPS * 1e6, 2),
            "bwd_bytes": bwd_bytes, "bwd_hbm_bound_us": round(bwd_bytes / COPY_BPS * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ab-reps", type=int, default=30, help="rounds of the interleaved gate A/B (0: leave it out)")
    a = ap.parse_args()
    torch.manual_seed(0)
    model = vt.make({"name": "autoencoder_stat", "args": ARGS}).cuda().train()
    res = {"metric": "autoencoder_stat clips/s (16x128x128) fwd+bwd, train 'adaptive'", "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "warmup": a.warmup, "legs": [step_rate(model, c, a.steps, a.warmup) for c in a.clips]}
    if a.ab_reps > 0:
        res["gate_ab"] = gate_ab(a.ab_reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
