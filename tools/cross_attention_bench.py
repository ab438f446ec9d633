"""Cross attention at the design's decoder shape (2048 queries x 256 first-frame keys, 8 heads of 64) on the GPU:

  kernels  vt_attention_cross_fwd and vt_attention_cross_bwd (dQ + dK/dV launches together) against
           F.scaled_dot_product_attention forward and its autograd backward on the same bf16 operands
  layer    design.CrossAttention forward + backward against its composition from stock torch ops under autocast(bf16)
           (tool-only yardstick: RMSNorm, nn.Linear, per-head RMSNorm, SDPA, sigmoid gate, nn.Linear)

for B = 4 and 8.  The two sides alternate inside one process, `--rounds` rounds of `--iters` calls each between device events, after
a warm-up of every shape; the figure per side is the median over rounds, with the min and max next to it.  Work per call (FLOPs of
the four / ten matrix products of attention forward / backward) is computed from the shapes, so the rates are algorithmic.
No speed bar: this shape has not been measured before.  The dK/dV kernel has only B * H * 2 workgroups at Lk = 256; its own time
comes from a kernel trace of `--trace-leg` (rocprofv3 --kernel-trace --stats -- python tools/cross_attention_bench.py --trace-leg),
given back with --stats <kernel_stats.csv>.

  python tools/cross_attention_bench.py --out profiles/cross_attention_bench.json
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import video_tokenizer_amd as vt  # noqa: E402
from video_tokenizer_amd import hip  # noqa: E402

H, LQ, LK = 8, 2048, 256
D = 64 * H


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def alternate(sides, rounds, iters, warmup=5):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, iters))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in t.items()}


class TorchCrossAttention(nn.Module):
    """the layer from stock torch ops (models/model_design/base/transformer.py:92-141 with SDPA for flash_attn_func)"""

    def __init__(self, dim, heads):
        super().__init__()
        self.h = heads
        self.nq, self.nkv = nn.Parameter(torch.ones(dim)), nn.Parameter(torch.ones(dim))
        self.to_q, self.to_kv, self.to_gate, self.out = (nn.Linear(dim, dim, bias=False), nn.Linear(dim, 2 * dim, bias=False),
                                                         nn.Linear(dim, dim, bias=False), nn.Linear(dim, dim, bias=False))
        self.qn, self.kn = nn.Parameter(torch.ones(64)), nn.Parameter(torch.ones(64))

    @staticmethod
    def rms(x, w, eps=1e-6):
        return (x * x.float().pow(2).mean(-1, keepdim=True).add(eps).rsqrt()).to(x.dtype) * w

    def forward(self, x, c):
        xn, cn = self.rms(x, self.nq), self.rms(c, self.nkv)
        q, gate = self.to_q(xn), self.to_gate(xn)
        k, v = self.to_kv(cn).chunk(2, dim=-1)
        q, k, v = (t.unflatten(-1, (self.h, 64)) for t in (q, k, v))
        q, k = self.rms(q, self.qn).to(v.dtype), self.rms(k, self.kn).to(v.dtype)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).flatten(-2)
        return self.out(o * torch.sigmoid(gate))


def bench_kernels(B, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(B)
    qg = torch.randn(B * LQ, 2 * D, device="cuda", generator=g).to(torch.bfloat16)       # q = columns 0..D of [to_q ; to_gate]'s output
    kv = torch.randn(B * LK, 2 * D, device="cuda", generator=g).to(torch.bfloat16)
    dO = torch.randn(B * LQ, D, device="cuda", generator=g).to(torch.bfloat16)
    q, k, v = qg[:, :D], kv[:, :D], kv[:, D:]
    o, lse = hip.attention_cross_fwd(q, k, v, B, LQ, LK, H)
    dq, dkv = torch.empty(B * LQ, D, device="cuda", dtype=torch.bfloat16), torch.empty_like(kv)
    hd = lambda t, L: t.reshape(B, L, H, 64).transpose(1, 2)
    tq, tk, tv = (hd(t, L).contiguous().requires_grad_(True) for t, L in ((q, LQ), (k, LK), (v, LK)))
    to = F.scaled_dot_product_attention(tq, tk, tv)
    tdO = hd(dO, LQ).contiguous()
    err = float((to.transpose(1, 2).reshape(B * LQ, D).float() - o.float()).norm() / to.float().norm())
    sides = {
        "hip_fwd": lambda: hip.attention_cross_fwd(q, k, v, B, LQ, LK, H),
        "torch_fwd": lambda: F.scaled_dot_product_attention(tq, tk, tv),
        "hip_bwd": lambda: hip.attention_cross_bwd(q, k, v, o, dO, lse, B, LQ, LK, H, dq=dq, dk=dkv[:, :D], dv=dkv[:, D:]),
        "torch_bwd": lambda: torch.autograd.grad(to, (tq, tk, tv), tdO, retain_graph=True),
    }
    r = alternate(sides, rounds, iters)
    flops = 4.0 * B * H * LQ * LK * 64                                   # QK^T and PV
    for k_, mult in (("hip_fwd", 1.0), ("torch_fwd", 1.0), ("hip_bwd", 2.5), ("torch_bwd", 2.5)):      # backward: five products + the recomputed scores count as five
        r[k_]["tflops"] = mult * flops / r[k_]["median_us"] * 1e-6
    r["rel_l2_hip_vs_torch_o"] = err
    return r


def bench_layer(B, rounds, iters):
    torch.manual_seed(0)
    ref = TorchCrossAttention(D, H).cuda()
    mine = vt.CrossAttention(D, H).cuda()
    with torch.no_grad():
        for a, b in ((mine.norm_q.weight, ref.nq), (mine.norm_kv.weight, ref.nkv), (mine.to_q.weight, ref.to_q.weight), (mine.to_kv.weight, ref.to_kv.weight),
                     (mine.to_gate.weight, ref.to_gate.weight), (mine.q_norm.weight, ref.qn), (mine.k_norm.weight, ref.kn),
                     (mine.out_proj.weight, ref.out.weight)):
            a.copy_(b)
    x = torch.randn(B, LQ, D, device="cuda", requires_grad=True)
    c = torch.randn(B, LK, D, device="cuda", requires_grad=True)
    w = torch.randn(B, LQ, D, device="cuda")

    def step_hip():
        (mine(x, c) * w).sum().backward()

    def step_torch():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ref(x, c)
        (y.float() * w).sum().backward()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        yt = ref(x, c).float()
    ym = mine(x, c).detach()
    r = alternate({"hip_layer_fwd_bwd": step_hip, "torch_layer_fwd_bwd": step_torch}, rounds, iters)
    r["rel_l2_hip_vs_torch_y"] = float((ym - yt).norm() / yt.norm())
    return r


def trace_leg():
    B = 8
    qg = torch.randn(B * LQ, 2 * D, device="cuda").to(torch.bfloat16)
    kv = torch.randn(B * LK, 2 * D, device="cuda").to(torch.bfloat16)
    dO = torch.randn(B * LQ, D, device="cuda").to(torch.bfloat16)
    q, k, v = qg[:, :D], kv[:, :D], kv[:, D:]
    for _ in range(30):
        o, lse = hip.attention_cross_fwd(q, k, v, B, LQ, LK, H)
        hip.attention_cross_bwd(q, k, v, o, dO, lse, B, LQ, LK, H)
    torch.cuda.synchronize()


def read_stats(path):
    """kernel_stats.csv of a rocprofv3 --stats run of --trace-leg -> average us of the three attention kernels (B = 8)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("attn_fwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"):
                if key in name:
                    out[key + "_avg_us"] = float(row["AverageNs"]) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="profiles/cross_attention_bench.json")
    ap.add_argument("--trace-leg", action="store_true", help="only run the kernels 30 times at B = 8 (the program of a rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 run of --trace-leg: adds the per-kernel times")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    if a.trace_leg:
        return trace_leg()
    res = {"shape": {"H": H, "Lq": LQ, "Lk": LK, "head_dim": 64}, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for B in (4, 8):
        res[f"B{B}"] = {"kernels": bench_kernels(B, a.rounds, a.iters), "layer": bench_layer(B, a.rounds, max(a.iters // 4, 10))}
    if a.stats:
        res["B8_kernel_trace"] = read_stats(a.stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
