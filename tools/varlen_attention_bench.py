"""Packed variable-length attention (vt_attention_varlen_fwd / _bwd) on the GPU, three questions:

  equal    8 sequences of 2048 rows (the `titok` geometry: 1024 latent + 1024 grid tokens), Hq = Hkv = 12, against vt_attention_fwd / _bwd on
           the same data, and against vt_attention_cross_* (B = 8) on the same three column views.  The packed kernels do the same work
           through another address computation, so their median should lie inside the dense kernels' own interquartile range over the
           rounds of this very run (`inside_dense_iqr`; a single slow dense round does not widen that band).  The cross side tells a cost
           of the separate strides (shared with the cross kernels) from a cost of the boundary table (varlen only).
  grouped  the same shape with (12, 4) against the (12, 12) run on head-expanded K / V: the grouped dK/dV workgroup sweeps three query
           heads and runs at two waves per SIMD instead of three.
  mixed    16 lengths drawn as the reference's smoke block draws them (base/blocks.py:230-241: a grid of 1..4 x 1..16 x 1..16 patches plus
           1..256 latent tokens, fixed seed), (12, 4), against the loop of per-sequence vt_attention_cross_* launches on the head-expanded
           operands and against the dense kernel on a batch padded to max_seqlen.

The sides alternate inside one process, `--rounds` rounds of `--iters` calls each between device events, after a warm-up of every side;
the figure per side is the median over rounds, with the min and max next to it.

  python tools/varlen_attention_bench.py --out profiles/varlen_attention_bench.json
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_tokenizer_amd import hip  # noqa: E402


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
    out = {}
    for k, v in t.items():
        q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
        out[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "q1_us": q[0], "q3_us": q[2]}
    return out


def packed(M, Hq, Hkv, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(M, 64 * (Hq + 2 * Hkv), device="cuda", generator=g).to(torch.bfloat16)
    dO = torch.randn(M, 64 * Hq, device="cuda", generator=g).to(torch.bfloat16)
    D, G = 64 * Hq, 64 * Hkv
    return qkv, (qkv[:, :D], qkv[:, D:D + G], qkv[:, D + G:]), dO


def varlen_sides(tag, ops, dO, cu, Hq, Hkv):
    q, k, v = ops
    M = q.shape[0]
    o, lse = hip.attention_varlen_fwd(q, k, v, cu, Hq, Hkv)
    dqkv = torch.empty(M, 64 * (Hq + 2 * Hkv), device="cuda", dtype=torch.bfloat16)
    D, G = 64 * Hq, 64 * Hkv
    return {
        tag + "_fwd": lambda: hip.attention_varlen_fwd(q, k, v, cu, Hq, Hkv, o=o, lse2=lse),
        tag + "_bwd": lambda: hip.attention_varlen_bwd(q, k, v, o, dO, lse, cu, Hq, Hkv, dq=dqkv[:, :D], dk=dqkv[:, D:D + G], dv=dqkv[:, D + G:]),
    }, o


def expand(ops, Hq, Hkv):
    q, k, v = ops
    M, g = q.shape[0], Hq // Hkv
    x = torch.cat([q] + [t.reshape(M, Hkv, 64).repeat_interleave(g, dim=1).reshape(M, 64 * Hq) for t in (k, v)], dim=1).contiguous()
    D = 64 * Hq
    return x, (x[:, :D], x[:, D:2 * D], x[:, 2 * D:])


def inside(r, a, b):
    """is side a's median inside side b's interquartile range over the rounds (not its min-max: one slow round would widen that)?"""
    return bool(r[b]["q1_us"] <= r[a]["median_us"] <= r[b]["q3_us"])


def leg_equal(rounds, iters):
    B, L, H = 8, 2048, 12
    qkv, ops, dO = packed(B * L, H, H, 1)
    cu = [b * L for b in range(B + 1)]
    sides, o = varlen_sides("varlen", ops, dO, cu, H, H)
    od, lsed = hip.attention_fwd(qkv, B, L, H)
    dqkv = torch.empty_like(qkv)
    sides["dense_fwd"] = lambda: hip.attention_fwd(qkv, B, L, H, o=od)
    sides["dense_bwd"] = lambda: hip.attention_bwd(qkv, od, dO, lsed, B, L, H, dqkv=dqkv)
    q, k, v = ops
    oc, lsec = hip.attention_cross_fwd(q, k, v, B, L, L, H)
    D = 64 * H
    dx = torch.empty_like(qkv)
    sides["cross_fwd"] = lambda: hip.attention_cross_fwd(q, k, v, B, L, L, H)
    sides["cross_bwd"] = lambda: hip.attention_cross_bwd(q, k, v, oc, dO, lsec, B, L, L, H, dq=dx[:, :D], dk=dx[:, D:2 * D], dv=dx[:, 2 * D:])
    r = alternate(sides, rounds, iters)
    r["same_bits_o"] = bool(torch.equal(o.view(torch.int16), od.reshape(B * L, 64 * H).view(torch.int16)))
    r["inside_dense_iqr"] = {"fwd": inside(r, "varlen_fwd", "dense_fwd"), "bwd": inside(r, "varlen_bwd", "dense_bwd")}
    r["ratio_varlen_over_dense"] = {p: r["varlen_" + p]["median_us"] / r["dense_" + p]["median_us"] for p in ("fwd", "bwd")}
    r["ratio_cross_over_dense"] = {p: r["cross_" + p]["median_us"] / r["dense_" + p]["median_us"] for p in ("fwd", "bwd")}
    return r


def leg_grouped(rounds, iters):
    B, L, Hq, Hkv = 8, 2048, 12, 4
    _, ops, dO = packed(B * L, Hq, Hkv, 2)
    cu = [b * L for b in range(B + 1)]
    sides, o = varlen_sides("grouped", ops, dO, cu, Hq, Hkv)
    _, xops = expand(ops, Hq, Hkv)
    xs, ox = varlen_sides("expanded", xops, dO, cu, Hq, Hq)
    sides.update(xs)
    r = alternate(sides, rounds, iters)
    r["same_bits_o"] = bool(torch.equal(o.view(torch.int16), ox.view(torch.int16)))
    r["ratio_grouped_over_expanded"] = {p: r["grouped_" + p]["median_us"] / r["expanded_" + p]["median_us"] for p in ("fwd", "bwd")}
    return r


def leg_mixed(rounds, iters):
    Hq, Hkv = 12, 4
    rng = random.Random(0)
    lengths = [rng.randrange(1, 5) * rng.randrange(1, 17) * rng.randrange(1, 17) + rng.randrange(1, 257) for _ in range(16)]
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    M, Lmax = cu[-1], max(lengths)
    _, ops, dO = packed(M, Hq, Hkv, 3)
    sides, _ = varlen_sides("varlen", ops, dO, cu, Hq, Hkv)
    _, (xq, xk, xv) = expand(ops, Hq, Hkv)
    D = 64 * Hq
    o = torch.empty(M, D, device="cuda", dtype=torch.bfloat16)
    dx = torch.empty(M, 3 * D, device="cuda", dtype=torch.bfloat16)
    lses = []
    for a, b in zip(cu[:-1], cu[1:]):
        ob, lb = hip.attention_cross_fwd(xq[a:b], xk[a:b], xv[a:b], 1, b - a, b - a, Hq)
        o[a:b] = ob
        lses.append(lb)

    def loop_fwd():
        for a, b in zip(cu[:-1], cu[1:]):
            hip.attention_cross_fwd(xq[a:b], xk[a:b], xv[a:b], 1, b - a, b - a, Hq)

    def loop_bwd():
        for (a, b), lb in zip(zip(cu[:-1], cu[1:]), lses):
            hip.attention_cross_bwd(xq[a:b], xk[a:b], xv[a:b], o[a:b], dO[a:b], lb, 1, b - a, b - a, Hq, dq=dx[a:b, :D], dk=dx[a:b, D:2 * D],
                                    dv=dx[a:b, 2 * D:])
    sides["cross_loop_fwd"], sides["cross_loop_bwd"] = loop_fwd, loop_bwd
    pad = torch.randn(16 * Lmax, 3 * D, device="cuda").to(torch.bfloat16)        # the dense kernel's cost on the padded batch (values do not matter)
    dOp = torch.randn(16 * Lmax, D, device="cuda").to(torch.bfloat16)
    op, lp = hip.attention_fwd(pad, 16, Lmax, Hq)
    dpad = torch.empty_like(pad)
    sides["padded_dense_fwd"] = lambda: hip.attention_fwd(pad, 16, Lmax, Hq, o=op)
    sides["padded_dense_bwd"] = lambda: hip.attention_bwd(pad, op, dOp, lp, 16, Lmax, Hq, dqkv=dpad)
    r = alternate(sides, rounds, iters)
    r["lengths"] = lengths
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="profiles/varlen_attention_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    res = {"rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0), "equal": leg_equal(a.rounds, a.iters),
           "grouped": leg_grouped(a.rounds, a.iters), "mixed": leg_mixed(a.rounds, a.iters)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
