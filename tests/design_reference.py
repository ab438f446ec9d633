"""CPU restatement of model_design's `CrossAttention` layer (models/model_design/base/transformer.py:18-27, 92-141) for the tests,
written from the formulae, and the deterministic inputs of its fixture (tests/golden/make_golden_cross.py writes the reference's
outputs for them, tests/test_design_cpu.py / test_design_gpu.py replay them).  TEST INFRASTRUCTURE ONLY.

    xn = RMSNorm(x; norm_q)            cn = RMSNorm(context; norm_kv)                       (fp32 in, fp32 out)
    q = to_q xn   gate = to_gate xn    k, v = chunk(to_kv cn)                               (Linear, no bias)
    q, k <- per 64-wide head: bf16(bf16(t * rsqrt(mean(t^2) + eps)) * w)                    (q_norm, k_norm)
    o = softmax(q k^T / 8) v           y = out_proj(o * sigmoid(gate))

`emulate_bf16=True` rounds where autocast(bf16) materialises bf16 tensors -- the rounding points of the HIP path: every Linear's
operands and output, the two roundings of the head norm, the attention output, sigmoid(gate) and the gate product.
"""
import numpy as np
import torch

from oracle import inputs as gen
from oracle.larp_oracle import _rb, linear

EPS = 1e-6
PARAM_NAMES = ("norm_q.weight", "norm_kv.weight", "to_q.weight", "to_kv.weight", "to_gate.weight", "q_norm.weight", "k_norm.weight",
               "out_proj.weight")
CASES = {
    "d128": dict(dim=128, heads=2, context_dim=None, B=2, Lq=70, Lk=33, seed=4100),
    "d256": dict(dim=256, heads=4, context_dim=128, B=2, Lq=130, Lk=65, seed=4200),
}
TENSORS = ("y", "dx", "dcontext") + tuple("d_" + n for n in PARAM_NAMES)      # what the fixture holds per case, as "<case>/<tensor>"


def case_inputs(name):
    """x, context, the cotangent w of the loss sum(y * w), and the eight parameters, as numpy arrays"""
    c = CASES[name]
    D, H, B, Lq, Lk, s = c["dim"], c["heads"], c["B"], c["Lq"], c["Lk"], c["seed"]
    Dc = c["context_dim"] or D

    def norm_w(n, seed):      # 1 + 0.2 N(0, 1): away from the all-ones initialisation, so that the weights' gradients matter
        return (1.0 + 0.2 * gen.normal((n,), seed)).astype(np.float32)
    return {
        "x": gen.normal((B, Lq, D), s + 1).astype(np.float32),
        "context": gen.normal((B, Lk, Dc), s + 2).astype(np.float32),
        "w": gen.normal((B, Lq, D), s + 3).astype(np.float32),
        "norm_q.weight": norm_w(D, s + 4),
        "norm_kv.weight": norm_w(Dc, s + 5),
        "to_q.weight": gen.xavier_uniform((D, D), s + 6).astype(np.float32),
        "to_kv.weight": gen.xavier_uniform((2 * D, Dc), s + 7).astype(np.float32),
        "to_gate.weight": gen.xavier_uniform((D, D), s + 8).astype(np.float32),
        "q_norm.weight": norm_w(64, s + 9),
        "k_norm.weight": norm_w(64, s + 10),
        "out_proj.weight": gen.xavier_uniform((D, D), s + 11).astype(np.float32),
    }


def rmsnorm(x, w, eps=EPS):
    return x * torch.rsqrt(torch.mean(x * x, dim=-1, keepdim=True) + eps) * w


def head_rmsnorm(t, w, heads, emu, eps=EPS):
    th = t.unflatten(-1, (heads, 64))
    u = _rb(th * torch.rsqrt(torch.mean(th * th, dim=-1, keepdim=True) + eps), emu)
    return _rb(u * w, emu)


def cross_attention(x, context, P, heads, emulate_bf16=False):
    """x [B, Lq, D], context [B, Lk, Dc], P: parameter name -> tensor; differentiable torch CPU"""
    emu = emulate_bf16
    xn = rmsnorm(x, P["norm_q.weight"])
    cn = rmsnorm(context, P["norm_kv.weight"])
    q = linear(xn, P["to_q.weight"], None, emu)
    gate = linear(xn, P["to_gate.weight"], None, emu)
    k, v = linear(cn, P["to_kv.weight"], None, emu).chunk(2, dim=-1)
    q = head_rmsnorm(q, P["q_norm.weight"], heads, emu).transpose(1, 2)            # [B, H, Lq, 64]
    k = head_rmsnorm(k, P["k_norm.weight"], heads, emu).transpose(1, 2)
    v = v.unflatten(-1, (heads, 64)).transpose(1, 2)
    att = torch.softmax((q @ k.transpose(-2, -1)) * 0.125, dim=-1)
    o = _rb(att @ v, emu).transpose(1, 2).flatten(-2)
    og = _rb(o * _rb(torch.sigmoid(gate), emu), emu)
    return linear(og, P["out_proj.weight"], None, emu)


def run_case(name, emulate_bf16=False):
    """-> dict tensor name (TENSORS) -> fp32 torch tensor, for the loss sum(y * w)"""
    I = {k: torch.from_numpy(v) for k, v in case_inputs(name).items()}
    x, ctx = I["x"].clone().requires_grad_(True), I["context"].clone().requires_grad_(True)
    P = {n: I[n].clone().requires_grad_(True) for n in PARAM_NAMES}
    y = cross_attention(x, ctx, P, CASES[name]["heads"], emulate_bf16)
    (y * I["w"]).sum().backward()
    out = {"y": y.detach(), "dx": x.grad, "dcontext": ctx.grad}
    out.update({"d_" + n: P[n].grad for n in PARAM_NAMES})
    return out


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


GOLDEN_FILES = ("design_cross_attention.npz", "design_cross_attention_2.npz", "design_cross_attention_3.npz")


def load_golden():
    """the fixture, merged over its files: "<case>/<tensor>" and "<case>/<tensor>_bf16_dist" -> numpy"""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for f in GOLDEN_FILES:
        with np.load(os.path.join(here, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out
