"""Inputs, cases and an fp32 restatement of the reference's packed grouped-query layer (`Attn` of models/model_titok/base/transformer.py:32-62
with the rotary tables of base/rope.py), for the fixture tests/golden/varlen_*.npz that the reference's own code wrote
(tests/golden/make_golden_varlen.py).  Plain torch on the CPU: importing this module needs no GPU and no built library.

Inputs come from oracle/inputs.py generators, so the fixture holds OUTPUTS only.  A case packs one clip per (grid, token count): sequence b
has tokens[b] latent rows followed by prod(grids[b]) grid rows."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import inputs as gen

EPS = 1e-5
PARAM_NAMES = ("pre_ln.weight", "pre_ln.bias", "to_qkv.weight", "q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias", "out_proj.weight")
_GRIDS = ((1, 2, 3), (2, 4, 4), (1, 8, 16))
_TOKENS = (1, 65, 128)                                       # lengths 7, 97, 256: M = 360
CASES = {
    "h6_2": dict(dim=384, heads=(6, 2), grids=_GRIDS, tokens=_TOKENS, seed=5100),
    "h4_2": dict(dim=256, heads=(4, 2), grids=_GRIDS[:2], tokens=_TOKENS[:2], seed=5200),   # lengths 7, 97: M = 104
    "h2_2": dict(dim=128, heads=(2, 2), grids=_GRIDS[:2], tokens=_TOKENS[:2], seed=5300),
}
TENSORS = ("y", "dx") + tuple("d_" + n for n in PARAM_NAMES)  # per case, as "<case>/<tensor>" (+ "_bf16_dist"), and "<case>/freqs_re|im"
GOLDEN_FILES = tuple(f"varlen_attn_{i}.npz" for i in range(6))      # each below the size limit of a committed file


def lengths(name):
    c = CASES[name]
    return [int(n + math.prod(g)) for g, n in zip(c["grids"], c["tokens"])]


def cu_seqlens(name):
    return [0] + [int(v) for v in np.cumsum(lengths(name))]


def case_inputs(name):
    """x [M, D], the cotangent w of the loss sum(y * w), and the eight parameters, as numpy float32 arrays"""
    c = CASES[name]
    D, (Hq, Hkv), s = c["dim"], c["heads"], c["seed"]
    M = sum(lengths(name))
    return {
        "x": gen.normal((M, D), s + 1).astype(np.float32),
        "w": gen.normal((M, D), s + 2).astype(np.float32),
        "pre_ln.weight": (1 + gen.normal((D,), s + 3, 0.1)).astype(np.float32),
        "pre_ln.bias": gen.normal((D,), s + 4, 0.1).astype(np.float32),
        "to_qkv.weight": gen.normal((D + 128 * Hkv, D), s + 5, D ** -0.5).astype(np.float32),
        "q_norm.weight": (1 + gen.normal((64,), s + 6, 0.1)).astype(np.float32),
        "q_norm.bias": gen.normal((64,), s + 7, 0.1).astype(np.float32),
        "k_norm.weight": (1 + gen.normal((64,), s + 8, 0.1)).astype(np.float32),
        "k_norm.bias": gen.normal((64,), s + 9, 0.1).astype(np.float32),
        "out_proj.weight": gen.normal((D, D), s + 10, D ** -0.5).astype(np.float32),
    }


def rotate(t, freqs):
    """apply_rotary_emb (rope.py:18-24): t [M, h, 64] fp32, freqs complex128 [M, 32]"""
    c = torch.view_as_complex(t.float().reshape(*t.shape[:-1], -1, 2)) * freqs.unsqueeze(-2)
    return torch.view_as_real(c).flatten(-2).type_as(t)


def attn(x, freqs, cu, P, heads):
    """Attn.forward in fp32: x [M, D], P: parameter name -> tensor; differentiable torch CPU"""
    Hq, Hkv = heads
    D = x.shape[-1]
    G = 64 * Hkv
    xn = F.layer_norm(x, (D,), P["pre_ln.weight"], P["pre_ln.bias"], EPS)
    q, k, v = (xn @ P["to_qkv.weight"].t()).split([D, G, G], dim=-1)
    q = rotate(F.layer_norm(q.unflatten(-1, (Hq, 64)), (64,), P["q_norm.weight"], P["q_norm.bias"], EPS), freqs)
    k = rotate(F.layer_norm(k.unflatten(-1, (Hkv, 64)), (64,), P["k_norm.weight"], P["k_norm.bias"], EPS), freqs)
    v = v.unflatten(-1, (Hkv, 64))
    g = Hq // Hkv
    out = []
    for a, b in zip(cu[:-1], cu[1:]):                        # every sequence attends inside itself; query head h on KV head h // g
        qs = q[a:b].transpose(0, 1)
        ks, vs = (t[a:b].repeat_interleave(g, dim=1).transpose(0, 1) for t in (k, v))
        out.append((torch.softmax(qs @ ks.transpose(-1, -2) * 0.125, dim=-1) @ vs).transpose(0, 1))
    return torch.cat(out, 0).flatten(-2) @ P["out_proj.weight"].t()


def run_case(name, freqs):
    """-> dict tensor name (TENSORS) -> fp32 torch tensor, for the loss sum(y * w)"""
    I = {k: torch.from_numpy(v) for k, v in case_inputs(name).items()}
    x = I["x"].clone().requires_grad_(True)
    P = {n: I[n].clone().requires_grad_(True) for n in PARAM_NAMES}
    y = attn(x, freqs, cu_seqlens(name), P, CASES[name]["heads"])
    (y * I["w"]).sum().backward()
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"d_" + n: P[n].grad for n in PARAM_NAMES})
    return out


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def load_golden():
    """the fixture, merged over its files: "<case>/<tensor>", "<case>/<tensor>_bf16_dist", "<case>/freqs_re", "<case>/freqs_im",
    "state_dict_keys", "<case>/state_dict_shapes" -> numpy"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for fn in GOLDEN_FILES:
        with np.load(os.path.join(here, fn)) as z:
            out.update({k: z[k] for k in z.files})
    return out
