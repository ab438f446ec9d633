"""Generate the `CrossAttention` fixture from the reference's own model_design code (build container only).

Run once here:  python tests/golden/make_golden_cross.py
It loads models/model_design/base/rope.py and base/transformer.py of the reference by FILE PATH, with the placeholder packages of
make_golden_stat.py (`models`, `models.model_design`, `models.model_design.base`) and a stand-in for `flash_attn`, which is absent.
Unlike in make_golden_stat.py the stand-in IS called here: `flash_attn_func(q, k, v)` on [B, L, H, hd] operands is
`F.scaled_dot_product_attention` on the operands transposed to [B, H, L, hd], transposed back -- flash-attn's published contract
(softmax(q k^T / sqrt(hd)) v, no mask, no dropout), the one tests/test_oracle_crosscheck.py already relies on.  Everything around
that call -- the two RMSNorms, the four Linears, the per-head q / k norms, the sigmoid gate, and all of autograd -- is the
reference's own arithmetic, in fp32 and under torch.autocast('cpu', bfloat16).

Inputs and weights come from tests/design_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed.  Per case
(design_reference.CASES) and for the loss sum(y * w):
  <case>/<tensor>            y, dx, dcontext and the eight parameter gradients of the reference's fp32 run, fp32
  <case>/<tensor>_bf16_dist  relative L2 distance between the reference's autocast-bf16 run and its fp32 run
The tensors are spread over three files (design_reference.GOLDEN_FILES) so that each stays below the size limit of a committed file.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from tests import design_reference as R  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("models", "models.model_design", "models.model_design.base"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    if "flash_attn" not in sys.modules:
        fa = types.ModuleType("flash_attn")

        def flash_attn_func(q, k, v):
            return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
        fa.flash_attn_func = flash_attn_func
        sys.modules["flash_attn"] = fa
    _load("models.model_design.base.rope", os.path.join(REF, "models/model_design/base/rope.py"))
    return _load("models.model_design.base.transformer", os.path.join(REF, "models/model_design/base/transformer.py"))


def run(tr, name, autocast):
    c = R.CASES[name]
    I = {k: torch.from_numpy(v) for k, v in R.case_inputs(name).items()}
    layer = tr.CrossAttention(c["dim"], c["heads"], c["context_dim"])
    assert tuple(layer.state_dict().keys()) == R.PARAM_NAMES
    layer.load_state_dict({n: I[n] for n in R.PARAM_NAMES})
    x, ctx = I["x"].clone().requires_grad_(True), I["context"].clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = layer(x, ctx)
    (y.float() * I["w"]).sum().backward()
    out = {"y": y.detach().float(), "dx": x.grad, "dcontext": ctx.grad}
    out.update({"d_" + n: p.grad.float() for n, p in layer.named_parameters()})
    return out


def main():
    tr = load_reference()
    big = {}          # the four matrices of the wide case go to files of their own
    files = [{}, {}, {}]
    for name in R.CASES:
        f32, b16 = run(tr, name, False), run(tr, name, True)
        for t in R.TENSORS:
            a = f32[t].numpy().astype(np.float32)
            where = 0
            if name == "d256" and t in ("y", "dx", "d_to_q.weight"):
                where = 1
            elif name == "d256" and t in ("d_to_kv.weight", "d_to_gate.weight", "d_out_proj.weight"):
                where = 2
            files[where][f"{name}/{t}"] = a
            files[0][f"{name}/{t}_bf16_dist"] = np.array(R.rel_l2(b16[t], f32[t]), dtype=np.float64)
            print(f"{name:5s} {t:18s} {tuple(a.shape)!s:14s} bf16_dist {R.rel_l2(b16[t], f32[t]):.3e}")
    for fn, d in zip(R.GOLDEN_FILES, files):
        np.savez_compressed(os.path.join(HERE, fn), **d)
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
