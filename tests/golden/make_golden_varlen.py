"""Generate the packed grouped-query `Attn` fixture from the reference's own model_titok code (build container only).

Run once here:  python tests/golden/make_golden_varlen.py
It loads models/model_titok/base/rope.py and base/transformer.py of the reference by FILE PATH, with placeholder packages (`models`,
`models.model_titok`, `models.model_titok.base`) and a stand-in for `flash_attn`, which is absent.  The stand-in IS called:
`flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)` on packed [M, H, hd] operands is, per sequence,
`F.scaled_dot_product_attention` on that sequence's rows with K / V `repeat_interleave`d over the group of query heads -- flash-attn's
published contract for grouped-query varlen attention (softmax(q k^T / sqrt(hd)) v inside every sequence, query head h on KV head
h // (Hq / Hkv), no mask, no dropout).  Everything around that call -- the LayerNorm, the Linears, the per-head q / k norms, the rotary
tables and their complex128 product, and all of autograd -- is the reference's own arithmetic, in fp32 and under
torch.autocast('cpu', bfloat16).

Inputs and weights come from tests/varlen_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed.  Per case
(varlen_reference.CASES) and for the loss sum(y * w):
  <case>/<tensor>              y, dx and the eight parameter gradients of the reference's fp32 run, fp32
  <case>/<tensor>_bf16_dist    relative L2 distance between the reference's autocast-bf16 run and its fp32 run
  <case>/freqs_re, freqs_im    RoPE.forward(grids, token_counts): the packed complex128 [M, 32] table (eval path; asserted here to equal the
                               train path's gather from the precomputed tables)
  <case>/state_dict_shapes     the shapes of the layer's state dict, in the order of state_dict_keys (joined by newlines)
The arrays are dealt to the files of varlen_reference.GOLDEN_FILES in order, a new file whenever the next array would take the current one
past 900 000 bytes, so that each file stays below the size limit of a committed file.
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

from tests import varlen_reference as R  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("models", "models.model_titok", "models.model_titok.base"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    fa = types.ModuleType("flash_attn")

    def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
        assert list(cu_seqlens_q) == list(cu_seqlens_k)
        g = q.shape[1] // k.shape[1]
        out = []
        for a, b in zip(cu_seqlens_q[:-1], cu_seqlens_q[1:]):
            a, b = int(a), int(b)
            qs = q[a:b].transpose(0, 1)
            ks, vs = (t[a:b].repeat_interleave(g, dim=1).transpose(0, 1) for t in (k, v))
            out.append(F.scaled_dot_product_attention(qs, ks, vs).transpose(0, 1))
        return torch.cat(out, 0)
    fa.flash_attn_varlen_func = flash_attn_varlen_func
    sys.modules["flash_attn"] = fa
    rope = _load("models.model_titok.base.rope", os.path.join(REF, "models/model_titok/base/rope.py"))
    return rope, _load("models.model_titok.base.transformer", os.path.join(REF, "models/model_titok/base/transformer.py"))


def tables(rope, name):
    c = R.CASES[name]
    r = rope.RoPE()
    dev = torch.device("cpu")
    r.eval()
    ev = r(c["grids"], c["tokens"], dev)
    r.train()
    tr = r(c["grids"], c["tokens"], dev)
    assert ev.dtype == torch.complex128 and tuple(ev.shape) == (sum(R.lengths(name)), 32) and torch.equal(ev, tr)
    return ev


def run(tr, name, freqs, autocast):
    c = R.CASES[name]
    I = {k: torch.from_numpy(v) for k, v in R.case_inputs(name).items()}
    layer = tr.Attn(c["dim"], list(c["heads"]))
    assert tuple(layer.state_dict().keys()) == R.PARAM_NAMES
    layer.load_state_dict({n: I[n] for n in R.PARAM_NAMES})
    x = I["x"].clone().requires_grad_(True)
    cu = R.cu_seqlens(name)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = layer(x, freqs, cu, max(R.lengths(name)))
    (y.float() * I["w"]).sum().backward()
    out = {"y": y.detach().float(), "dx": x.grad}
    out.update({"d_" + n: p.grad.float() for n, p in layer.named_parameters()})
    return out, layer


def main():
    rope, tr = load_reference()
    arrays = {"state_dict_keys": np.array("\n".join(R.PARAM_NAMES))}
    for name in R.CASES:
        freqs = tables(rope, name)
        (f32, layer), (b16, _) = run(tr, name, freqs, False), run(tr, name, freqs, True)
        arrays[f"{name}/freqs_re"] = freqs.real.numpy()
        arrays[f"{name}/freqs_im"] = freqs.imag.numpy()
        arrays[f"{name}/state_dict_shapes"] = np.array("\n".join(",".join(str(d) for d in v.shape) for v in layer.state_dict().values()))
        for t in R.TENSORS:
            arrays[f"{name}/{t}"] = f32[t].numpy().astype(np.float32)
            arrays[f"{name}/{t}_bf16_dist"] = np.array(R.rel_l2(b16[t], f32[t]), dtype=np.float64)
            print(f"{name:5s} {t:18s} {tuple(f32[t].shape)!s:14s} bf16_dist {R.rel_l2(b16[t], f32[t]):.3e}")
    files, size = [{}], 0
    for key, a in arrays.items():
        if size and size + a.nbytes > 900000:
            files.append({})
            size = 0
        files[-1][key] = a
        size += a.nbytes
    assert len(files) == len(R.GOLDEN_FILES), len(files)
    for fn, d in zip(R.GOLDEN_FILES, files):
        np.savez_compressed(os.path.join(HERE, fn), **d)
        nbytes = os.path.getsize(os.path.join(HERE, fn))
        print(fn, nbytes, "bytes")
        assert nbytes < (1 << 20)


if __name__ == "__main__":
    main()
