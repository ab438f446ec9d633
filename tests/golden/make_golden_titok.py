"""Generate the packed `titok` encoder / decoder fixture from the reference's own model_titok code (build container only).

Run once here:  python tests/golden/make_golden_titok.py
It loads base/rope.py, base/transformer.py, base/blocks.py, quantizer/fsq.py and titok.py of the reference's models/model_titok by FILE
PATH, with placeholder packages and the stand-in for `flash_attn` of make_golden_varlen.py (per-sequence scaled_dot_product_attention with
K / V `repeat_interleave`d over the group of query heads, flash-attn's published contract).  `get_model_dims` of the loaded blocks module is
replaced to get the small stacks of titok_reference.CASES; everything else -- patching, the packed concatenations, LayerNorms, Linears,
GEGLU, rotary tables, FSQ and all of autograd -- is the reference's own arithmetic, in fp32 and under torch.autocast('cpu', bfloat16).

Inputs and weights come from tests/titok_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed.  Per case and stage
(titok_reference.CASES, STAGES):
  <case>/<stage>/<tensor>            the tensors of titok_reference.tensors(case, stage) from the reference's fp32 run, fp32
  <case>/<stage>/<tensor>_bf16_dist  relative L2 distance between the reference's autocast-bf16 run and its fp32 run
  <case>/codes                       the reference's FSQ of its fp32 z: the decoder stage's input
  <case>/<stage>/state_dict_keys, state_dict_shapes   of the reference's TiTokEncoder / TiTokDecoder (joined by newlines)
  titok/state_dict_keys, state_dict_shapes            of the reference's TiTok (the hard-coded base geometry), built on the meta device
The arrays are dealt to the files of titok_reference.GOLDEN_FILES in order, a new file whenever the next array would take the current one
past 900 000 bytes, so that each file stays below the size limit of a committed file.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests import titok_reference as R  # noqa: E402
import make_golden_varlen as V  # noqa: E402


def load_reference():
    rope, tr = V.load_reference()
    models = sys.modules["models"]
    models.register = lambda name: (lambda cls: cls)
    pkg = types.ModuleType("models.model_titok.quantizer")
    pkg.__path__ = []
    sys.modules["models.model_titok.quantizer"] = pkg
    base = os.path.join(V.REF, "models/model_titok")
    blocks = V._load("models.model_titok.base.blocks", os.path.join(base, "base/blocks.py"))
    fsq = V._load("models.model_titok.quantizer.fsq", os.path.join(base, "quantizer/fsq.py"))
    titok = V._load("models.model_titok.titok", os.path.join(base, "titok.py"))
    return blocks, fsq, titok


def build(blocks, case, stage):
    dims = R.CASES[case]["dims"]
    real = blocks.get_model_dims
    blocks.get_model_dims = lambda *a, **k: dims
    try:
        m = (blocks.TiTokEncoder(out_channels=R.TOKEN_SIZE) if stage == "enc" else blocks.TiTokDecoder(in_channels=R.TOKEN_SIZE))
    finally:
        blocks.get_model_dims = real
    shapes = R.param_shapes(case, stage)
    assert list(m.state_dict()) == list(shapes) and all(tuple(v.shape) == shapes[k] for k, v in m.state_dict().items())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage).items()}, strict=True)
    return m


def run(blocks, case, stage, autocast, codes=None):
    m = build(blocks, case, stage)
    w_z, w_p = R.cotangents(case)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        if stage == "enc":
            vids = [torch.from_numpy(v).clone().requires_grad_(True) for v in R.clips(case)]
            z = m(vids, list(R.TOKENS))
            loss = (z.float() * torch.from_numpy(w_z)).sum()
        else:
            c = codes.clone().requires_grad_(True)
            pred = m(c, list(R.TOKENS), [list(s) for s in R.CLIP_SIZES])
            assert [tuple(p.shape) for p in pred] == [(3,) + s for s in R.CLIP_SIZES]
            loss = sum((p.float() * torch.from_numpy(w)).sum() for p, w in zip(pred, w_p))
    loss.backward()
    out = ({"z": z.detach().float(), "d_clips": R.flat([v.grad for v in vids])} if stage == "enc"
           else {"pred": R.flat([p.detach().float() for p in pred]), "d_codes": c.grad})
    named = dict(m.named_parameters())
    out.update({"d_" + n: named[n].grad.float() for n in R.stored_params(case, stage)})
    return out, m


def describe(sd):
    return np.array("\n".join(sd)), np.array("\n".join(",".join(str(d) for d in v.shape) for v in sd.values()))


def main():
    blocks, fsq, titok = load_reference()
    arrays = {}
    quant = fsq.FSQ(levels=list(R.LEVELS))
    assert not quant.state_dict()                 # FSQ contributes no key (its buffers are not persistent) ...
    real_fsq, titok.FSQ = titok.FSQ, lambda levels: torch.nn.Identity()   # ... and calls .item(), which a meta tensor refuses
    try:
        with torch.device("meta"):
            whole = titok.TiTok(bottleneck=None, prior_model=None)
    finally:
        titok.FSQ = real_fsq
    arrays["titok/state_dict_keys"], arrays["titok/state_dict_shapes"] = describe(whole.state_dict())
    assert whole.encoder.width == 768 and whole.encoder.num_layers == 12 and whole.encoder.heads == [12, 4]
    for case in R.CASES:
        codes = None
        for stage in R.STAGES:
            (f32, m), (b16, _) = run(blocks, case, stage, False, codes), run(blocks, case, stage, True, codes)
            arrays[f"{case}/{stage}/state_dict_keys"], arrays[f"{case}/{stage}/state_dict_shapes"] = describe(m.state_dict())
            if stage == "enc":
                with torch.no_grad():
                    codes = quant(f32["z"])[0].float()
                arrays[f"{case}/codes"] = codes.numpy().astype(np.float32)
            for t in R.tensors(case, stage):
                arrays[f"{case}/{stage}/{t}"] = f32[t].numpy().astype(np.float32)
                arrays[f"{case}/{stage}/{t}_bf16_dist"] = np.array(R.rel_l2(b16[t], f32[t]), dtype=np.float64)
                print(f"{case} {stage} {t:48s} {tuple(f32[t].shape)!s:14s} bf16_dist {R.rel_l2(b16[t], f32[t]):.3e}")
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
