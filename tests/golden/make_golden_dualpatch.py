"""Generate the `autoencoder_dualpatch` encoder / decoder fixture from the reference's own model_dualpatch code (build container only).

Run once here:  python tests/golden/make_golden_dualpatch.py
It loads base/utils.py, base/transformer.py, base/blocks.py and autoencoder.py of the reference's models/model_dualpatch and
models/model/quantizer/fsq.py by FILE PATH, with placeholder packages and a stand-in for `flash_attn`, which is absent.  The stand-in IS
called: `flash_attn_func(q, k, v)` on [B, L, H, hd] operands is `F.scaled_dot_product_attention` on the transposed heads (no mask, scale
hd^-0.5: flash-attn's published contract).  `get_model_dims` of the loaded blocks module is replaced to get the small stacks of
dualpatch_reference.CASES; everything else -- the temporal split, both Conv3d, the position tables, the concatenations, the layer stack, both
ConvTranspose3d, FSQ and all of autograd -- is the reference's own arithmetic, in fp32 and under torch.autocast('cpu', bfloat16).

Inputs and weights come from tests/dualpatch_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed.  Per case and stage
(dualpatch_reference.CASES, STAGES):
  <case>/<stage>/<tensor>            the tensors of dualpatch_reference.tensors(case, stage) from the reference's fp32 run, fp32
  <case>/<stage>/<tensor>_bf16_dist  relative L2 distance between the reference's autocast-bf16 run and its fp32 run
  <case>/codes                       the reference's FSQ of its fp32 z: the decoder stage's input
  <case>/<stage>/state_dict_keys, state_dict_shapes   of the reference's Encoder / Decoder (joined by newlines)
  model/state_dict_keys, state_dict_shapes            of the reference's AutoEncoder (the hard-coded default geometry), built on the meta device
An array above dualpatch_reference.SPLIT_BYTES is cut into row chunks "<key>@<i>of<k>"; the arrays are dealt to the files of
dualpatch_reference.GOLDEN_FILES in order, a new file whenever the next array would take the current one past 900 000 bytes, so that each
file stays below the size limit of a committed file.
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

from tests import dualpatch_reference as R  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("models", "models.model_dualpatch", "models.model_dualpatch.base", "models.model", "models.model.quantizer"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    sys.modules["models"].register = lambda name: (lambda cls: cls)
    fa = types.ModuleType("flash_attn")
    fa.flash_attn_func = lambda q, k, v: F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
    sys.modules["flash_attn"] = fa
    base = os.path.join(REF, "models/model_dualpatch")
    for name in ("utils", "transformer"):
        _load(f"models.model_dualpatch.base.{name}", os.path.join(base, f"base/{name}.py"))
    blocks = _load("models.model_dualpatch.base.blocks", os.path.join(base, "base/blocks.py"))
    fsq = _load("models.model.quantizer.fsq", os.path.join(REF, "models/model/quantizer/fsq.py"))
    return blocks, fsq, _load("models.model_dualpatch.autoencoder", os.path.join(base, "autoencoder.py"))


def build(blocks, case, stage):
    c = R.CASES[case]
    real = blocks.get_model_dims
    blocks.get_model_dims = lambda *a, **k: c["dims"]
    try:
        m = (blocks.Encoder(out_channels=R.TOKEN_SIZE, out_tokens=c["tokens"], **R.geometry(case)) if stage == "enc"
             else blocks.Decoder(in_channels=R.TOKEN_SIZE, in_tokens=c["tokens"], **R.geometry(case)))
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
            x = torch.from_numpy(R.video(case)).clone().requires_grad_(True)
            y = m(x)
            loss = (y.float() * torch.from_numpy(w_z)).sum()
        else:
            x = codes.clone().requires_grad_(True)
            y = m(x)
            assert tuple(y.shape) == R.video_shape(case)
            loss = (y.float() * torch.from_numpy(w_p)).sum()
    loss.backward()
    out = {"z": y.detach().float(), "d_video": x.grad} if stage == "enc" else {"pred": y.detach().float(), "d_codes": x.grad}
    named = dict(m.named_parameters())
    out.update({"d_" + n: named[n].grad.float() for n in R.stored_params(case, stage)})
    return out, m


def describe(sd):
    return np.array("\n".join(sd)), np.array("\n".join(",".join(str(d) for d in v.shape) for v in sd.values()))


def main():
    blocks, fsq, auto = load_reference()
    arrays = {}
    quant = fsq.FSQ(levels=list(R.LEVELS))
    assert not quant.state_dict()                 # FSQ contributes no key (its buffers are not persistent) ...
    real_fsq, auto.FSQ = auto.FSQ, lambda levels: torch.nn.Identity()     # ... and calls .item(), which a meta tensor refuses
    try:
        with torch.device("meta"):
            whole = auto.AutoEncoder(bottleneck=None, prior_model=None)
    finally:
        auto.FSQ = real_fsq
    arrays["model/state_dict_keys"], arrays["model/state_dict_shapes"] = describe(whole.state_dict())
    assert (whole.encoder.width, whole.encoder.num_layers, whole.encoder.heads) == (768, 5, 12)
    assert (whole.encoder.out_tokens, whole.encoder.first_num_tokens, whole.encoder.rest_num_tokens) == (1024, 256, 1280)
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
                a = f32[t].numpy().astype(np.float32)
                dist = R.rel_l2(b16[t], f32[t])
                assert dist > 0, (case, stage, t)                        # no bar sits on a zero
                arrays[f"{case}/{stage}/{t}_bf16_dist"] = np.array(dist, dtype=np.float64)
                print(f"{case} {stage} {t:48s} {tuple(a.shape)!s:20s} bf16_dist {dist:.3e}")
                k = -(-a.nbytes // R.SPLIT_BYTES)
                if k == 1:
                    arrays[f"{case}/{stage}/{t}"] = a
                else:
                    for i, part in enumerate(np.array_split(a, k, axis=0)):
                        arrays[f"{case}/{stage}/{t}@{i}of{k}"] = part
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
