"""Generate the fixture of model_design's transformer stack and modules from the reference's own code (build container only).

Run once here:  python tests/golden/make_golden_design_stack.py
It loads base/rope.py, base/transformer.py, base/utils.py, base/blocks.py, quantizer/fsq.py and autoencoder.py of the reference's
models/model_design by FILE PATH, with the placeholder packages and the SDPA stand-in for `flash_attn` of make_golden_cross.py (plus a
`models.register` that only returns the class).  Inputs and weights come from tests/design_stack_reference.py (oracle/inputs.py
generators), so only OUTPUTS are committed:
  <case>/<tensor>            the reference's fp32 run for the loss sum(y * w): y, dx, dcontext, every parameter gradient, and d_res_scales, the
                             gradients of the 0-dim residual scales pooled into one vector                       (cases xs2, s1)
  <module>/<tensor>          the same for Encoder, FirstFrameEncoder (pre-FSQ tokens, dvideo) and UnifiedDecoder (pred_frames for the reference's
                             own quantised codes mod/main_q, mod/first_q; their gradients), parameter gradients of at most 4096 elements
  <...>_bf16_dist            relative L2 distance between the reference's autocast-bf16 run and its fp32 run
  rope/<case>_cos, _sin      real and imaginary part of the reference's get_freqs for the two stack cases (float64)
  state_dict/names, shapes   name -> shape of the full-size reference model's state_dict() (names and shapes only)
spread over several files (design_stack_reference.GOLDEN_FILES) so that each stays below the largest fixture already committed.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
FILE_CAP = 800_000            # raw bytes per file; the limit is 891 148 (tests/golden/bottleneck_small.npz)

from tests import design_stack_reference as R  # noqa: E402
from tests.golden import make_golden_cross as G  # noqa: E402


def load_reference():
    tr = G.load_reference()                                   # placeholder packages, flash_attn stand-in, rope.py, transformer.py
    sys.modules["models"].register = lambda name: (lambda cls: cls)
    for pkg in ("models.model_design.quantizer",):
        m = type(sys)(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    base = os.path.join(G.REF, "models/model_design")
    G._load("models.model_design.base.utils", os.path.join(base, "base/utils.py"))
    bl = G._load("models.model_design.base.blocks", os.path.join(base, "base/blocks.py"))
    G._load("models.model_design.quantizer.fsq", os.path.join(base, "quantizer/fsq.py"))
    ae = G._load("models.model_design.autoencoder", os.path.join(base, "autoencoder.py"))
    return tr, bl, ae, sys.modules["models.model_design.base.rope"]


def grads_of(module):
    return {n: p.grad.float() for n, p in module.named_parameters()}


def run_stack(tr, rope, name, autocast):
    c = R.STACK_CASES[name]
    I = {k: torch.from_numpy(v) for k, v in R.stack_inputs(name).items()}
    m = tr.TransformerStack(c["dim"], heads=c["heads"], mlp_ratio=c["mlp_ratio"], num_layers=c["num_layers"], has_cross_attn=c["cross"])
    names = list(R.stack_param_shapes(c["dim"], c["mlp_ratio"], c["num_layers"], c["cross"]))
    assert list(m.state_dict().keys()) == names, (list(m.state_dict().keys()), names)
    m.load_state_dict({n: I[n] for n in names})
    x = I["x"].clone().requires_grad_(True)
    ctx = I["context"].clone().requires_grad_(True) if c["cross"] else None
    freqs = rope.get_freqs(c["tokens"], list(c["grid"]), head_dim=64)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = m(x, freqs, context=ctx)
    assert y.dtype == torch.float32                                # final_norm of the fp32 stream returns fp32 under autocast too
    (y.float() * I["w"]).sum().backward()
    return R.collect(y, {"dx": x.grad, "dcontext": ctx.grad if ctx is not None else None}, grads_of(m), names)


def build_mods(bl):
    g = R.MOD
    I = {k: torch.from_numpy(v) for k, v in R.mod_inputs().items()}
    mods = {"encoder": bl.Encoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=3, out_channels=g["token_size"],
                                  in_grid=g["in_grid"], out_tokens=g["tokens"]),
            "first_frame_encoder": bl.FirstFrameEncoder(model_size=g["model_size"], patch_size_hw=g["patch_size"][1:], in_channels=3,
                                                        out_channels=g["token_size"], in_hw=g["in_grid"][1:], out_tokens=g["cond_tokens"]),
            "decoder": bl.UnifiedDecoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=g["token_size"], out_channels=3,
                                         in_tokens=g["tokens"], cond_tokens=g["cond_tokens"], out_grid=g["in_grid"])}
    shapes = R.mod_shapes()
    for k, m in mods.items():
        assert {n: tuple(v.shape) for n, v in m.state_dict().items()} == shapes[k] and list(m.state_dict()) == list(shapes[k]), k
        m.load_state_dict({n: I[f"{k}.{n}"] for n in shapes[k]})
    return mods, I


def run_mod(bl, ae, codes, autocast):
    mods, I = build_mods(bl)
    out = {}
    for k, w in (("encoder", "w_main"), ("first_frame_encoder", "w_first")):
        video = I["video"].clone().requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            tok = mods[k](video if k == "encoder" else video[:, :, 0:1])
        (tok.float() * I[w]).sum().backward()
        res = R.collect(tok, {"dvideo": video.grad}, grads_of(mods[k]), list(R.mod_shapes()[k]), small_only=True, y_name="tokens")
        out.update({f"{k}/{n}": v for n, v in res.items()})
    if codes is None:                                              # the reference's own quantised codes of its fp32 tokens
        from models.model_design.quantizer.fsq import FSQ
        q = FSQ(levels=[8, 8, 8, 5, 5, 5])
        codes = tuple(q(out[f"{k}/tokens"])[0].detach() for k in ("encoder", "first_frame_encoder"))
    mq, fq = (t.clone().requires_grad_(True) for t in codes)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        pred = mods["decoder"](mq, cond=fq)
    (pred.float() * I["w_pred"]).sum().backward()
    res = R.collect(pred, {"dmain_q": mq.grad, "dfirst_q": fq.grad}, grads_of(mods["decoder"]), list(R.mod_shapes()["decoder"]), small_only=True,
                    y_name="pred_frames")
    out.update({f"decoder/{n}": v for n, v in res.items()})
    return out, codes


def main():
    tr, bl, ae, rope = load_reference()
    small, big = {}, []                                            # scalars, tables and lists go to the first file; tensors are packed greedily
    for name, c in R.STACK_CASES.items():
        f32, b16 = run_stack(tr, rope, name, False), run_stack(tr, rope, name, True)
        for t in f32:
            big.append((f"{name}/{t}", f32[t].numpy().astype(np.float32)))
            small[f"{name}/{t}_bf16_dist"] = np.array(R.rel_l2(b16[t], f32[t]), dtype=np.float64)
            print(f"{name:4s} {t:44s} {tuple(f32[t].shape)!s:14s} bf16_dist {R.rel_l2(b16[t], f32[t]):.3e}")
        fr = rope.get_freqs(c["tokens"], list(c["grid"]), head_dim=64)
        small[f"rope/{name}_cos"], small[f"rope/{name}_sin"] = fr.real.numpy().astype(np.float64), fr.imag.numpy().astype(np.float64)
    f32, codes = run_mod(bl, ae, None, False)
    b16, _ = run_mod(bl, ae, codes, True)
    small["mod/main_q"], small["mod/first_q"] = codes[0].numpy().astype(np.float32), codes[1].numpy().astype(np.float32)
    for t in f32:
        big.append((t, f32[t].numpy().astype(np.float32)))
        small[f"{t}_bf16_dist"] = np.array(R.rel_l2(b16[t], f32[t]), dtype=np.float64)
        print(f"mod  {t:60s} {tuple(f32[t].shape)!s:18s} bf16_dist {R.rel_l2(b16[t], f32[t]):.3e}")
    torch.manual_seed(0)
    sd = ae.AutoEncoder(bottleneck=None, prior_model=None).state_dict()
    small["state_dict/names"] = np.array(list(sd.keys()))
    small["state_dict/shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    files, sizes = [dict(small)], [sum(v.nbytes for v in small.values())]
    for k, a in big:
        for i in range(len(files)):
            if sizes[i] + a.nbytes <= FILE_CAP:
                break
        else:
            files.append({})
            sizes.append(0)
            i = len(files) - 1
        files[i][k] = a
        sizes[i] += a.nbytes
    assert len(files) == len(R.GOLDEN_FILES), (len(files), sizes)
    for fn, d in zip(R.GOLDEN_FILES, files):
        np.savez_compressed(os.path.join(HERE, fn), **d)
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
