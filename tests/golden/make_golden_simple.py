"""Generate the `autoencoder_convpatchify_simplytransformer` fixture from the reference's own code (build container only).

Run once here:  python tests/golden/make_golden_simple.py
It loads models/model_new/base/{rope,utils,transformer,simpletransformer,blocks}.py, models/model_new/quantizer/fsq.py and
models/model_new/autoencoder.py of the reference by FILE PATH, with the placeholders tests/golden/make_golden_stat.py uses: `flash_attn`
(base/transformer.py imports `flash_attn_func`; the gated layer is never run here) and empty `models...` package modules with a no-op
`register`.  base/simpletransformer.py itself uses torch ops only, so everything below is the reference's own arithmetic, in fp32 on the CPU.

Inputs and weights come from tests/simple_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed, in simple_pieces.npz:
  layout, n_params       state-dict keys / shapes and parameter count of the registered class as the reference builds it
  stack_*                ResidualAttentionBlock1 (B 2, L 64, width 128, 2 heads, 2 layers): output, input gradient, every parameter
                         gradient (the blocks' weight-matrix gradients sub-sampled [::4, ::4]) under loss = sum(cot * out)
  enc_*, dec_*           Encoder3 / Decoder3 (`tiny`, 8x32x32 clips, 32 latent tokens): output, input gradient and the gradients of
                         every parameter of at most 1024 elements
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from tests import simple_reference as S  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("models", "models.model_new", "models.model_new.base", "models.model_new.quantizer"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    sys.modules["models"].register = lambda name: (lambda cls: cls)
    if "flash_attn" not in sys.modules:
        fa = types.ModuleType("flash_attn")

        def flash_attn_func(*a, **k):
            raise RuntimeError("placeholder: the gated layer is never run by this generator")
        fa.flash_attn_func = flash_attn_func
        sys.modules["flash_attn"] = fa
    base = os.path.join(REF, "models/model_new/base")
    for name in ("rope", "utils", "transformer", "simpletransformer"):
        _load(f"models.model_new.base.{name}", os.path.join(base, name + ".py"))
    blocks = _load("models.model_new.base.blocks", os.path.join(base, "blocks.py"))
    _load("models.model_new.quantizer.fsq", os.path.join(REF, "models/model_new/quantizer/fsq.py"))
    return sys.modules["models.model_new.base.simpletransformer"], blocks


def registered_class():
    """the class autoencoder.py registers under S.NAME (the file defines ten classes that are all called AutoEncoder...)"""
    found = {}
    sys.modules["models"].register = lambda name: (lambda cls: found.setdefault(name, cls))
    _load("models.model_new.autoencoder", os.path.join(REF, "models/model_new/autoencoder.py"))
    return found[S.NAME]


def main():
    simple, blocks = load_reference()
    out = {}
    torch.manual_seed(0)
    model = registered_class()(**S.YAML_ARGS)
    assert type(model.encoder).__name__ == "Encoder3" and type(model.encoder.model_layers).__name__ == "ResidualAttentionBlock1"
    out["layout"] = np.array(json.dumps({k: list(v.shape) for k, v in model.state_dict().items()}))
    out["n_params"] = np.array(sum(p.numel() for p in model.parameters()), dtype=np.int64)
    del model

    # ResidualAttentionBlock1 on its own
    g = S.STACK_PIECE
    st = simple.ResidualAttentionBlock1(embed_dim=g["width"], heads=g["heads"], mlp_ratio=4.0, num_layer=g["layers"])
    st.load_state_dict(S.init_stack_state_dict(g["width"], g["layers"], g["seed"]), strict=True)
    freqs = sys.modules["models.model_new.base.rope"].get_freqs(g["tokens"], g["grid"], head_dim=g["width"] // g["heads"])
    I = {k: torch.from_numpy(v) for k, v in S.stack_piece_inputs().items()}
    x = I["x"].clone().requires_grad_(True)
    y = st(x, freqs)
    (y * I["cot"]).sum().backward()
    out["stack_out"], out["stack_dx"] = y.detach().numpy(), x.grad.numpy()
    for k, q in st.named_parameters():
        out["stack_d." + k] = S.subsample(k, q.grad).contiguous().numpy()

    # Encoder3 / Decoder3
    cfg = S.make_cfg(**S.PIECE_CFG)
    sd = S.init_state_dict(cfg, S.PIECE_SEED)
    clip = [cfg["frames"], cfg["side"], cfg["side"]]
    I = {k: torch.from_numpy(v) for k, v in S.model_piece_inputs().items()}
    enc = blocks.Encoder3(model_size=cfg["size"], patch_size=cfg["patch"], in_channels=3, out_channels=len(S.LEVELS), in_grid=clip, out_tokens=cfg["tokens"])
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
    dec = blocks.Decoder3(model_size=cfg["size"], patch_size=cfg["patch"], in_channels=len(S.LEVELS), out_channels=3, in_tokens=cfg["tokens"], out_grid=clip)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    for tag, mod, xin, cot in (("enc", enc, I["video"], I["enc_cot"]), ("dec", dec, I["codes"], I["dec_cot"])):
        x = xin.clone().requires_grad_(True)
        y = mod(x)
        (y * cot).sum().backward()
        out[tag + "_out"], out[tag + "_dx"] = y.detach().numpy(), x.grad.numpy()
        for k, q in mod.named_parameters():
            if q.numel() <= 1024:
                out[f"{tag}_d.{k}"] = q.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "simple_pieces.npz"), **out)
    print("wrote simple_pieces.npz:", {k: v.shape for k, v in out.items() if not k.startswith(("stack_d.", "enc_d.", "dec_d."))},
          os.path.getsize(os.path.join(HERE, "simple_pieces.npz")), "bytes")


if __name__ == "__main__":
    main()
