"""Generate the `autoencoder_stat` fixtures from the reference's own model_stat code (build container only).

Run once here:  python tests/golden/make_golden_stat.py
It loads models/model_stat/base/blocks.py, models/model_stat/quantizer/fsq.py and models/model_stat/autoencoder.py of the reference
by FILE PATH, together with the model_new files they import (base/transformer.py, base/utils.py, base/rope.py).  Two import lines
need placeholders, none of which is ever called: `flash_attn` (base/transformer.py imports `flash_attn_func`, absent; the layer
stacks are constructed for the state-dict layout but never run) and the `models` package (autoencoder.py imports `register`; a
no-op decorator stands in, and empty package modules stand for `models.model_new...` / `models.model_stat...` so the by-path modules
can be registered under their own names).  This follows make_golden.py's `timm` placeholder.

Inputs come from tests/stat_reference.py (oracle/inputs.py generators), so only OUTPUTS are committed:
  stat_layout.npz  -- state-dict keys, shapes and parameter count of `autoencoder_stat` as the reference builds it
  stat_pieces.npz  -- proj_in on the rearranged patches; ProbPredictor outputs and the input / parameter gradients through the 0.1
                      STE of blocks.py:89; the decoder's proj_out + rearrange; the eval-mode masking + FSQ of `encode` for given x / probs
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

from tests import stat_reference as S  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("models", "models.model_new", "models.model_new.base", "models.model_stat", "models.model_stat.base",
                "models.model_stat.quantizer"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    sys.modules["models"].register = lambda name: (lambda cls: cls)
    if "flash_attn" not in sys.modules:
        fa = types.ModuleType("flash_attn")

        def flash_attn_func(*a, **k):
            raise RuntimeError("placeholder: the layer stacks are never run by this generator")
        fa.flash_attn_func = flash_attn_func
        sys.modules["flash_attn"] = fa
    _load("models.model_new.base.rope", os.path.join(REF, "models/model_new/base/rope.py"))
    _load("models.model_new.base.utils", os.path.join(REF, "models/model_new/base/utils.py"))
    _load("models.model_new.base.transformer", os.path.join(REF, "models/model_new/base/transformer.py"))
    blocks = _load("models.model_stat.base.blocks", os.path.join(REF, "models/model_stat/base/blocks.py"))
    _load("models.model_stat.quantizer.fsq", os.path.join(REF, "models/model_stat/quantizer/fsq.py"))
    ae = _load("models.model_stat.autoencoder", os.path.join(REF, "models/model_stat/autoencoder.py"))
    return blocks, ae


def main():
    blocks, ae = load_reference()
    torch.manual_seed(0)
    model = ae.AutoEncoder(bottleneck=None, prior_model=None, **{k: v for k, v in S.YAML_ARGS.items() if k not in ("bottleneck", "prior_model")})
    sd = model.state_dict()
    layout = {k: list(v.shape) for k, v in sd.items()}
    np.savez_compressed(os.path.join(HERE, "stat_layout.npz"), layout=np.array(json.dumps(layout)),
                        n_params=np.array(sum(p.numel() for p in model.parameters()), dtype=np.int64))

    I = {k: torch.from_numpy(v) for k, v in S.piece_inputs().items()}
    W, P = S.PIECE["width"], S.PIECE["patch"]
    out = {}
    # Encoder: proj_in on the rearranged patches (blocks.py:72-76), an Encoder of the piece geometry
    enc = blocks.Encoder(model_size="tiny", patch_size=list(P), in_channels=3, out_channels=6,
                         in_grid=[S.PIECE["frames"], S.PIECE["side"], S.PIECE["side"]], out_tokens=S.PIECE["lat_tokens"])
    assert enc.width == W
    with torch.no_grad():
        enc.proj_in.weight.copy_(I["proj_in_w"])
        enc.proj_in.bias.copy_(I["proj_in_b"])
        from einops import rearrange
        rows = rearrange(I["video"], "b c (t pt) (h ph) (w pw) -> b (t h w) (pt ph pw c)", pt=P[0], ph=P[1], pw=P[2])
        out["proj_in_out"] = enc.proj_in(rows).numpy()
    # ProbPredictor through x_for_prob = x.detach() + 0.1 * (x - x.detach()) (blocks.py:89-90)
    head = enc.prob_head
    with torch.no_grad():
        head.net[0].weight.copy_(I["fc1_w"])
        head.net[0].bias.copy_(I["fc1_b"])
        head.net[2].weight.copy_(I["fc2_w"])
        head.net[2].bias.copy_(I["fc2_b"])
    x = I["lat"].clone().requires_grad_(True)
    x_for_prob = x.detach() + 0.1 * (x - x.detach())
    probs = head(x_for_prob).view(x.shape[0], x.shape[1])
    (probs * I["probs_cot"]).sum().backward()
    out["head_probs"] = probs.detach().numpy()
    out["head_dx"] = x.grad.numpy()
    out["head_dw1"] = head.net[0].weight.grad.numpy()
    out["head_db1"] = head.net[0].bias.grad.numpy()
    out["head_dw2"] = head.net[2].weight.grad.numpy()
    out["head_db2"] = head.net[2].bias.grad.numpy()
    # Decoder: proj_out + rearrange (blocks.py:143-150)
    dec = blocks.Decoder(model_size="tiny", patch_size=list(P), in_channels=6, out_channels=3, in_tokens=S.PIECE["lat_tokens"],
                         out_grid=[S.PIECE["frames"], S.PIECE["side"], S.PIECE["side"]])
    with torch.no_grad():
        dec.proj_out.weight.copy_(I["proj_out_w"])
        dec.proj_out.bias.copy_(I["proj_out_b"])
        y = dec.proj_out(I["dec_y"])
        out["dec_video"] = rearrange(y, "b (t h w) (pt ph pw c) -> b c (t pt) (h ph) (w pw)", t=dec.grid[0], h=dec.grid[1], w=dec.grid[2],
                                     pt=P[0], ph=P[1], pw=P[2]).numpy()
    # eval-mode masking of encode (autoencoder.py:98-128) for given x / probs: the encoder is replaced by a stand-in returning them
    probs_in = S.bf16_sigmoid(I["enc_logits"])
    model.encoder = type("GivenEncoder", (torch.nn.Module,), {"forward": lambda self, data: (I["enc_x"], probs_in)})()
    model.eval()
    with torch.no_grad():
        x_q, d = model.encode(None, current_epoch=0)
    assert d["stage"] == "adaptive"
    out["enc_codes"] = x_q.numpy()
    out["enc_mask"] = d["mask"].float().numpy()
    out["enc_indices"] = d["indices"].to(torch.int32).numpy()
    out["enc_probs"] = probs_in.numpy()
    np.savez_compressed(os.path.join(HERE, "stat_pieces.npz"), **out)
    print("wrote stat_layout.npz, stat_pieces.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
