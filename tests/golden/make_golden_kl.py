"""Generate the KL ('skl') bottleneck fixtures from the reference's own models/bottleneck.py (build container only).

Run once here:  python tests/golden/make_golden_kl.py
It loads the reference's bottleneck.py through make_golden.load_reference() and runs `SummedKLDivergenceRegularizer` (over
`DiagonalGaussianDistribution`) on the inputs of tests/kl_reference.fixture_inputs, with torch.randn re-seeded so that the noise the
reference draws is recorded too.  Committed outputs:
  kl_pieces.npz  -- z (logvar entries below -30, above 20 and exactly at both bounds), the noise, the sample, mean, kl(), loss_kl, and
                    dz of the weighted loss tests/kl_reference.weighted_loss
  kl_layout.npz  -- state-dict names and shapes of Bottleneck(regularizer=skl) at (bottleneck_dim 8, input 64, output 48, 16 tokens)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import kl_reference as K  # noqa: E402
from tests.golden import make_golden  # noqa: E402

LAYOUT_ARGS = dict(bottleneck_dim=8, input_dim=64, output_dim=48, token_nums=16)


def main():
    _, bott, _ = make_golden.load_reference()
    z, _, w = K.fixture_inputs()
    d = z.shape[-1] // 2
    reg = bott.SummedKLDivergenceRegularizer(dim=d)
    zz = z.clone().requires_grad_(True)
    torch.manual_seed(1234)
    out = reg(zz)
    torch.manual_seed(1234)
    eps = torch.randn(out["regularized_z"].shape)
    loss = K.weighted_loss(out, w)
    loss.backward()
    pieces = {"z": z, "w": w, "noise": eps, "sample": out["regularized_z"].detach(), "mean": out["bottleneck_rep"].detach(),
              "kl": out["dist"].kl().detach(), "loss_kl": out["loss_kl"].detach().reshape(1), "dz": zz.grad}
    np.savez_compressed(os.path.join(HERE, "kl_pieces.npz"), **{k: v.numpy().astype(np.float32) for k, v in pieces.items()})

    torch.manual_seed(0)
    b = bott.Bottleneck(regularizer={"name": "skl", "args": {}}, norm="none", **LAYOUT_ARGS)
    sd = b.state_dict()
    np.savez_compressed(os.path.join(HERE, "kl_layout.npz"), names=np.array(json.dumps(list(sd))),
                        shapes=np.array(json.dumps([list(v.shape) for v in sd.values()])), args=np.array(json.dumps(LAYOUT_ARGS)))
    print("wrote kl_pieces.npz, kl_layout.npz:", list(sd), float(out["loss_kl"]))


if __name__ == "__main__":
    main()
