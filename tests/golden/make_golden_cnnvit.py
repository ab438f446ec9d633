"""Generate the `autoencoder_cnnvit` ends fixture from the reference's own models/model_cnnvit/base/cnnvit.py (build container only).

Run once here:  python tests/golden/make_golden_cnnvit.py
The reference file imports only torch and is loaded by FILE PATH.  Per case and stage of tests/cnnvit_reference.py it builds the reference's
Encoder_cnn / Decoder_cnn, loads the generated parameters, and runs forward + backward twice: in fp32, and under
torch.autocast('cpu', bfloat16).  Stored: the fp32 tensors and, per tensor, the relative L2 distance of the autocast run to the fp32 run (the
key layout is in tests/cnnvit_reference.py).  Inputs and weights come from oracle/inputs.py generators, so only outputs are committed.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/models/model_cnnvit/base/cnnvit.py"

from tests import cnnvit_reference as R  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_cnnvit", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, case, stage, autocast):
    cls = ref.Encoder_cnn if stage == "enc" else ref.Decoder_cnn
    m = cls(**R.ctor(case, stage))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage, shapes).items()}, strict=True)
    x = torch.from_numpy(R.stage_input(case, stage)).requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = m(x)
    out.float().backward(torch.from_numpy(R.cotangent(case, stage)))
    got = {"out": out.detach().float().numpy(), "din": x.grad.numpy()}
    for k, p in m.named_parameters():
        if R.stored_grad(case, stage, k):
            got["g:" + k] = p.grad.float().numpy()
    return got


def main():
    torch.manual_seed(0)
    ref = load_reference()
    arrays = {}
    for case in R.CASES:
        for stage in R.STAGES:
            f32, b16 = run(ref, case, stage, False), run(ref, case, stage, True)
            for k, v in f32.items():
                arrays[f"{case}/{stage}/{k}"] = v.astype(np.float32)
                arrays[f"{case}/{stage}/{k}_bf16_dist"] = np.float64(R.rel_l2(b16[k], v))
            print(case, stage, len(f32), "tensors; out dist", R.rel_l2(b16["out"], f32["out"]), "din dist", R.rel_l2(b16["din"], f32["din"]))
    for stage, cls in zip(R.STAGES, (ref.Encoder_cnn, ref.Decoder_cnn)):
        with torch.device("meta"):
            sd = cls().state_dict()
        arrays[f"default/{stage}/state_dict_keys"] = np.array("\n".join(sd))
        arrays[f"default/{stage}/state_dict_shapes"] = np.array("\n".join(",".join(map(str, v.shape)) for v in sd.values()))
    n = R.write_golden(arrays)
    print(f"wrote {n} files, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
