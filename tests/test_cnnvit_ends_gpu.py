"""video_tokenizer_amd.cnnvit.Encoder_cnn / Decoder_cnn on the GPU against the fixture made from the reference's own base/cnnvit.py
(tests/golden/make_golden_cnnvit.py): every stored tensor within 2 x the reference's own autocast-bf16 distance to its fp32 run; a second forward
+ backward reproduces every bit; two clips at once equal two one-clip calls bit for bit (GroupNorm is per clip and nothing else mixes clips);
a channels_last_3d input and a contiguous one give the same bits."""
import pytest
import torch

from tests import cnnvit_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def build(case, stage):
    import video_tokenizer_amd as vt
    m = (vt.Encoder_cnn if stage == "enc" else vt.Decoder_cnn)(**R.ctor(case, stage))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage, shapes).items()}, strict=True)
    return m.cuda()


def run(m, x, cot):
    """forward + backward: out, din and every parameter gradient, as fp32 CPU tensors"""
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    out = m(x)
    out.backward(cot.to(out.dtype))
    torch.cuda.synchronize()
    got = {"out": out.detach().float().cpu(), "din": x.grad.float().cpu()}
    got.update({"g:" + k: p.grad.float().cpu() for k, p in m.named_parameters()})
    return got


@pytest.fixture(scope="module")
def runs():
    """(model, input, cotangent, first run) per case and stage, computed once and shared"""
    out = {}
    for case in R.CASES:
        for stage in R.STAGES:
            m = build(case, stage)
            x, cot = torch.from_numpy(R.stage_input(case, stage)).cuda(), torch.from_numpy(R.cotangent(case, stage)).cuda()
            out[case, stage] = (m, x, cot, run(m, x, cot))
    return out


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("stage", R.STAGES)
def test_every_stored_tensor_within_twice_the_references_bf16_distance(golden, runs, case, stage):
    got = runs[case, stage][3]
    rows, over = [], []
    for key in sorted(k for k in golden if k.startswith(f"{case}/{stage}/") and not k.endswith("_bf16_dist")):
        name = key.split("/", 2)[2]
        dist, bar = R.rel_l2(got[name].numpy(), golden[key]), 2.0 * float(golden[key + "_bf16_dist"])
        rows.append((dist / bar, name, dist, bar))
        if not dist <= bar:
            over.append((name, dist, bar))
    rows.sort(reverse=True)
    print(f"{case}/{stage}: {len(rows)} tensors, worst ratios (distance / bar): " + "; ".join(f"{n} {r:.3f}" for r, n, _, _ in rows[:6])
          + f"; out {next(r for r, n, _, _ in rows if n == 'out'):.3f}; din {next(r for r, n, _, _ in rows if n == 'din'):.3f}")
    assert not over, over


@pytest.mark.parametrize("stage", R.STAGES)
def test_second_run_batch_split_and_layout_give_the_same_bits(runs, stage):
    m, x, cot, first = runs["A", stage]
    again = run(m, x, cot)
    for k in first:
        assert torch.equal(first[k], again[k]), f"second run: {k}"
    # a channels_last_3d input and a contiguous one (the latent has 64 channels; the video's layout is the layout pass's business either way)
    cl = run(m, x.contiguous(memory_format=torch.channels_last_3d), cot.contiguous(memory_format=torch.channels_last_3d))
    for k in first:
        assert torch.equal(first[k], cl[k]), f"channels_last_3d input: {k}"
    # two clips at once = two one-clip calls: outputs and input gradients bit for bit
    for b in range(x.shape[0]):
        one = run(m, x[b:b + 1].contiguous(), cot[b:b + 1].contiguous())
        assert torch.equal(one["out"][0], first["out"][b]) and torch.equal(one["din"][0], first["din"][b]), f"clip {b} alone"
