"""`autoencoder_dualpatch` on the GPU: its encoder, decoder and whole model against the fixture the reference's own code wrote
(tests/golden/make_golden_dualpatch.py), and against themselves.

Tolerance, from the reference alone (the rule of tests/test_titok_model_gpu.py and tests/test_design_gpu.py): for both cases and both stages,
every stored tensor -- z, d_video and the encoder's parameter gradients; pred, d_codes and the decoder's -- is within 2 x the distance of the
reference's OWN autocast-bf16 CPU run from its fp32 run (`<tensor>_bf16_dist` in the fixture).  Each stage prints
`RATIO <case> <stage> <tensor> <distance> <bf16_dist> <ratio>` first.  A second step reproduces every bit.

One tensor per layer is a mathematical zero: without a rotary embedding a bias on every key shifts every score of a query by the same
amount, which the softmax ignores, so d k_norm.bias is rounding noise in every run (the reference's fp32 values are ~1e-9, its bf16 run is
~1e4 x that away).  The rule above still applies as written: the bar then says that this build's noise is within twice the reference's.

The rest is exact, on the square case B: the stream DualPatchEmbed builds equals the concatenation of latent_queries and two PatchEmbed calls
on contiguous slices; forward equals decode(encode(.)); decode_indices equals decode of the codes; the whole-model backward equals the two
stages chained by hand.  One forward + backward at the default geometry closes the file.

Measured ratios on an MI355X (distance / bf16_dist, bar 2); per stage the outputs, the input-side gradients, and the largest and smallest over
all stored tensors (the full table is in DESIGN.md 5j):
  A enc: z 1.068, d_video 0.955; largest z, smallest 0.285 (attn_layer.1.k_norm.bias), 0.658 (attn_layer.1.q_norm.weight) among the non-zero ones
  A dec: pred 1.011, d_codes 0.779; largest 1.088 (ffd_layer.1.0.weight), smallest 0.228 (attn_layer.0.k_norm.bias), 0.534 (first_unpatch.bias)
  B enc: z 1.043, d_video 0.990; largest 1.061 (rest_patch_embed.bias), smallest 0.228 (k_norm.bias), 0.437 (proj_out.bias)
  B dec: pred 1.003, d_codes 0.942; largest 1.875 (rest_unpatch.bias: three numbers), smallest 0.118 (k_norm.bias), 0.341 (q_norm.bias)
"""
import pytest
import torch

from oracle import inputs as gen
from tests import dualpatch_reference as R

pytestmark = pytest.mark.gpu


def vt():
    import video_tokenizer_amd
    return video_tokenizer_amd


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _build(case, stage):
    c = R.CASES[case]
    m = (vt().DualPatchEncoder(out_channels=R.TOKEN_SIZE, out_tokens=c["tokens"], _dims=c["dims"], **R.geometry(case)) if stage == "enc"
         else vt().DualPatchDecoder(in_channels=R.TOKEN_SIZE, in_tokens=c["tokens"], _dims=c["dims"], **R.geometry(case)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage).items()}, strict=True)     # the reference's keys
    return m.cuda()


def _step(m, case, stage, golden):
    w_z, w_p = R.cotangents(case)
    m.zero_grad(set_to_none=True)
    if stage == "enc":
        x = torch.from_numpy(R.video(case)).cuda().requires_grad_(True)
        z = m(x)
        (z * torch.from_numpy(w_z).cuda()).sum().backward()
        out = {"z": z.detach(), "d_video": x.grad}
    else:
        c = torch.from_numpy(golden[f"{case}/codes"]).cuda().requires_grad_(True)
        pred = m(c)
        (pred * torch.from_numpy(w_p).cuda()).sum().backward()
        out = {"pred": pred.detach(), "d_codes": c.grad}
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    out.update({"d_" + n: named[n].grad for n in R.stored_params(case, stage)})
    return out


@pytest.mark.parametrize("stage", R.STAGES)
@pytest.mark.parametrize("case", list(R.CASES))
def test_stage_matches_the_reference_within_its_own_bf16_distance(golden, case, stage):
    m = _build(case, stage)
    out = _step(m, case, stage, golden)
    failures = []
    for t in R.tensors(case, stage):
        want = torch.from_numpy(golden[f"{case}/{stage}/{t}"])
        assert out[t] is not None and tuple(out[t].shape) == tuple(want.shape) and out[t].dtype == torch.float32, t
        d, bar = R.rel_l2(out[t].cpu(), want), float(golden[f"{case}/{stage}/{t}_bf16_dist"])
        print(f"RATIO {case} {stage} {t} {d:.3e} {bar:.3e} {d / bar:.3f}")
        if not d <= 2 * bar:
            failures.append((t, d, bar))
    assert not failures, failures
    again = _step(m, case, stage, golden)                               # a second step reproduces every bit
    for t in R.tensors(case, stage):
        assert torch.equal(out[t], again[t]), t


def test_stream_equals_patch_embeds_of_contiguous_slices():
    """bit for bit on the square case: the same GEMM on the same rows, the same epilogue; only where the rows land differs"""
    F = vt().functional
    enc = _build("B", "enc")
    x = torch.from_numpy(R.video("B")).cuda()
    T0 = enc.first_frame_temporal_patch
    with torch.no_grad():
        got = enc.stream(x)
        first = F.PatchEmbed.apply(x[:, :, :T0].contiguous(), enc.first_patch_embed.weight, enc.first_patch_embed.bias, enc.first_pos_embed)
        rest = F.PatchEmbed.apply(x[:, :, T0:].contiguous(), enc.rest_patch_embed.weight, enc.rest_patch_embed.bias, enc.rest_pos_embed)
        want = torch.cat([enc.latent_queries.expand(x.shape[0], -1, -1), first, rest], dim=1)
    assert tuple(got.shape) == (4, 64, 512) and torch.equal(got, want)


def _small_model():
    torch.manual_seed(0)
    c = R.CASES["B"]
    m = vt().AutoEncoderDualPatch(_geometry=dict(dims=c["dims"], tokens=c["tokens"], **R.geometry("B")), junk=1).cuda()
    with torch.no_grad():                                               # biases and affines away from their initial 0 / 1
        for i, p in enumerate(m.parameters()):
            if p.dim() == 1:
                p.add_(torch.from_numpy(gen.normal(tuple(p.shape), 9500 + i, 0.1)).cuda())
    return m


def test_whole_model_is_its_stages_chained():
    m = _small_model()
    x = torch.from_numpy(R.video("B")).cuda()
    w = torch.from_numpy(R.cotangents("B")[1]).cuda()
    out = m(x)["pred_frames"]
    assert tuple(out.shape) == R.video_shape("B") and out.dtype == torch.float32
    (out * w).sum().backward()
    whole = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert all(g is not None for g in whole.values())

    x_q, info = m.encode(x)
    assert torch.equal(m.decode(x_q), out)                              # forward = decode(encode(.))
    z = m.encoder(x)
    codes, d = m.quantize(z)
    assert torch.equal(codes, x_q) and torch.equal(info["indices"], d["indices"]) and tuple(d["indices"].shape) == (4, 16)
    assert torch.equal(m.decode_indices(info["indices"]), m.decode(codes))   # the codes are exact functions of the indices

    m.zero_grad(set_to_none=True)                                       # the decoder stage alone, from a leaf ...
    leaf = x_q.detach().clone().requires_grad_(True)
    (m.decode(leaf) * w).sum().backward()
    for n, p in m.decoder.named_parameters():
        assert torch.equal(p.grad, whole["decoder." + n]), n
    m.zero_grad(set_to_none=True)                                       # ... and the encoder stage with the cotangent it delivers
    codes.backward(leaf.grad)                                           # through the FSQ backward
    for n, p in m.encoder.named_parameters():
        assert torch.equal(p.grad, whole["encoder." + n]), n


def test_default_geometry_runs_forward_and_backward():
    torch.manual_seed(0)
    m = vt().make({"name": "autoencoder_dualpatch", "args": dict(bottleneck=None, prior_model=None)}).cuda()
    x = torch.from_numpy(gen.video_clips(1, 16, 128, 9600)).cuda()
    pred = m(x)["pred_frames"]
    assert tuple(pred.shape) == (1, 3, 16, 128, 128) and pred.dtype == torch.float32 and bool(torch.isfinite(pred).all())
    (pred - x).square().mean().backward()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
