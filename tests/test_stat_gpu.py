"""`autoencoder_stat` on the GPU: the token-gate kernels (csrc/vt_stat.hip) at the reference size against FSQ and a float64 autograd
restatement, the Bernoulli draw, the whole model at a small geometry against tests/stat_reference.py, the reference's own pieces
(tests/golden/stat_pieces.npz) and one training step at the reference geometry.  GPU only."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import inputs as gen
from oracle import titok_oracle as T
from tests import stat_reference as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def vt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd as v
    v.hip.lib()
    return v


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _gate_inputs(M=8 * 1280, W=768, seed=700):
    u = torch.from_numpy(gen.normal((M, W), seed, 1.0)).to(torch.bfloat16).cuda()
    g = F.gelu(u.float()).to(torch.bfloat16)
    w2 = torch.from_numpy(gen.normal((W,), seed + 1, 0.05)).cuda()
    b2 = torch.tensor([0.02], device="cuda")
    z = torch.from_numpy(gen.normal((M, 6), seed + 2, 1.5)).cuda()
    return u, g, w2, b2, z


def test_gate_kernels_at_reference_size(vt):
    """M = 8 x 1280 rows of width 768, d = 6: the mask, codes and indices are exact; probs and every gradient against float64"""
    H = vt.hip
    u, g, w2, b2, z = _gate_inputs()
    M, W = g.shape
    probs, mask, codes, idx = H.stat_gate_forward(g, w2, b2, z, S.LEVELS, H.STAT_THRESHOLD)
    assert torch.equal(mask, (probs > 0.5).float())
    assert 0.2 < float(mask.mean()) < 0.8
    c_ref, i_ref = H.fsq_forward((z * mask[:, None]).contiguous(), S.LEVELS)
    assert torch.equal(codes, c_ref) and torch.equal(idx, i_ref)
    p64 = torch.sigmoid(g.double() @ w2.double() + 0.02)
    assert float((probs.double() - p64).abs().max()) < 6e-3           # bf16 logit and bf16 probability: <= ~2^-8
    assert torch.equal(probs, probs.to(torch.bfloat16).float())
    forced = torch.from_numpy((gen.uniform((M,), 703) < 0.6).astype(np.float32)).cuda()
    probs_f, mask_f, codes_f, idx_f = H.stat_gate_forward(g, w2, b2, z, S.LEVELS, H.STAT_FORCED, mask_in=forced)
    c_ref, i_ref = H.fsq_forward((z * forced[:, None]).contiguous(), S.LEVELS)
    assert torch.equal(mask_f, forced) and torch.equal(probs_f, probs) and torch.equal(codes_f, c_ref) and torch.equal(idx_f, i_ref)

    dcodes = torch.from_numpy(gen.normal((M, 6), 704)).cuda()
    dprobs = torch.from_numpy(gen.normal((M,), 705)).cuda()
    dmask = torch.from_numpy(gen.normal((M,), 706)).cuda()
    outs = [H.stat_gate_backward(dcodes, dprobs, dmask, z, forced, probs_f, u, g, w2, S.LEVELS, True) for _ in range(2)]
    for a, b in zip(*outs):                                            # fixed-order partial sums: bit-identical run to run
        assert torch.equal(a, b)
    dU, dz, dw2, db2 = outs[0]
    # float64 autograd restatement of the same forward (sampled / forced mask behind the STE, FSQ's straight-through round)
    u64 = u.double().cpu().requires_grad_(True)
    w64 = w2.double().cpu().requires_grad_(True)
    b64 = torch.tensor([0.02], dtype=torch.float64, requires_grad=True)
    z64 = z.double().cpu().requires_grad_(True)
    gg = g.double().cpu()
    g_u = T.gelu_erf(u64)
    logit = (gg + (g_u - g_u.detach())) @ w64 + b64                   # value: the bf16 g the kernel reads; gradient: gelu'(u)
    p = torch.sigmoid(logit)
    fm = forced.double().cpu()
    m = (fm - p).detach() + p
    cq, _, _ = T.fsq(z64 * m[:, None], S.LEVELS)
    ((cq.double() * dcodes.double().cpu()).sum() + (p * dprobs.double().cpu()).sum() + (m * dmask.double().cpu()).sum()).backward()
    assert rel(dz, z64.grad) < 1e-4
    assert rel(dU.float(), u64.grad) < 3e-2
    assert rel(dw2, w64.grad) < 3e-2 and rel(db2, b64.grad) < 3e-2
    # threshold mode: the mask is a constant, only dprobs reaches the logit
    dU_t, dz_t, _, db2_t = H.stat_gate_backward(dcodes, dprobs, dmask, z, mask, probs, u, g, w2, S.LEVELS, False)
    dl = dprobs.double() * probs.double() * (1 - probs.double())
    assert rel(db2_t, dl.sum().reshape(1)) < 1e-4
    c_ref_grad = H.fsq_backward((z * mask[:, None]).contiguous(), dcodes, S.LEVELS) * mask[:, None]
    assert torch.equal(dz_t, c_ref_grad)


def test_sampling_rates_seeds_and_fresh_draws(vt):
    """rows driven to p in {0.02, 0.3, 0.5, 0.7, 0.98}: the keep rate of each is within 4 sigma of binomial; a seed fixes the draw;
    consecutive training calls of the model draw afresh"""
    H = vt.hip
    targets = (0.02, 0.3, 0.5, 0.7, 0.98)
    n, W = 8192, 768
    logits = torch.tensor([math.log(t / (1 - t)) for t in targets]).repeat_interleave(n)
    g = torch.zeros(len(targets) * n, W, dtype=torch.bfloat16)
    g[:, 0] = logits.to(torch.bfloat16)
    g = g.cuda()
    w2 = torch.zeros(W, device="cuda")
    w2[0] = 1.0
    b2 = torch.zeros(1, device="cuda")
    probs, mask, _, _ = H.stat_gate_forward(g, w2, b2, None, None, H.STAT_SAMPLE, seed=12345)
    for i, t in enumerate(targets):
        p = float(probs[i * n])
        assert abs(p - t) < 0.01 and torch.all(probs[i * n:(i + 1) * n] == p)
        k = float(mask[i * n:(i + 1) * n].sum())
        assert abs(k - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (t, p, k)
    again = H.stat_gate_forward(g, w2, b2, None, None, H.STAT_SAMPLE, seed=12345)[1]
    other = H.stat_gate_forward(g, w2, b2, None, None, H.STAT_SAMPLE, seed=12346)[1]
    assert torch.equal(again, mask) and not torch.equal(other, mask)

    cfg = S.make_cfg("tiny")
    m = _build(vt, cfg).train()
    video = torch.from_numpy(gen.video_clips(2, 8, 32, 711)).cuda()
    with torch.no_grad():
        a = m.encode(video)[1]
        b = m.encode(video)[1]
    assert torch.equal(a["probs"], b["probs"]) and not torch.equal(a["mask"], b["mask"])
    assert a["stage"] == "adaptive" and a["indices"].dtype == torch.int32


def _build(vt, cfg):
    m = vt.make({"name": "autoencoder_stat", "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        in_grid=[cfg["frames"], cfg["side"], cfg["side"]], patch_size=cfg["patch"], tokens=cfg["tokens"], model_size=cfg["size"])}})
    m.load_state_dict(S.init_state_dict(cfg), strict=True)
    return m.cuda()


@pytest.mark.parametrize("mode", ["train_adaptive", "eval_threshold", "train_vanilla"])
def test_model_matches_restatement(vt, mode):
    """the whole model (tiny stacks, 8x32x32 clips, 32 latent tokens, B * L = 64) in each gate mode against the restatement, which
    takes the device's mask and codes: pred_frames, probs, mask and EVERY parameter gradient (the probability head's included) under
    loss = sum w * pred_frames + sum a * probs + sum c * mask.  Bars as test_titok_gpu.py::test_autoencoder_matches_oracle."""
    cfg = S.make_cfg("tiny")
    sd = S.init_state_dict(cfg)
    m = _build(vt, cfg)
    m.train(mode != "eval_threshold")
    epoch = -1 if mode == "train_vanilla" else 0
    video = torch.from_numpy(gen.video_clips(2, 8, 32, 720))
    w = torch.from_numpy(gen.normal((2, 3, 8, 32, 32), 721))
    a = torch.from_numpy(gen.normal((2, 32), 722))
    c = torch.from_numpy(gen.normal((2, 32), 723))
    codes, info = m.encode(video.cuda(), current_epoch=epoch)
    pred = m.decode(codes)
    assert info["stage"] == ("vanilla" if epoch < 0 else "adaptive")
    assert pred.shape == video.shape and info["probs"].shape == (2, 32) and info["mask"].shape == (2, 32)
    dmask = info["mask"].detach().cpu()
    if mode == "train_vanilla":
        assert torch.all(dmask == 1)
    if mode == "eval_threshold":
        assert torch.equal(info["mask"], (info["probs"] > 0.5).float())
    if mode == "train_adaptive":
        assert info["mask"].requires_grad and 0 < float(dmask.detach().mean()) < 1
    loss = (pred * w.cuda()).sum() + (info["probs"] * a.cuda()).sum() + (info["mask"] * c.cuda()).sum()
    loss.backward()

    ste = mode == "train_adaptive"
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    taps = {}
    ref = S.stat_forward(p, cfg, video, dmask, ste, emu=True, force_codes=codes.detach().cpu(), taps=taps)
    with torch.no_grad():
        exact = S.stat_forward(sd, cfg, video, dmask, ste, emu=False, force_codes=codes.detach().cpu())
    gap = rel(ref["pred_frames"], exact["pred_frames"])
    tol = max(3e-2, 1.5 * gap)
    assert rel(pred, ref["pred_frames"]) < tol, (gap, tol)
    assert float((info["probs"].cpu() - ref["probs"]).abs().max()) < 3e-2
    assert torch.allclose(info["mask"].detach().cpu(), ref["mask"].detach(), atol=1e-6)
    ((ref["pred_frames"] * w).sum() + (ref["probs"] * a).sum() + (ref["mask"] * c).sum()).backward()
    # the scalar mask tokens' gradients are sums over B * rows * W entries that cancel to a small fraction of their magnitude: their
    # bar is that of the expanded gradient they sum, 4 x tol x its norm (the same per-entry error, accumulated over the entries)
    for k, t in taps.items():
        q = dict(m.named_parameters())[k]
        assert abs(float(q.grad) - float(p[k].grad)) < 4 * tol * float(t.grad.double().norm()), (k, float(q.grad), float(p[k].grad))
    worst = max((rel(q.grad, p[k].grad), k) for k, q in m.named_parameters() if k not in taps)
    assert worst[0] < 4 * tol, worst
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())


def test_reference_pieces_match_fixtures(vt):
    """patchify, the probability head (with its 0.1-scaled input gradient), the decoder projection + rearrange and the eval-mode
    masking of encode against the reference's own code (tests/golden/make_golden_stat.py)"""
    from video_tokenizer_amd import stat as ST
    from video_tokenizer_amd.functional import Linear as LinearFn, PatchEmbed as PatchEmbedFn, Unpatchify as UnpatchifyFn
    ref = np.load(os.path.join(GOLDEN, "stat_pieces.npz"))
    I = {k: torch.from_numpy(v).cuda() for k, v in S.piece_inputs().items()}
    P, grid_in = S.PIECE["patch"], [S.PIECE["frames"], S.PIECE["side"], S.PIECE["side"]]
    enc = ST.Encoder("tiny", P, 3, 6, grid_in, S.PIECE["lat_tokens"]).cuda()
    dec = ST.Decoder("tiny", P, 6, 3, S.PIECE["lat_tokens"], grid_in).cuda()
    with torch.no_grad():
        enc.proj_in.weight.copy_(I["proj_in_w"])
        enc.proj_in.bias.copy_(I["proj_in_b"])
        head = enc.prob_head
        head.net[0].weight.copy_(I["fc1_w"])
        head.net[0].bias.copy_(I["fc1_b"])
        head.net[2].weight.copy_(I["fc2_w"])
        head.net[2].bias.copy_(I["fc2_b"])
        dec.proj_out.weight.copy_(I["proj_out_w"])
        dec.proj_out.bias.copy_(I["proj_out_b"])
        tok = PatchEmbedFn.apply(I["video"], enc.conv_weight(), enc.proj_in.bias, None)
    assert rel(tok, torch.from_numpy(ref["proj_in_out"])) < 1e-2
    lat = I["lat"].clone().requires_grad_(True)
    probs = head.gate(lat, x_grad_scale=0.1)[1]
    (probs * I["probs_cot"]).sum().backward()
    assert float((probs.cpu() - torch.from_numpy(ref["head_probs"])).abs().max()) < 1e-2
    assert rel(lat.grad, torch.from_numpy(ref["head_dx"])) < 3e-2
    for name, t in (("head_dw1", head.net[0].weight), ("head_db1", head.net[0].bias), ("head_dw2", head.net[2].weight), ("head_db2", head.net[2].bias)):
        assert rel(t.grad, torch.from_numpy(ref[name])) < 3e-2, name
    with torch.no_grad():
        B, N = I["dec_y"].shape[:2]
        rows = LinearFn.apply(I["dec_y"], *dec.row_weights())
        video = UnpatchifyFn.apply(rows.reshape(B * N, -1), (B, 3, grid_in[0], grid_in[1], P[0], P[1]))
    assert rel(video, torch.from_numpy(ref["dec_video"])) < 1e-2
    # eval masking: logits placed in column 0 of g with w2 = e_0, so the gate's probabilities are the fixture's given ones
    lg = I["enc_logits"].reshape(-1)
    g = torch.zeros(lg.numel(), 128, dtype=torch.bfloat16, device="cuda")
    g[:, 0] = lg.to(torch.bfloat16)
    w2 = torch.zeros(128, device="cuda")
    w2[0] = 1.0
    x = I["enc_x"].reshape(-1, 6).contiguous()
    probs, mask, codes, idx = vt.hip.stat_gate_forward(g, w2, torch.zeros(1, device="cuda"), x, S.LEVELS, vt.hip.STAT_THRESHOLD)
    assert torch.equal(probs.cpu(), torch.from_numpy(ref["enc_probs"]).reshape(-1))
    assert torch.equal(mask.cpu(), torch.from_numpy(ref["enc_mask"]).reshape(-1))
    assert torch.equal(codes.cpu(), torch.from_numpy(ref["enc_codes"]).reshape(-1, 6))
    assert torch.equal(idx.cpu(), torch.from_numpy(ref["enc_indices"]).reshape(-1))


def test_reference_geometry_train_step_and_eval(vt):
    """vt.make with the yaml's args: 2 clips of 16x128x128, 1280 latent tokens, base stacks; train forward + backward, then eval"""
    m = vt.make({"name": "autoencoder_stat", "args": dict(S.YAML_ARGS)}).cuda().train()
    video = torch.from_numpy(gen.video_clips(2, 16, 128, 730)).cuda()
    out = m(video, current_epoch=0)
    assert out["pred_frames"].shape == (2, 3, 16, 128, 128) and out["probs"].shape == (2, 1280) and out["mask"].shape == (2, 1280)
    assert out["stage"] == "adaptive"
    (out["pred_frames"].square().mean() + out["probs"].mean() + 0.1 * out["mask"].mean()).backward()
    assert torch.isfinite(out["pred_frames"]).all() and torch.isfinite(out["probs"]).all()
    for name, q in m.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), name
    assert float(m.encoder.prob_head.net[0].weight.grad.abs().sum()) > 0
    m.eval()
    with torch.no_grad():
        ev = m(video)
    assert torch.equal(ev["mask"], (ev["probs"] > 0.5).float()) and torch.isfinite(ev["pred_frames"]).all()
