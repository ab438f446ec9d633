"""The KL ('skl') bottleneck on the GPU: vt_kl_forward / vt_kl_backward against the CPU restatement (tests/kl_reference.py) with
the device's noise, the noise's statistics and counter scheme, and LARPTokenizer with regularizer 'skl' through the fused engine, the
composed path, decode_from_bottleneck, config B at two clips, GraphedStep replays and the data-parallel wrapper.  GPU only."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import inputs as gen
from oracle import larp_oracle as O
from tests import kl_reference as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd as v
    v.hip.lib()
    return v


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _z(B, N, d, seed):
    z = torch.from_numpy(gen.normal((B, N, 2 * d), seed, 2.0)).float()
    lv = z[..., 1::2]
    lv[0, 0, :4] = torch.tensor([-31.0, -30.0, 20.0, 21.5])     # below, at and above the clamp bounds
    lv[-1, 5, :4] = torch.tensor([-30.0, 20.0, -45.0, 33.0])
    z[..., 1::2] = lv
    return z


@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_kernels_match_restatement_and_are_bit_stable(vt, d):
    H = vt.hip
    B, N = 4, 1024
    z = _z(B, N, d, 900 + d)
    g = torch.from_numpy(gen.normal((B, N, d), 901 + d)).float()
    gm = torch.from_numpy(gen.normal((B, N, d), 902 + d, 0.5)).float()
    gkl = torch.tensor([0.7])
    zc = z.cuda()
    mean, sample, noise, loss, pad = H.kl_forward(zc, seed=0x1234_5678_9ABC, ldp=64)
    dz, dpad = H.kl_backward(zc, noise, g.cuda(), gm.cuda(), gkl.cuda(), ldp=64)
    torch.cuda.synchronize()
    again = H.kl_forward(zc, seed=0x1234_5678_9ABC, ldp=64)
    dz2, dpad2 = H.kl_backward(zc, noise, g.cuda(), gm.cuda(), gkl.cuda(), ldp=64)
    for a, b in zip((mean, sample, noise, loss, pad, dz, dpad), tuple(again) + (dz2, dpad2)):
        assert torch.equal(a, b)                                     # run to run: bit-identical (fixed-order loss sum)
    zr = z.clone().requires_grad_(True)
    ref = K.kl_bottleneck(zr, noise.cpu())
    assert torch.equal(mean.cpu(), ref["mean"].detach())
    torch.testing.assert_close(sample.cpu(), ref["regularized_z"].detach(), rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(loss.item(), ref["loss_kl"].item(), rtol=1e-5)
    p2 = pad.float().reshape(B * N, 64)
    assert torch.equal(p2[:, :d], sample.reshape(B * N, d).to(torch.bfloat16).float()) and not p2[:, d:].any()
    (ref["regularized_z"] * g + ref["mean"] * gm).sum().add(gkl[0] * ref["loss_kl"]).backward()
    # float64 restatement; per element the bar scales with the terms that are added (the logvar gradient's two terms can cancel,
    # exp(logvar) reaches 4.9e8 at the upper bound: an fp32 result is only as exact as its largest term)
    z64 = z.double().requires_grad_(True)
    r64 = K.kl_bottleneck(z64, noise.cpu().double())
    (r64["regularized_z"] * g.double() + r64["mean"] * gm.double()).sum().add(gkl[0].double() * r64["loss_kl"]).backward()
    k = float(gkl[0]) / B
    scale = torch.empty_like(z64)
    scale[..., 0::2] = (g + gm).abs().double() + k * r64["mean"].abs()
    scale[..., 1::2] = 0.5 * (g.double() * noise.cpu().double() * torch.exp(0.5 * r64["logvar"])).abs() + 0.5 * k * (torch.exp(r64["logvar"]) + 1)
    err = (dz.cpu().double() - z64.grad).abs()
    assert bool((err <= 4e-6 * scale.detach() + 1e-6).all()), float((err / (scale.detach() + 1e-30)).max())
    assert rel(dz, zr.grad) < 1e-5
    lv, dlv = z[..., 1::2], dz.cpu()[..., 1::2]
    assert (dlv[(lv < -30) | (lv > 20)] == 0).all() and (dlv[(lv == -30) | (lv == 20)] != 0).all()
    q = dpad.float().reshape(B * N, 64)
    assert torch.equal(q[:, :2 * d], dz.reshape(B * N, 2 * d).to(torch.bfloat16).float()) and not q[:, 2 * d:].any()


def test_noise_statistics_and_counter_scheme(vt):
    H = vt.hip
    B, N, d = 8, 8192, 16                                            # 2^20 draws
    z = torch.zeros(B, N, 2 * d, device="cuda")
    seed = (77 << 32) | 5
    _, _, e, _, _ = H.kl_forward(z, seed=seed)
    x = e.double().reshape(-1).cpu()
    n = x.numel()
    assert n >= 1 << 20 and torch.isfinite(x).all()
    assert abs(float(x.mean())) < 5.0 / math.sqrt(n)
    assert abs(float(x.var()) - 1.0) < 5.0 * math.sqrt(2.0 / n)
    xs = x.sort().values
    cdf = torch.special.ndtr(xs)
    i = torch.arange(1, n + 1, dtype=torch.float64)
    ks = float(torch.maximum(i / n - cdf, cdf - (i - 1) / n).max())
    assert ks < 1.628 / math.sqrt(n), ks                             # Kolmogorov-Smirnov, 1 % level
    # same seed and counter: bit-equal; the device counter adds to the low seed word (eager and replayed calls, same sequence)
    ctr = torch.tensor([5], dtype=torch.int32, device="cuda")
    _, _, e_same, _, _ = H.kl_forward(z, seed=seed)
    _, _, e_ctr, _, _ = H.kl_forward(z, seed=77 << 32, seed_counter=ctr)
    _, _, e_next, _, _ = H.kl_forward(z, seed=seed + 1)
    assert torch.equal(e, e_same) and torch.equal(e, e_ctr)
    assert not torch.equal(e, e_next) and float((e - e_next).abs().mean()) > 0.5


def _build(vt, cfg, norm="none", seed=7):
    model = vt.make(K.kl_spec(cfg, norm))
    sd = K.init_kl_state_dict(cfg, seed=seed)
    if norm == "ln_d":
        d2 = 2 * cfg["bottleneck_dim"]
        sd["bottleneck.norm_layer.weight"] = torch.from_numpy(gen.uniform((d2,), seed + 503, 0.9, 1.1)).float()
        sd["bottleneck.norm_layer.bias"] = torch.from_numpy(gen.uniform((d2,), seed + 504, -0.1, 0.1)).float()
    model.load_state_dict(sd, strict=True)
    return model.cuda(), sd


KEYS = {"pred_frames", "encoded", "bottleneck_rep", "projected_z", "input_norm_first", "input_norm_last", "regularized_z", "dist", "loss_kl"}


def _step(model, x, w, c_kl=0.7):
    for p in model.parameters():
        p.grad = None
    out = model(x)
    ((out["pred_frames"] * w).sum() + c_kl * out["loss_kl"]).backward()
    torch.cuda.synchronize()
    return out, {n: p.grad.clone() for n, p in model.named_parameters()}


def _parity(vt, cfg, model, sd, B, clip_seed, tol_fwd, tol_grad):
    x = torch.from_numpy(gen.video_clips(B, cfg["frame_num"], cfg["input_size"], clip_seed))
    w = torch.from_numpy(gen.normal(tuple(x.shape), clip_seed + 1))
    model.train()
    out, grads = _step(model, x.cuda(), w.cuda())
    assert set(out) == KEYS, set(out) ^ KEYS
    d = cfg["bottleneck_dim"]
    assert tuple(out["bottleneck_rep"].shape) == (B, cfg["bottleneck_token_num"], d)
    assert tuple(out["projected_z"].shape) == (B, cfg["bottleneck_token_num"], 2 * d)
    assert out["loss_kl"].dim() == 0 and torch.equal(out["dist"].mean, out["projected_z"][..., 0::2])
    eps = model.last_noise.detach().cpu()
    assert eps.shape == out["bottleneck_rep"].shape
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("_pe") and k != "decoder_patch_query_embed") for k, v in sd.items()}
    ref = K.tokenizer_forward(p, cfg, x, eps)
    ((ref["pred_frames"] * w).sum() + 0.7 * ref["loss_kl"]).backward()
    fwd = {k: rel(out[k], ref[k]) for k in ("pred_frames", "encoded", "projected_z", "bottleneck_rep", "regularized_z")}
    print("KL PARITY", cfg.get("encoder_depth"), B, {k: round(v, 6) for k, v in fwd.items()})
    for k, e in fwd.items():
        assert e < tol_fwd, (k, e, tol_fwd)
    np.testing.assert_allclose(out["loss_kl"].item(), ref["loss_kl"].item(), rtol=tol_fwd)
    np.testing.assert_allclose(out["input_norm_first"].item(), ref["input_norm_first"].item(), rtol=1e-2)
    assert len(grads) == len(list(model.parameters()))
    bad = [(n, rel(grads[n], p[n].grad)) for n in grads if rel(grads[n], p[n].grad) > tol_grad]
    assert not bad, (tol_grad, sorted(bad, key=lambda t: -t[1])[:6])
    return out


def test_tiny_model_through_the_engine_matches_restatement(vt):
    cfg = O.make_cfg("tiny")
    model, sd = _build(vt, cfg)
    assert model._engine is not None and not model._composed
    _parity(vt, cfg, model, sd, 2, 11, 2e-2, 6e-2)


def test_tiny_model_on_the_composed_path_matches_restatement(vt):
    cfg = O.make_cfg("tiny")
    model, sd = _build(vt, cfg, norm="ln_d")
    assert model._composed and model._engine is None
    _parity(vt, cfg, model, sd, 2, 13, 2e-2, 6e-2)


def test_decode_from_bottleneck(vt):
    cfg = O.make_cfg("tiny")
    model, sd = _build(vt, cfg)
    x = torch.from_numpy(gen.video_clips(2, cfg["frame_num"], cfg["input_size"], 21)).cuda()
    model.eval()
    with torch.no_grad():
        e = model.encode_eval(x)
        v = model.decode_from_bottleneck(e["bottleneck_rep"])
    torch.cuda.synchronize()
    assert "num_x_tokens" in e and "loss_kl" in e
    mean = e["bottleneck_rep"].cpu()
    enc = O.linear(mean, sd["bottleneck.out_linear.weight"], sd["bottleneck.out_linear.bias"], True)
    ref = O.tokenizer_decode(sd, cfg, enc, True)
    assert rel(v, ref) < 2e-2
    # the reference samples in eval mode too: two encodes draw different noise around the same mean
    with torch.no_grad():
        a, b = model(x), model(x)
    assert torch.equal(a["bottleneck_rep"], b["bottleneck_rep"]) and not torch.equal(a["regularized_z"], b["regularized_z"])


def test_config_B_two_clips_forward_backward_matches_restatement(vt):
    """config B at its own size (16x128x128, 12 + 12 blocks, 1024 latents, d = 24 -> 48 projected columns), two clips, every
    parameter gradient, within the full-size bars of test_model_gpu (1e-2 forward, 2e-2 gradients)"""
    cfg = O.make_cfg("B")
    model, sd = _build(vt, cfg, seed=13)
    _parity(vt, cfg, model, sd, 2, 81, 1e-2, 2e-2)


def test_graphed_step_replays_equal_eager_steps(vt):
    from video_tokenizer_amd.engine import GraphedStep
    from video_tokenizer_amd.optim import FusedAdam
    cfg = O.make_cfg("tiny", frame_num=8, input_size=64, bottleneck_token_num=128)
    xs = [torch.from_numpy(gen.video_clips(2, cfg["frame_num"], cfg["input_size"], 300 + i)).cuda() for i in range(4)]

    def loss_fn(out, x):
        return (out["pred_frames"] - x).abs().mean() + 0.1 * out["loss_kl"]

    def fresh():
        model, _ = _build(vt, cfg)
        model.train()
        return model, FusedAdam(model, lr=1e-3, betas=(0.5, 0.9))

    torch.manual_seed(1234)
    model, opt = fresh()
    model._engine.seed_counter = 100
    eager = []
    for i in range(3):
        opt.zero_grad(set_to_none=True)
        out = model(xs[i])
        loss = loss_fn(out, xs[i])
        loss.backward()
        eager.append((loss.detach().clone(), out["regularized_z"].clone(), {n: p_.grad.clone() for n, p_ in model.named_parameters()}))
        opt.step()
    torch.cuda.synchronize()
    torch.manual_seed(1234)
    model2, opt2 = fresh()
    graphed = GraphedStep(model2, xs[3], loss_fn, outputs=("bottleneck_rep", "regularized_z", "loss_kl"))
    graphed.set_seed_counter(100)
    for i in range(3):
        loss, out = graphed(xs[i])
        torch.cuda.synchronize()
        assert torch.equal(loss, eager[i][0]), i
        assert torch.equal(out["regularized_z"], eager[i][1]), i       # same noise: the device counter follows the eager sequence
        for n, p_ in model2.named_parameters():
            assert p_.grad is not None and torch.equal(p_.grad, eager[i][2][n]), (i, n)
        opt2.step()
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(a, b), n
    graphed.close()


def test_data_parallel_step_equals_unwrapped_step(vt):
    import torch.distributed as dist
    from video_tokenizer_amd.parallel import DataParallelTokenizer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        cfg = O.make_cfg("tiny")
        model, _ = _build(vt, cfg)
        model.train()
        x = torch.from_numpy(gen.video_clips(2, cfg["frame_num"], cfg["input_size"], 31)).cuda()
        w = torch.from_numpy(gen.normal(tuple(x.shape), 32)).cuda()

        def run(net, k):
            model._engine.seed_counter = k          # the same noise in both runs
            for p in model.parameters():
                p.grad = None
            out = net(x)
            ((out["pred_frames"] * w).sum() + 0.7 * out["loss_kl"]).backward()
            torch.cuda.synchronize()
            return {n: p.grad.clone() for n, p in model.named_parameters()}

        plain = run(model, 50)
        dp = DataParallelTokenizer(model, bucket_bytes=8 << 20)
        wrapped = run(dp, 50)
        bad = [n for n in plain if not torch.equal(plain[n], wrapped[n])]
        assert not bad, bad
        model._engine.reducer = None
    finally:
        if created:
            dist.destroy_process_group()
