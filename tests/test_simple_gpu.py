"""`autoencoder_convpatchify_simplytransformer` on the GPU: the rotary kernel (csrc/vt_rope.hip) against fp32 torch math, the wiring of
vt_stack_forward_rotary / vt_stack_backward_rotary (bit-exact against the plain calls where the rotation is absent or the identity), the
rotary block stack and the whole model against the CPU restatement (tests/simple_reference.py, pinned to the reference's own modules by
tests/test_simple_cpu.py), and one training step at the reference geometry.  GPU only.

Measured on an MI355X (relative L2 unless noted; the bars are set in the tests, from the project's bars and the restatement's own
bf16-vs-fp32 gap, not from these numbers):
  vt_rope_rotate             forward / conjugate <= 7.5e-6, max abs 0.016 (one bf16 ulp where fp32 fused multiply-adds round differently;
                             bars 3e-3 / 0.04)
  stack vs restatement       over the 8 cases: output 1.65e-3 .. 2.43e-3 (bar 5e-3; restatement gap 2.9e-4 .. 2.6e-3), dx 1.69e-3 .. 3.21e-3
                             (bar 2e-2; gap 3.0e-4 .. 2.7e-3), worst parameter gradient 5.16e-3 .. 5.75e-3, always a norm1.weight whose own
                             gap is 4.0e-3 .. 5.2e-3 (bar 2e-2)
  whole model (12 + 12)      indices agree on 0.953 of the 64 entries (cap 0.8); pred_frames 5.29e-3 at gap 7.67e-3 (tol 3.0e-2); worst
                             parameter gradient 1.10e-2 (bar 0.12); mask tokens -1.2e-2 vs -3.9e-3 and 0 vs 1.1e-2 against summed entries of
                             norm 1.5e4 / 1.2e4 (bar 0.12 x that)
"""
import math

import pytest
import torch

from oracle import inputs as gen
from oracle import titok_oracle as T
from tests import simple_reference as S

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


def _rotate_ref(x, cos, sin, L, H, conjugate):
    """fp32 torch math with the kernel's rounding point: bf16 -> fp32, (a + ib)(c +- is), one rounding to bf16; q and k columns only"""
    M, D = x.shape[0], 64 * H
    pos = torch.arange(M) % L
    c, s = cos[pos][:, None, :], (-sin if conjugate else sin)[pos][:, None, :]          # [M, 1, 32]
    out = x.clone()
    for blk in range(2):
        t = x[:, blk * D:(blk + 1) * D].float().reshape(M, H, 32, 2)
        a, b = t[..., 0], t[..., 1]
        y = torch.stack([a * c - b * s, a * s + b * c], dim=-1).reshape(M, D)
        out[:, blk * D:(blk + 1) * D] = y.to(torch.bfloat16)
    return out


@pytest.mark.parametrize("B,L,H", [(2, 64, 4), (3, 200, 12), (2, 77, 2), (4, 2048, 12)])
def test_rope_rotate_kernel(vt, B, L, H):
    """forward and conjugate against fp32 math (bars of test_titok_gpu.py::test_qknorm_rope_forward_backward); L = 200 and 77 are not
    multiples of 64, M = 600 and 154 not multiples of 128; v and the rows behind M keep their bits; equal positions of different clips
    rotate equally"""
    D, M = 64 * H, B * L
    tokens = L // 2
    rest = L - tokens
    grid = next([t, h, rest // (t * h)] for t in (2, 1) for h in (4, 5, 7, 1) if rest % (t * h) == 0)
    cos, sin = vt.titok.rope_tables(tokens, grid)
    assert cos.shape == (L, 32)
    x = torch.from_numpy(gen.normal((M + 5, 3 * D), 1700 + L, 1.5)).to(torch.bfloat16)
    x[L:2 * L] = x[:L]                                                                 # clip 1 repeats clip 0
    for conj in (False, True):
        want = _rotate_ref(x[:M], cos, sin, L, H, conj)
        buf = x.cuda()
        got = vt.hip.rope_rotate(buf, L, H, cos.cuda(), sin.cuda(), conjugate=conj, rows=M)
        assert got.data_ptr() == buf.data_ptr()                                        # in place
        got = got.cpu()
        e, mx = rel(got[:M, :2 * D], want[:, :2 * D]), float((got[:M, :2 * D].float() - want[:, :2 * D].float()).abs().max())
        print(f"vt_rope_rotate B={B} L={L} H={H} conjugate={int(conj)}: rel {e:.2e}, max abs {mx:.3f}")
        assert e < 3e-3 and mx < 0.04
        assert torch.equal(got[:M, 2 * D:], x[:M, 2 * D:])                             # v: bit-equal to the input
        assert torch.equal(got[M:], x[M:])                                             # rows behind M: not touched
        assert torch.equal(got[:L, :2 * D], got[L:2 * L, :2 * D])
        assert not torch.equal(got[:M, :2 * D], x[:M, :2 * D])
    # the conjugate undoes the forward up to the two bf16 roundings
    buf = x.cuda()
    vt.hip.rope_rotate(buf, L, H, cos.cuda(), sin.cuda(), rows=M)
    vt.hip.rope_rotate(buf, L, H, cos.cuda(), sin.cuda(), conjugate=True, rows=M)
    assert rel(buf[:M, :2 * D], x[:M, :2 * D]) < 2 * 3e-3


def _geom(L):
    """(latent tokens, grid) of an L-row sequence for the rotary tables"""
    grid = [2, 4, (L // 2) // 8]
    return L - math.prod(grid), grid


def _run_stack(vt, x, params, n_head, dy, tables):
    """one forward + backward through the C entry points on a fresh workspace.  tables: "plain" = vt_stack_forward / _backward,
    None = the rotary calls with NULL tables, (cos, sin) = the rotary calls"""
    Fn, H = vt.functional, vt.hip
    B, L, D = x.shape
    assert tables is None or tables == "plain" or all(t.shape == (L, 32) and t.dtype == torch.float32 and t.is_contiguous() for t in tables)
    depth = len(params) // Fn.PARAMS_PER_BLOCK
    handle, nbytes = Fn._stack((B, L, D, n_head, depth))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    grads = [torch.empty_like(p) for p in params]
    pa, ga = Fn._block_array(params, depth), Fn._block_array(grads, depth)
    lib = H.lib()
    if tables == "plain":
        H.check(lib.vt_stack_forward(handle, pa, H.ptr(x), H.ptr(ws), H.ptr(out), H.stream()), "vt_stack_forward")
        H.check(lib.vt_stack_backward(handle, pa, H.ptr(dy), H.ptr(ws), ga, H.ptr(dx), 1, H.stream()), "vt_stack_backward")
    else:
        c, s = (None, None) if tables is None else (H.ptr(tables[0]), H.ptr(tables[1]))
        H.check(lib.vt_stack_forward_rotary(handle, pa, c, s, H.ptr(x), H.ptr(ws), H.ptr(out), H.stream()), "vt_stack_forward_rotary")
        H.check(lib.vt_stack_backward_rotary(handle, pa, c, s, H.ptr(dy), H.ptr(ws), ga, H.ptr(dx), 1, H.stream()), "vt_stack_backward_rotary")
    torch.cuda.synchronize()
    return [out, dx] + grads


@pytest.mark.parametrize("width,heads,L", [(128, 2, 64), (768, 12, 200)])
def test_rotary_stack_wiring_is_bit_exact(vt, width, heads, L):
    """NULL tables == the plain calls, bit for bit (output, dx, every gradient); so are identity tables (cos = 1, sin = 0: x * 1 - y * 0
    and bf16 -> fp32 -> bf16 are exact), which exercises the two extra launches per block; real tables change the output"""
    depth, B = 2, 2
    sd = S.init_stack_state_dict(width, depth, 1800 + width)
    params = [v.cuda() for k, v in sd.items() if k.startswith("blocks.")]
    assert len(params) == depth * vt.functional.PARAMS_PER_BLOCK
    x = torch.from_numpy(gen.normal((B, L, width), 1801, 1.0)).cuda()
    dy = torch.from_numpy(gen.normal((B, L, width), 1802, 1.0)).cuda()
    plain = _run_stack(vt, x, params, heads, dy, "plain")
    null = _run_stack(vt, x, params, heads, dy, None)
    ident = _run_stack(vt, x, params, heads, dy, (torch.ones(L, 32, device="cuda"), torch.zeros(L, 32, device="cuda")))
    for i, (a, b, c) in enumerate(zip(plain, null, ident)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), ("NULL tables", i)
        assert torch.equal(a, c), ("identity tables", i)
    cos, sin = vt.titok.rope_tables(*_geom(L))
    real = _run_stack(vt, x, params, heads, dy, (cos.cuda(), sin.cuda()))
    assert not torch.equal(real[0], plain[0]) and not torch.equal(real[1], plain[1])
    # the handle keeps nothing of the tables: a plain call after a rotary one is the plain result again
    again = _run_stack(vt, x, params, heads, dy, "plain")
    assert all(torch.equal(a, b) for a, b in zip(plain, again))


OUT_BAR, GRAD_BAR = 5e-3, 2e-2      # the project's bars of the gated layer / stack against its restatement (tests/test_titok_gpu.py)


@pytest.mark.parametrize("L", [64, 200])
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("width,heads", [(128, 2), (768, 12)])
def test_rotary_stack_matches_restatement(vt, width, heads, depth, L):
    """ResidualAttentionBlock1 (blocks + final LayerNorm) on the engine against the bf16-emulating restatement: output, dx and EVERY
    parameter gradient under loss = sum(cot * out).  Each bound is max(project bar, 1.5 x the restatement's own emu-vs-fp32 gap of that
    quantity), as test_titok_gpu.py::test_autoencoder_matches_oracle derives its bound.  B = 2: M = 400 at L = 200 is not a multiple
    of 128."""
    B = 2
    tokens, grid = _geom(L)
    sd = S.init_stack_state_dict(width, depth, 1900 + width + depth)
    x0 = torch.from_numpy(gen.normal((B, L, width), 1901, 1.0))
    cot = torch.from_numpy(gen.normal((B, L, width), 1902, 1.0))
    ang = T.rope_angles(tokens, grid, 64)
    runs = {}
    for emu in (True, False):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        xr = x0.clone().requires_grad_(True)
        y = S.stack(xr, p, "", depth, heads, ang, emu=emu)
        (y * cot).sum().backward()
        runs[emu] = (y.detach(), xr.grad, {k: q.grad for k, q in p.items()})
    m = vt.titok.ResidualAttentionBlock1(width, heads, 4, depth)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    xd = x0.cuda().requires_grad_(True)
    cos, sin = vt.titok.rope_tables(tokens, grid)
    out = m(xd, (cos.cuda(), sin.cuda()))
    (out * cot.cuda()).sum().backward()
    ref, exact = runs[True], runs[False]
    rows = [("out", out, ref[0], exact[0], OUT_BAR), ("dx", xd.grad, ref[1], exact[1], GRAD_BAR)]
    rows += [(k, q.grad, ref[2][k], exact[2][k], GRAD_BAR) for k, q in m.named_parameters()]
    bad, worst = [], (0.0, "")
    for name, got, want, ex, bar in rows:
        e, gap = rel(got, want), rel(want, ex)
        if name in ("out", "dx"):
            print(f"stack W={width} depth={depth} L={L}: {name} err {e:.2e} (restatement gap {gap:.2e}, bar {max(bar, 1.5 * gap):.2e})")
        else:
            worst = max(worst, (e, f"{name} gap {gap:.2e}"))
        if not e < max(bar, 1.5 * gap):
            bad.append((name, e, gap))
    print(f"stack W={width} depth={depth} L={L}: worst parameter gradient {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad


def _build(vt, cfg, seed):
    m = vt.make({"name": S.NAME, "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        in_grid=[cfg["frames"], cfg["side"], cfg["side"]], patch_size=cfg["patch"], tokens=cfg["tokens"])}})
    sd = S.init_state_dict(cfg, seed)
    m.load_state_dict(sd, strict=True)
    return sd, m.cuda()


def test_model_matches_restatement(vt):
    """the registered model at the reduced clip of its siblings (8x32x32, 32 latent tokens, L = 64, full 12 + 12 depth) against the
    restatement.  Free-running FSQ indices agree on >= 0.8 of the entries (the family's cap; tests/test_simple_cpu.py guards that the
    restatement alone stays within 0.10 on these seeds).  With the device's codes forced through the restatement's decoder: pred_frames
    within tol = max(3e-2, 1.5 x the restatement's emu-vs-fp32 gap); where tol < 0.15 every parameter gradient within 4 x tol.  The
    scalar mask tokens are the exception the stat model's test also makes: their exact gradient is 0 (see S.encoder3), what either side
    holds is the residue of a sum over B * rows * W entries, so it is judged against 4 x tol x the norm of the entries it sums."""
    cfg = S.make_cfg("base")
    sd, m = _build(vt, cfg, S.MODEL_SEED)
    assert len(m.encoder.model_layers.blocks) == 12 and m.encoder.width == 768
    video = torch.from_numpy(gen.video_clips(2, cfg["frames"], cfg["side"], S.VIDEO_SEED))
    up = torch.from_numpy(gen.normal((2, 3, cfg["frames"], cfg["side"], cfg["side"]), 1621))
    codes, info = m.encode(video.cuda())
    out = m(video.cuda())["pred_frames"]
    assert out.shape == video.shape and info["indices"].shape == (2, 32) and info["indices"].dtype == torch.int32
    (out * up.cuda()).sum().backward()

    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    with torch.no_grad():
        free = S.model_forward(sd, cfg, video, emu=True)
    agree = float((free["indices"] == info["indices"].cpu()).float().mean())
    print(f"model: free-running indices agree on {agree:.3f} of {free['indices'].numel()} entries")
    assert agree >= 0.8
    forced = codes.detach().cpu().float()
    taps = {}
    ref = S.model_forward(p, cfg, video, emu=True, force_codes=forced, taps=taps)
    with torch.no_grad():
        exact = S.model_forward(sd, cfg, video, emu=False, force_codes=forced)
    gap = rel(ref["pred_frames"], exact["pred_frames"])
    tol = max(3e-2, 1.5 * gap)
    e = rel(out, ref["pred_frames"])
    print(f"model: pred_frames err {e:.2e}, restatement gap {gap:.2e}, tol {tol:.2e}")
    assert e < tol, (e, gap, tol)
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())
    if tol < 0.15:
        (ref["pred_frames"] * up).sum().backward()
        named = dict(m.named_parameters())
        for k, t in taps.items():
            d = abs(float(named[k].grad) - float(p[k].grad))
            print(f"model: {k} grad {float(named[k].grad):.3e} vs {float(p[k].grad):.3e}, summed entries' norm {float(t.grad.double().norm()):.3e}")
            assert d < 4 * tol * float(t.grad.double().norm()), (k, float(named[k].grad), float(p[k].grad))
        worst = max((rel(q.grad, p[k].grad), k) for k, q in named.items() if k not in taps)
        print(f"model: worst parameter gradient {worst[0]:.2e} ({worst[1]}), bar {4 * tol:.2e}")
        assert worst[0] < 4 * tol, worst
    with torch.no_grad():
        again = m.decode_indices(info["indices"])
    assert rel(again, out) < 1e-6


def test_registry_surface_and_step_at_the_reference_geometry(vt):
    """vt.make with the yaml-style arguments: one 16x128x128 clip (1024 patch + 1024 latent tokens, 12 + 12 blocks of width 768) forward
    and backward through vt_stack_forward_rotary / vt_stack_backward_rotary"""
    m = vt.make({"name": S.NAME, "args": dict(S.YAML_ARGS)})
    assert m.prior_model is None and m.quantize.codebook_size == 64000 and len(m.encoder.model_layers.blocks) == 12
    m = m.cuda()
    video = torch.from_numpy(gen.video_clips(1, 16, 128, 1630)).cuda()
    out = m(video)["pred_frames"]
    assert out.shape == (1, 3, 16, 128, 128) and torch.isfinite(out).all()
    out.float().abs().mean().backward()
    for name, q in m.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    for side in (m.encoder, m.decoder):
        g = side.model_layers.blocks[0].attn.qkv.weight.grad
        assert float(g.abs().sum()) > 0
    codes, info = m.encode(video)
    assert codes.shape == (1, 1024, 6) and info["indices"].shape == (1, 1024)
