"""model_design's transformer stack on the GPU: the new row kernels against the passes they replace or against torch on the device, and
design.TransformerStack / Encoder / FirstFrameEncoder / UnifiedDecoder / AutoEncoder against the fixture the reference's own code wrote
(tests/golden/make_golden_design_stack.py).

Kernel bars.  vt_qkrms_rope_* is BIT-identical to the chain vt_head_rmsnorm_*(q), (k), a copy of v, vt_rope_rotate (both round at the same
points); its dq_w / dk_w are the same fp32 terms summed in another order (relative L2 1e-5) and repeat bit for bit.  vt_residual_scale_* is
bit-equal to torch's own expressions on the device; d(scale) is held against a float64 sum to 1e-5 * sum|g y| (an fp32 sum of n terms in a
tree of partials errs by a few 2^-24 of that) and repeats bit for bit.  The fp32 RMSNorm is held to 1e-6 (forward) and 1e-5 (backward)
relative L2 against the float64 formula and autograd.

Model bar, from the reference alone (as tests/test_design_gpu.py): every tensor's relative L2 distance to the reference's fp32 result is at
most 2 x the distance of the reference's OWN autocast-bf16 CPU run from it (`<tensor>_bf16_dist`).  The gradients of the 0-dim residual scales
are single numbers, and the ratio of two single draws of rounding noise is wide; they are pooled per case into one vector (d_res_scales)
before the distance is taken.  Each case prints `RATIO <case>/<tensor> <distance> <bf16_dist> <ratio>` before it asserts.

Measured ratios on an MI355X (distance / bf16_dist, bar 2; smallest and largest of each case, the outputs and the pooled scales):
  xs2 (39 tensors):            0.839 (layers.1.self_attn.q_norm) ... 1.237 (layers.1.cross_attn.k_norm); y 0.985, dx 1.029, dcontext 0.987, d_res_scales 1.207
  s1 (13 tensors):             0.422 (d_res_scales) ... 1.082 (layers.0.self_attn.norm); y 1.005, dx 1.002
  encoder (24):                0.506 (proj_out.bias) ... 1.136 (layers.3.self_attn.k_norm); tokens 0.996, dvideo 1.015, d_res_scales 0.767
  first_frame_encoder (16):    0.501 (d_res_scales) ... 1.038 (dvideo); tokens 0.919
  decoder (44):                0.582 (d_res_scales) ... 1.119 (dmain_q); pred_frames 1.006, dfirst_q 0.832
Every tensor lies where the reference's own bf16 run lies, within 24 %: two evaluations that round at the same points and sum in another order are
two draws of the same rounding noise.  The pooled scale gradients stay below the bar too (largest 1.207), so the bar is 2 for them as well.
The CPU restatement with the same rounding points lies at 0.4 - 1.47 (tests/test_design_stack_cpu.py).
"""
import pytest
import torch

from oracle import inputs as gen
from tests import design_stack_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def hip():
    import video_tokenizer_amd as vt
    return vt.hip


def _dev(a, dtype=None):
    t = torch.from_numpy(a).cuda()
    return t.to(dtype) if dtype is not None else t


# ------------------------------------------------------------------------------------------------------------------ the fused q/k pass
QK_SHAPES = [(2, 70, 2), (3, 130, 8)]


def _qk_inputs(B, L, H, seed):
    D, M = 64 * H, B * L
    Mp = (M + 63) // 64 * 64                                        # a padded buffer: rows M .. must stay as they are
    qkvg = _dev(gen.normal((Mp, 4 * D), seed), torch.bfloat16)
    q_w = _dev((1.0 + 0.2 * gen.normal((64,), seed + 1)).astype("float32"))
    k_w = _dev((1.0 + 0.2 * gen.normal((64,), seed + 2)).astype("float32"))
    cos, sin = (t.cuda() for t in R.tables(L - 8, (2, 2, 2)))
    return D, M, Mp, qkvg, q_w, k_w, cos, sin


@pytest.mark.parametrize("B,L,H", QK_SHAPES)
def test_qkrms_rope_fwd_is_the_chain_of_passes_bit_for_bit(hip, B, L, H):
    D, M, Mp, qkvg, q_w, k_w, cos, sin = _qk_inputs(B, L, H, 700 + H)
    keep = qkvg.clone()
    out = torch.full((Mp, 3 * D), 7.0, device="cuda", dtype=torch.bfloat16)
    hip.qkrms_rope_fwd(qkvg, L, H, q_w, k_w, R.EPS, cos, sin, rows=M, out=out)
    chain = torch.full((Mp, 3 * D), 7.0, device="cuda", dtype=torch.bfloat16)
    chain[:M, :D] = hip.head_rmsnorm_fwd(qkvg[:M, :D], q_w, R.EPS, H)
    chain[:M, D:2 * D] = hip.head_rmsnorm_fwd(qkvg[:M, D:2 * D], k_w, R.EPS, H)
    chain[:M, 2 * D:] = qkvg[:M, 2 * D:3 * D]
    hip.rope_rotate(chain, L, H, cos, sin, rows=M)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), chain.view(torch.int16))          # rows >= M included: still the fill value
    assert torch.equal(qkvg.view(torch.int16), keep.view(torch.int16))          # the input, its gate columns included, is only read
    assert not torch.equal(out[:M, :D], qkvg[:M, :D])


@pytest.mark.parametrize("B,L,H", QK_SHAPES)
def test_qkrms_rope_bwd_is_the_chain_of_passes(hip, B, L, H):
    D, M, Mp, qkvg, q_w, k_w, cos, sin = _qk_inputs(B, L, H, 720 + H)
    dqkv = _dev(gen.normal((M, 3 * D), 740 + H), torch.bfloat16)

    def fused(want_dw=True):
        dqkvg = torch.full((Mp, 4 * D), 7.0, device="cuda", dtype=torch.bfloat16)
        dw = hip.qkrms_rope_bwd(qkvg, dqkv, L, H, q_w, k_w, R.EPS, cos, sin, dqkvg, want_dw=want_dw)
        return dqkvg, dw
    dqkvg, (dq_w, dk_w) = fused()
    rot = hip.rope_rotate(dqkv.clone(), L, H, cos, sin, conjugate=True)
    chain = torch.full((Mp, 4 * D), 7.0, device="cuda", dtype=torch.bfloat16)
    _, cq_w = hip.head_rmsnorm_bwd(rot[:, :D], qkvg[:M, :D], q_w, R.EPS, H, dx=chain[:M, :D])
    _, ck_w = hip.head_rmsnorm_bwd(rot[:, D:2 * D], qkvg[:M, D:2 * D], k_w, R.EPS, H, dx=chain[:M, D:2 * D])
    chain[:M, 2 * D:3 * D] = dqkv[:, 2 * D:]
    torch.cuda.synchronize()
    assert torch.equal(dqkvg.view(torch.int16), chain.view(torch.int16))        # columns 3D.. and rows >= M: still the fill value
    for got, want in ((dq_w, cq_w), (dk_w, ck_w)):
        d = R.rel_l2(got.cpu(), want.cpu())
        print(f"DW rel_l2 {d:.3e}")
        assert d <= 1e-5
    again, (dq2, dk2) = fused()
    assert torch.equal(dq2, dq_w) and torch.equal(dk2, dk_w) and torch.equal(again.view(torch.int16), dqkvg.view(torch.int16))
    nodw, (n1, n2) = fused(want_dw=False)                                       # NULL dq_w / dk_w
    assert n1 is None and n2 is None and torch.equal(nodw.view(torch.int16), dqkvg.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ the scaled residual
@pytest.mark.parametrize("dim", [128, 512])
@pytest.mark.parametrize("rows", [1, 140, 333])
def test_residual_scale_is_torchs_expression_on_the_device(hip, rows, dim):
    x = _dev(gen.normal((rows, dim), 800 + rows))
    y = _dev(gen.normal((rows, dim), 801 + rows), torch.bfloat16)
    g = _dev(gen.normal((rows, dim), 802 + rows))
    s = torch.tensor(0.57731234, device="cuda")
    out = hip.residual_scale_fwd(x, y.float(), s)
    assert torch.equal(out, x + (s * y))                                         # a 0-dim fp32 tensor times a bf16 tensor is a bf16 tensor
    gb = g.bfloat16()

    def bwd(want_ds=True):
        return hip.residual_scale_bwd(g, y.float() if want_ds else None, s, want_ds=want_ds)
    dy, ds = bwd()
    assert torch.equal(dy, (s * gb).float())
    ref = (gb.double() * y.double()).sum()
    mag = (gb.double() * y.double()).abs().sum()
    err = abs(ds.double() - ref).item()
    print(f"DS rows {rows} dim {dim}: {ds.item():.6f} ref {ref.item():.6f} err {err:.3e} bar {1e-5 * mag.item():.3e}")
    assert ds.dim() == 0 and err <= 1e-5 * mag.item()
    dy2, ds2 = bwd()
    assert torch.equal(ds2, ds) and torch.equal(dy2, dy)
    dy3, none = bwd(want_ds=False)                                               # NULL dscale: a frozen scale
    assert none is None and torch.equal(dy3, dy)


def test_residual_scale_function_gradients():
    import video_tokenizer_amd.functional as F_
    x = _dev(gen.normal((2, 35, 128), 820)).requires_grad_(True)
    y = _dev(gen.normal((2, 35, 128), 821), torch.bfloat16).float().requires_grad_(True)
    s = torch.tensor(0.8125, device="cuda", requires_grad=True)                # exact in bf16
    w = _dev(gen.normal((2, 35, 128), 822), torch.bfloat16).float()
    (F_.ResidualScale.apply(x, y, s) * w).sum().backward()
    assert torch.equal(x.grad, w) and torch.equal(y.grad, (0.8125 * w).bfloat16().float())
    assert abs(s.grad.item() - (w.double() * y.detach().double()).sum().item()) <= 1e-5 * (w * y.detach()).abs().sum().item()


# ------------------------------------------------------------------------------------------------------------------ the fp32 RMSNorm
@pytest.mark.parametrize("rows,dim", [(141, 128), (70, 512)])
def test_rmsnorm_f32_matches_float64(hip, rows, dim):
    x = _dev(gen.normal((rows, dim), 840 + dim))
    w = _dev((1.0 + 0.2 * gen.normal((dim,), 841 + dim)).astype("float32"))
    g = _dev(gen.normal((rows, dim), 842 + dim))
    y, rstd = hip.rmsnorm_any_f32_fwd(x, w, R.EPS)
    dx, dw = hip.rmsnorm_any_f32_bwd(g, x, w, rstd)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + R.EPS) * w64
    (y64 * g.double()).sum().backward()
    assert y.dtype == torch.float32 and R.rel_l2(y.cpu(), y64.detach().cpu()) <= 1e-6
    assert R.rel_l2(dx.cpu(), x64.grad.cpu()) <= 1e-5 and R.rel_l2(dw.cpu(), w64.grad.cpu()) <= 1e-5
    dx2, dw2 = hip.rmsnorm_any_f32_bwd(g, x, w, rstd)
    assert torch.equal(dw2, dw) and torch.equal(dx2, dx)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_new_kernels_refuse_bad_arguments(hip):
    B, L, H = 1, 16, 2
    D, M = 64 * H, B * L
    cos, sin = (t.cuda() for t in R.tables(8, (2, 2, 2)))
    w = torch.ones(64, device="cuda")
    flat = torch.zeros(M * (4 * D + 4) + 64, device="cuda", dtype=torch.bfloat16)
    good = flat[:M * 4 * D].view(M, 4 * D)
    hip.qkrms_rope_fwd(good, L, H, w, w, R.EPS, cos, sin)
    with pytest.raises(hip.HipError, match="vt_qkrms_rope_fwd: buffers must be 16-byte aligned"):
        hip.qkrms_rope_fwd(flat[4:4 + M * 4 * D].view(M, 4 * D), L, H, w, w, R.EPS, cos, sin)
    with pytest.raises(hip.HipError, match="vt_qkrms_rope_fwd: row strides .* multiples of 8"):
        hip.qkrms_rope_fwd(flat[:M * (4 * D + 4)].view(M, 4 * D + 4)[:, :4 * D], L, H, w, w, R.EPS, cos, sin)
    dqkv = torch.zeros(M, 3 * D, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(hip.HipError, match="vt_qkrms_rope_bwd: row strides .* multiples of 8"):
        hip.qkrms_rope_bwd(good, dqkv, L, H, w, w, R.EPS, cos, sin, torch.zeros_like(flat)[:M * (4 * D + 4)].view(M, 4 * D + 4)[:, :4 * D])
    with pytest.raises(hip.HipError, match="vt_qkrms_rope_bwd: buffers must be 16-byte aligned"):
        hip.qkrms_rope_bwd(good, dqkv, L, H, w, w, R.EPS, cos, sin, torch.zeros_like(flat)[4:4 + M * 4 * D].view(M, 4 * D))
    s = torch.tensor(0.5, device="cuda")
    f = torch.zeros(8 * 128 + 8, device="cuda")
    with pytest.raises(hip.HipError, match="vt_residual_scale_fwd: .* dim % 4 == 0"):
        hip.residual_scale_fwd(f[:60].view(10, 6), f[64:124].view(10, 6), s)
    with pytest.raises(hip.HipError, match="vt_residual_scale_fwd: buffers must be 16-byte aligned"):
        hip.residual_scale_fwd(f[1:1 + 512].view(4, 128), torch.zeros(4, 128, device="cuda"), s)
    with pytest.raises(hip.HipError, match="vt_residual_scale_bwd: .* dim % 4 == 0"):
        hip.residual_scale_bwd(f[:60].view(10, 6), f[64:124].view(10, 6), s)
    with pytest.raises(hip.HipError, match="vt_rmsnorm_any_f32_fwd: width 192 unsupported"):
        hip.rmsnorm_any_f32_fwd(torch.zeros(4, 192, device="cuda"), torch.ones(192, device="cuda"), R.EPS)
    with pytest.raises(hip.HipError, match="vt_rmsnorm_any_f32_fwd: buffers must be 16-byte aligned"):
        hip.rmsnorm_any_f32_fwd(f[1:1 + 512].view(4, 128), torch.ones(128, device="cuda"), R.EPS)
    for call in (lambda: hip.qkrms_rope_fwd(good.cpu(), L, H, w, w, R.EPS, cos, sin),
                 lambda: hip.residual_scale_fwd(torch.zeros(4, 128), torch.zeros(4, 128), s),
                 lambda: hip.residual_scale_bwd(torch.zeros(4, 128), torch.zeros(4, 128), s),
                 lambda: hip.rmsnorm_any_f32_fwd(torch.zeros(4, 128), torch.ones(128), R.EPS)):
        with pytest.raises(hip.HipError, match="GPU tensors only"):
            call()


# ------------------------------------------------------------------------------------------------------------------ the stack
def _compare(got, golden, prefix):
    failures = []
    for t, v in got.items():
        want = torch.from_numpy(golden[f"{prefix}{t}"])
        assert v is not None and tuple(v.shape) == tuple(want.shape), t
        d, bar = R.rel_l2(v.cpu(), want), float(golden[f"{prefix}{t}_bf16_dist"])
        print(f"RATIO {prefix}{t} {d:.3e} {bar:.3e} {d / bar:.3f}")
        if not d <= 2 * bar:
            failures.append((t, d, bar))
    assert not failures, failures


def _stack(case):
    import video_tokenizer_amd as vt
    c = R.STACK_CASES[case]
    I = {k: torch.from_numpy(v) for k, v in R.stack_inputs(case).items()}
    m = vt.TransformerStack(c["dim"], heads=c["heads"], mlp_ratio=c["mlp_ratio"], num_layers=c["num_layers"], has_cross_attn=c["cross"])
    names = list(R.stack_param_shapes(c["dim"], c["mlp_ratio"], c["num_layers"], c["cross"]))
    assert list(m.state_dict().keys()) == names
    m.load_state_dict({n: I[n] for n in names}, strict=True)                    # the reference's keys
    return m.cuda(), I, names, tuple(t.cuda() for t in R.tables(c["tokens"], c["grid"]))


def _stack_step(m, I, names, tabs):
    x = I["x"].cuda().requires_grad_(True)
    ctx = I["context"].cuda().requires_grad_(True) if "context" in I else None
    m.zero_grad(set_to_none=True)
    y = m(x, tabs, context=ctx)
    (y * I["w"].cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters()}
    return y, x.grad, ctx.grad if ctx is not None else None, grads


@pytest.mark.parametrize("case", list(R.STACK_CASES))
def test_stack_matches_the_reference_within_its_own_bf16_distance(golden, case):
    m, I, names, tabs = _stack(case)
    y, dx, dctx, grads = _stack_step(m, I, names, tabs)
    assert y.dtype == torch.float32 and dx.dtype == torch.float32
    got = R.collect(y, {"dx": dx, "dcontext": dctx}, grads, names)
    assert {f"{case}/{t}" for t in got} == {k for k in golden if k.startswith(case + "/") and not k.endswith("_bf16_dist")}
    _compare(got, golden, case + "/")
    y2, dx2, dctx2, grads2 = _stack_step(m, I, names, tabs)                      # a second step reproduces every bit
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and (dctx is None or torch.equal(dctx2, dctx))
    for n in names:
        assert torch.equal(grads2[n], grads[n]), n


def test_stack_frozen_parameters_skip_their_gradient():
    m, I, names, tabs = _stack("xs2")
    y, dx, dctx, full = _stack_step(m, I, names, tabs)
    frozen = ("layers.0.res_scale_sa", "layers.1.res_scale_ca", "layers.1.res_scale_ffn", "layers.0.self_attn.to_gate.weight", "layers.0.self_attn.k_norm.weight",
              "layers.1.self_attn.out_proj.weight", "layers.0.ffn.1.weight", "layers.1.ffn.0.weight", "layers.1.cross_attn.to_kv.weight", "final_norm.weight")
    for n in frozen:
        m.get_parameter(n).requires_grad_(False)
    y2, dx2, dctx2, part = _stack_step(m, I, names, tabs)
    for n in names:
        if n in frozen:
            assert part[n] is None, n
        else:
            assert torch.equal(part[n], full[n]), n
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and torch.equal(dctx2, dctx)
    with torch.no_grad():                                                        # context None: the cross branch is skipped, as in the reference
        y3 = m(I["x"].cuda(), tabs, context=None)
    assert y3.shape == y.shape and not torch.equal(y3, y)


# ------------------------------------------------------------------------------------------------------------------ the modules
def _modules():
    import video_tokenizer_amd as vt
    g = R.MOD
    I = {k: torch.from_numpy(v) for k, v in R.mod_inputs().items()}
    mods = {"encoder": vt.Encoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=3, out_channels=g["token_size"], in_grid=g["in_grid"],
                                  out_tokens=g["tokens"]),
            "first_frame_encoder": vt.FirstFrameEncoder(model_size=g["model_size"], patch_size_hw=g["patch_size"][1:], in_channels=3,
                                                        out_channels=g["token_size"], in_hw=g["in_grid"][1:], out_tokens=g["cond_tokens"]),
            "decoder": vt.UnifiedDecoder(model_size=g["model_size"], patch_size=g["patch_size"], in_channels=g["token_size"], out_channels=3,
                                         in_tokens=g["tokens"], cond_tokens=g["cond_tokens"], out_grid=g["in_grid"])}
    shapes = R.mod_shapes()
    for k, m in mods.items():
        sd = m.state_dict()
        assert list(sd.keys()) == list(shapes[k]) and all(tuple(sd[n].shape) == shapes[k][n] for n in sd), k
        m.load_state_dict({n: I[f"{k}.{n}"] for n in shapes[k]}, strict=True)   # the reference's keys
        back = m.state_dict()
        assert all(torch.equal(back[n], I[f"{k}.{n}"]) for n in shapes[k]), k   # round trip
        m.cuda()
    return mods, I, shapes


def test_modules_match_the_reference_within_its_own_bf16_distance(golden):
    mods, I, shapes = _modules()
    for k, w in (("encoder", "w_main"), ("first_frame_encoder", "w_first")):
        video = I["video"].cuda().requires_grad_(True)
        tok = mods[k](video if k == "encoder" else video[:, :, 0:1])
        (tok * I[w].cuda()).sum().backward()
        got = R.collect(tok, {"dvideo": video.grad}, {n: p.grad for n, p in mods[k].named_parameters()}, list(shapes[k]), small_only=True, y_name="tokens")
        assert {f"{k}/{t}" for t in got} == {n for n in golden if n.startswith(k + "/") and not n.endswith("_bf16_dist")}
        _compare(got, golden, k + "/")
    mq, fq = (torch.from_numpy(golden[n]).cuda().requires_grad_(True) for n in ("mod/main_q", "mod/first_q"))
    pred = mods["decoder"](mq, cond=fq)
    (pred * I["w_pred"].cuda()).sum().backward()
    got = R.collect(pred, {"dmain_q": mq.grad, "dfirst_q": fq.grad}, {n: p.grad for n, p in mods["decoder"].named_parameters()}, list(shapes["decoder"]),
                    small_only=True, y_name="pred_frames")
    assert {f"decoder/{t}" for t in got} == {n for n in golden if n.startswith("decoder/") and not n.endswith("_bf16_dist")}
    _compare(got, golden, "decoder/")
    with pytest.raises(ValueError, match="no cond provided"):
        mods["decoder"](mq)


def test_autoencoder_design_end_to_end():
    """The pieces on each side of the quantiser are compared above; across FSQ one flipped code is a legitimate large difference, so the whole
    model is checked for consistency with itself."""
    import video_tokenizer_amd as vt
    g = R.MOD
    torch.manual_seed(3)
    m = vt.make({"name": "autoencoder_design", "args": {"bottleneck": None, "prior_model": None, "num_latent_tokens": 1024,
                                                          "_geometry": dict(in_grid=list(g["in_grid"]), patch_size=list(g["patch_size"]), tokens=g["tokens"],
                                                                            cond_tokens=g["cond_tokens"], model_size=g["model_size"])}}).cuda()
    assert isinstance(m, vt.AutoEncoder)
    x = _dev(gen.video_clips(g["B"], g["in_grid"][0], g["in_grid"][1], 901).astype("float32"))
    main_q, first_q, main_idx, first_idx = m.encode(x)
    assert main_q.shape == (g["B"], g["tokens"], 6) and first_q.shape == (g["B"], g["cond_tokens"], 6)
    out = m(x)
    assert set(out) == {"pred_frames"} and out["pred_frames"].shape == x.shape
    assert torch.equal(out["pred_frames"], m.decode(main_q, first_q))
    assert torch.equal(m.decode_from_indices(main_idx, first_idx), m.decode(main_q, first_q))
    assert torch.equal(m.decode_from_indices(main_idx["indices"], first_idx["indices"]), m.decode(main_q, first_q))
    out["pred_frames"].square().mean().backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
