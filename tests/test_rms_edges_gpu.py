"""The row passes of the three newest model families at their edges: the whole-row RMSNorm families (csrc/vt_rmsnorm.h), the per-head
RMSNorm (csrc/vt_cross.hip), the fused q/k RMS-norm + rotary pass and the scaled residual (csrc/vt_design.hip), the rotary pass of the plain
stack (csrc/vt_rope.hip) and SwiGLU (csrc/vt_ar.hip), against the float64 references, bars and share conditions of tests/rms_cases.py (whose
power tests/test_rms_cases_cpu.py proves without a kernel).  What the shapes are for:

    entry point                                   launch cap                                 a case past it
    vt_rmsnorm*_fwd                               2048 blocks x 4 rows                       8197 rows at widths 128, 768, 2560
    vt_rmsnorm*_bwd                               256 blocks x 4 rows                        1029 rows at every width
    vt_head_rmsnorm_fwd / vt_qkrms_rope_fwd       2048 blocks x 32 head vectors              (8193, 8) / (5, 1640, 8)
    vt_head_rmsnorm_bwd / vt_qkrms_rope_bwd       512 blocks x 32 head vectors               (2049, 8) / (2, 1025, 8)
    vt_rope_rotate                                4096 blocks x 256 / min(16 H, 256) rows    65537 rows at H = 1, 4097 at H = 16; 272 pieces at H = 17
    vt_residual_scale_fwd / _bwd                  4096 / 256 blocks x 256 float4             (8193, 512) / (2049, 128)
    vt_swiglu_fwd / _bwd                          4096 blocks x 256 units of 8 columns       (4100, 2048)

Common to every case, as in tests/test_gated_edges_gpu.py: every output and workspace is a view into a larger allocation that holds a
poison bit pattern before the call, and everything outside the documented output region keeps it (row padding, the other column blocks,
TAIL rows behind the tensor, the gate columns of the [M, 4D] gradient: the reference quantity is the whole backing buffer, bar 0 there);
padding of inputs is NaN and reaches no output; inputs keep their bits; a second call reproduces every output bit.  Optional operands are
absent in turn (rstd NULL in the forward; dres absent or present by case; dx, dxb, or both; dq_w / dk_w NULL; dscale NULL with y and the
workspace NULL), and what is written then has the bits of the full call.  The partial-sum workspaces hold poison before the call, so a
block that owns no row must write its zeros for the sums to come out.

After the module's tests a fixture prints the worst error / bar per kernel and quantity (profiles/rms_edges_err_over_bar.txt holds one run).
A one-rounding bar is reached to within a few per cent by construction (a value just above a power of two that rounds by half a step), so
ratios near 1 on the bf16 outputs (y, dxb, out, dqkvg, qkv, a, dh) say nothing about slack; the fp32 outputs (rstd, dx of the whole-row
families), the exact ones (ratio 0 or failure) and the column sums show the real margin."""
import collections

import pytest
import torch

from tests import rms_cases as R
from tests.test_gated_edges_gpu import _at, _bits, _is_poison, _p16, _p32, _same_bits

pytestmark = pytest.mark.gpu
WORST = collections.OrderedDict()


@pytest.fixture(scope="module", autouse=True)
def worst_error_over_bar():
    """after the module's tests: the table of profiles/rms_edges_err_over_bar.txt for whatever part of the file was run"""
    yield
    print("\nworst error / bar per kernel and quantity over the cases of tests/test_rms_edges_gpu.py that ran")
    for (kernel, nm), r in WORST.items():
        print(f"RMS_EDGES {kernel:18s} {nm:8s} {r:.3f}")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _judge(bars, got):
    """every asserted quantity within its bar, every share condition met; records the worst ratio"""
    kernel = bars.case.kernel
    for nm, r in bars.ratios(got).items():
        if r is None:
            continue
        key = (kernel, nm)
        WORST[key] = max(WORST.get(key, 0.0), r)
        print(f"{bars.case.name} {nm}: error / bar = {r:.3f}")
        assert r <= 1.0, (bars.case.name, nm, r)
    for nm, q in bars.q.items():
        if nm in got and q.tight is not None:
            s = q.share(got[nm])
            assert s <= R.SHARE, (bars.case.name, nm, s)


def _kept(dev, host):
    return torch.equal(_bits(dev.cpu()), _bits(host))


@pytest.mark.parametrize("name", [n for f in R.RMS_FAMILIES for n in R.names(f)])
def test_rmsnorm_edges(hip, name):
    b = R.bars(name)
    c = b.case
    rows, dim, T = c.rows, c.dim, c.rows + R.TAIL
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    fwd, bwd = getattr(lib, f"vt_{c.kernel}_fwd"), getattr(lib, f"vt_{c.kernel}_bwd")
    nws = getattr(lib, f"vt_{c.kernel}_bwd_workspace_bytes")(dim) // 4
    x, dy, w, rstd_in = c.x.cuda(), c.dy.cuda(), c.w.cuda(), c.rstd_in.cuda()
    dres = c.dres.cuda() if c.has_dres else None
    pout = _p16 if c.bf else _p32

    def forward(with_rstd=True):
        y, rstd = pout(T, dim), _p32(T)
        hip.check(fwd(ptr(x), ptr(w), c.eps, rows, dim, ptr(y), ptr(rstd) if with_rstd else None, st), "fwd")
        torch.cuda.synchronize()
        return y, rstd

    def backward(want_dx=True, want_dxb=True):
        dx, dxb, dw, ws = _p32(T, dim), _p16(T, dim), _p32(dim + 8), _p32(nws)
        if c.bf:
            hip.check(bwd(ptr(dy), ptr(x), ptr(w), ptr(rstd_in), ptr(dres), rows, dim, ptr(dx) if want_dx else None, ptr(dxb) if want_dxb else None,
                          ptr(dw), ptr(ws), st), "bwd")
        else:
            hip.check(bwd(ptr(dy), ptr(x), ptr(w), ptr(rstd_in), rows, dim, ptr(dx), ptr(dw), ptr(ws), st), "bwd")
        torch.cuda.synchronize()
        return dx, dxb, dw

    y, rstd = forward()
    assert _same_bits(forward(), (y, rstd))
    y0, rstd0 = forward(with_rstd=False)                                   # rstd NULL: the same y, nothing else written
    assert _same_bits((y0,), (y,)) and _is_poison(rstd0)
    dx, dxb, dw = backward()
    assert _same_bits(backward(), (dx, dxb, dw))
    assert _is_poison(dw[dim:])
    got = {"y": y.cpu(), "rstd": rstd.cpu(), "dx": dx.cpu(), "dw": dw[:dim].cpu()}
    if c.bf:
        got["dxb"] = dxb.cpu()
        a = backward(want_dxb=False)                                       # dx alone, dxb alone: the bits of the full call
        assert _same_bits((a[0], a[2]), (dx, dw)) and _is_poison(a[1])
        a = backward(want_dx=False)
        assert _same_bits((a[1], a[2]), (dxb, dw)) and _is_poison(a[0])
    else:
        assert _is_poison(dxb)
    assert _kept(x, c.x) and _kept(dy, c.dy) and _kept(rstd_in, c.rstd_in) and (dres is None or _kept(dres, c.dres))
    assert bool(torch.isfinite(y[:rows].float()).all()) and bool(torch.isfinite(dx[:rows]).all()) and bool(torch.isfinite(dw[:dim]).all())
    _judge(b, got)


@pytest.mark.parametrize("name", R.names("head_rmsnorm"))
def test_head_rmsnorm_edges(hip, name):
    b = R.bars(name)
    c = b.case
    M, H, W, T = c.M, c.H, 64 * c.H, c.M + R.TAIL
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    x, dy, w = c.x.cuda(), c.dy.cuda(), c.w.cuda()
    nws = lib.vt_head_rmsnorm_bwd_workspace_bytes() // 4

    def call(in_place=False):
        y, dx, dw, ws = _p16(T, c.y_rs), dy.clone() if in_place else _p16(T, c.dx_rs), _p32(64 + 8), _p32(nws)
        src = dx if in_place else dy
        hip.check(lib.vt_head_rmsnorm_fwd(ptr(x), c.x_rs, ptr(w), c.eps, M, H, ptr(y), c.y_rs, st), "vt_head_rmsnorm_fwd")
        hip.check(lib.vt_head_rmsnorm_bwd(ptr(src), c.dy_rs, ptr(x), c.x_rs, ptr(w), c.eps, M, H, ptr(dx), c.dy_rs if in_place else c.dx_rs, ptr(dw), ptr(ws),
                                          st), "vt_head_rmsnorm_bwd")
        torch.cuda.synchronize()
        return y, dx, dw

    y, dx, dw = call()
    assert _same_bits(call(), (y, dx, dw))
    assert _kept(x, c.x) and _kept(dy, c.dy) and _is_poison(dw[64:])
    _, dxi, dwi = call(in_place=True)                                       # dx == dy: the same bits, and dy's padding keeps its own
    assert _same_bits((dxi[:M, :W], dwi), (dx[:M, :W], dw))
    assert torch.equal(_bits(dxi[:M, W:]), _bits(dy[:M, W:])) and torch.equal(_bits(dxi[M:]), _bits(dy[M:]))
    assert bool(torch.isfinite(y[:M, :W].float()).all()) and bool(torch.isfinite(dx[:M, :W].float()).all()) and bool(torch.isfinite(dw[:64]).all())
    _judge(b, {"y": y.cpu(), "dx": dx.cpu(), "dw": dw[:64].cpu()})


@pytest.mark.parametrize("name", R.names("qkrms_rope"))
def test_qkrms_rope_edges(hip, name):
    b = R.bars(name)
    c = b.case
    M, L, H, D, T = c.M, c.L, c.H, c.D, c.M + R.TAIL
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    back, upb = c.backing.cuda(), c.up_backing.cuda()
    par = [p.cuda() for p in c.params]
    cos, sin = c.cos_ext.cuda(), c.sin_ext.cuda()            # the kernel's tables are rows [0, L) of these
    nws = lib.vt_qkrms_rope_bwd_workspace_bytes() // 4

    def call(want_dw=True):
        out, dq, grads, ws = _p16(T, c.out_rs), _p16(T, c.dq_rs), _p32(2, 64), _p32(nws)
        hip.check(lib.vt_qkrms_rope_fwd(ptr(back), c.in_rs, M, L, H, ptr(par[0]), ptr(par[1]), c.eps, ptr(cos), ptr(sin), ptr(out), c.out_rs, st),
                  "vt_qkrms_rope_fwd")
        hip.check(lib.vt_qkrms_rope_bwd(ptr(back), c.in_rs, ptr(upb), M, L, H, ptr(par[0]), ptr(par[1]), c.eps, ptr(cos), ptr(sin), ptr(dq), c.dq_rs,
                                        ptr(grads[0]) if want_dw else None, ptr(grads[1]) if want_dw else None, ptr(ws), st), "vt_qkrms_rope_bwd")
        torch.cuda.synchronize()
        return out, dq, grads

    out, dq, grads = call()
    assert _same_bits(call(), (out, dq, grads))
    o0, d0, g0 = call(want_dw=False)                                        # dq_w, dk_w NULL: the same rows, no sums
    assert _same_bits((o0, d0), (out, dq)) and _is_poison(g0)
    assert _kept(back, c.backing) and _kept(upb, c.up_backing)
    assert torch.equal(_bits(out[:M, 2 * D:3 * D]), _bits(back[:M, 2 * D:3 * D]))              # v and its gradient: copies, bit for bit
    assert torch.equal(_bits(dq[:M, 2 * D:3 * D]), _bits(upb[:M, 2 * D:]))
    assert _is_poison(dq[:M, 3 * D:]) and _is_poison(out[:M, 3 * D:]) and _is_poison(out[M:]) and _is_poison(dq[M:])
    assert bool(torch.isfinite(dq[:M, :3 * D].float()).all()) and bool(torch.isfinite(out[:M, :3 * D].float()).all()) and bool(torch.isfinite(grads).all())
    got = {"out": out.cpu(), "dqkvg": dq.cpu()}
    got.update({nm: grads[i].cpu() for i, nm in enumerate(R.QKR_COLS)})
    _judge(b, got)


@pytest.mark.parametrize("name", R.names("rope_rotate"))
def test_rope_rotate_edges(hip, name):
    b = R.bars(name)
    c = b.case
    M, L, H = c.M, c.L, c.H
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    cos, sin = c.cos_ext.cuda(), c.sin_ext.cuda()

    def call(conj, src=None):
        buf = (c.qkv.cuda() if src is None else src.clone())
        hip.check(lib.vt_rope_rotate(ptr(buf), c.ld, M, L, H, ptr(cos), ptr(sin), conj, st), "vt_rope_rotate")       # rows [0, M) of M + TAIL
        torch.cuda.synchronize()
        return buf

    y = call(c.conj)
    assert _same_bits((call(c.conj),), (y,))
    assert torch.equal(_bits(y[M:]), _bits(c.qkv[M:].cuda())) and torch.equal(_bits(y[:M, 128 * H:]), _bits(c.qkv[:M, 128 * H:].cuda()))
    _judge(b, {"qkv": y.cpu()})
    if not c.conj:
        # the conjugate of the forward restores the input to one bf16 rounding per element: the forward's rounding of the pair (2^-8 of each
        # component, carried through a rotation: at most their sum), the final rounding of the restored value, and the fp32 floor twice
        z = call(1, y)[:M, :128 * H].cpu().double()
        xin = c.qkv[:M, :128 * H].double()
        want = b.q["qkv"].want[:M, :128 * H].abs().reshape(M, 2 * H, 32, 2)
        pair = want.sum(-1, keepdim=True).expand(M, 2 * H, 32, 2).reshape(M, 128 * H)
        mag = xin.abs().reshape(M, 2 * H, 32, 2).sum(-1, keepdim=True).expand(M, 2 * H, 32, 2).reshape(M, 128 * H)
        bound = 2.0 ** -8 * (1 + 2.0 ** -7) * (pair + xin.abs()) + 2 * R.FLOOR * mag
        r = float(((z - xin).abs() / bound.clamp(min=1e-300)).max())
        WORST[("rope_rotate", "restored")] = max(WORST.get(("rope_rotate", "restored"), 0.0), r)
        assert r <= 1.0, r


@pytest.mark.parametrize("name", R.names("residual_scale"))
def test_residual_scale_edges(hip, name):
    b = R.bars(name)
    c = b.case
    rows, dim, T = c.rows, c.dim, c.rows + R.TAIL
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    x, yv, dout, scale = c.x.cuda(), c.y.cuda(), c.dout.cuda(), c.scale.cuda()
    nws = lib.vt_residual_scale_bwd_workspace_bytes() // 4

    def call(want_ds=True):
        out, dy, ds, ws = _p32(T, dim), _p32(T, dim), _p32(8), _p32(nws)
        hip.check(lib.vt_residual_scale_fwd(ptr(x), ptr(yv), ptr(scale), rows, dim, ptr(out), st), "vt_residual_scale_fwd")
        hip.check(lib.vt_residual_scale_bwd(ptr(dout), ptr(yv) if want_ds else None, ptr(scale), rows, dim, ptr(dy), ptr(ds) if want_ds else None,
                                            ptr(ws) if want_ds else None, st), "vt_residual_scale_bwd")
        torch.cuda.synchronize()
        return out, dy, ds, ws

    out, dy, ds, ws = call()
    assert _same_bits(call()[:3], (out, dy, ds))
    o0, d0, s0, w0 = call(want_ds=False)                                    # a frozen scale: y and workspace NULL, the same dy
    assert _same_bits((o0, d0), (out, dy)) and _is_poison(s0) and _is_poison(w0)
    nblk = min((rows * dim // 4 + 255) // 256, nws)
    assert _is_poison(ds[1:]) and _is_poison(ws[nblk:])                     # one partial per block that ran, nothing behind them
    assert _kept(x, c.x) and _kept(yv, c.y) and _kept(dout, c.dout) and _kept(scale, c.scale)
    _judge(b, {"out": out.cpu(), "dy": dy.cpu(), "dscale": ds[:1].cpu()})


@pytest.mark.parametrize("name", R.names("swiglu"))
def test_swiglu_edges(hip, name):
    b = R.bars(name)
    c = b.case
    M, I, T = c.M, c.I, c.M + R.TAIL
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    h, da = c.h.cuda(), c.da.cuda()

    def call():
        a, dh = _p16(T, I), _p16(T, 2 * I)
        hip.check(lib.vt_swiglu_fwd(ptr(h), M, I, ptr(a), st), "vt_swiglu_fwd")
        hip.check(lib.vt_swiglu_bwd(ptr(da), ptr(h), M, I, ptr(dh), st), "vt_swiglu_bwd")
        torch.cuda.synchronize()
        return a, dh

    a, dh = call()
    assert _same_bits(call(), (a, dh))
    assert _kept(h, c.h) and _kept(da, c.da) and _is_poison(a[M:]) and _is_poison(dh[M:])
    assert bool(torch.isfinite(a[:M].float()).all()) and bool(torch.isfinite(dh[:M].float()).all())
    _judge(b, {"a": a.cpu(), "dh": dh.cpu()})


def test_edge_shapes_are_not_refused_and_bad_ones_launch_nothing(hip):
    """the smallest legal problems pass the argument checks (the cases above run them); these do not, and leave their outputs untouched"""
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    f = torch.zeros(4096, device="cuda")
    g = torch.zeros(8, 1024, dtype=torch.bfloat16, device="cuda")
    o32, o16 = _p32(4096), _p16(8, 1024)
    assert lib.vt_rmsnorm_fwd(ptr(f), ptr(f), 1e-5, 1, 128, ptr(o16), None, st) == -1                     # 128 is not a llama-abs width
    assert lib.vt_rmsnorm_any_fwd(ptr(f), ptr(f), 1e-6, 1, 192, ptr(o16), None, st) == -1
    assert lib.vt_rmsnorm_any_bwd(ptr(g), ptr(f), ptr(f), ptr(f), None, 1, 128, None, None, ptr(o32), ptr(o32), st) == -1      # neither dx nor dxb
    assert lib.vt_rmsnorm_any_f32_fwd(_at(f, 1), ptr(f), 1e-6, 1, 128, ptr(o32), None, st) == -1          # a misaligned x
    assert lib.vt_head_rmsnorm_fwd(ptr(g), 56, ptr(f), 1e-6, 4, 1, ptr(o16), 64, st) == -1                # x_rs < 64 H
    assert lib.vt_head_rmsnorm_bwd(ptr(g), 64, ptr(g), 64, ptr(f), 1e-6, 4, 1, ptr(g), 64, ptr(o32), ptr(o32), st) == -1       # dx overlaps x
    assert lib.vt_qkrms_rope_fwd(ptr(g), 256, 6, 4, 1, ptr(f), ptr(f), 1e-6, ptr(f), ptr(f), ptr(o16), 192, st) == -1          # M % L != 0
    assert lib.vt_qkrms_rope_fwd(ptr(g), 184, 4, 4, 1, ptr(f), ptr(f), 1e-6, ptr(f), ptr(f), ptr(o16), 192, st) == -1          # in_rs < 3D
    assert lib.vt_rope_rotate(ptr(o16), 120, 4, 4, 1, ptr(f), ptr(f), 0, st) == -1                        # ld < 128 H
    assert lib.vt_rope_rotate(ptr(o16), 128, 4, 4, 1, ptr(f), ptr(f), 2, st) == -1
    assert lib.vt_residual_scale_fwd(ptr(f), ptr(f), ptr(f), 1, 6, ptr(o32), st) == -1                    # dim % 4 != 0
    assert lib.vt_residual_scale_bwd(ptr(f), None, ptr(f), 1, 4, ptr(o32), ptr(o32), ptr(o32), st) == -1  # dscale without y
    assert lib.vt_swiglu_fwd(ptr(g), 1, 12, ptr(o16), st) == -1 and lib.vt_swiglu_bwd(ptr(g), ptr(g), 1, 12, ptr(o16), st) == -1   # I % 8 != 0
    torch.cuda.synchronize()
    assert _is_poison(o32) and _is_poison(o16)
