"""The row passes of csrc/vt_gated.hip (qknorm_rope, the sigmoid gates, GEGLU) and csrc/vt_stat.hip (the token gate) at their edges, against
the float64 references, bars and share conditions of tests/gated_cases.py (whose power tests/test_gated_cases_cpu.py proves without a
kernel).  Common to every case: outputs and workspaces hold a poison bit pattern before the call and everything outside the documented
output region keeps it (row padding, the other column blocks, rows behind the tensor: every tensor is a view of a larger allocation);
padding of inputs is NaN and reaches no output; inputs keep their bits; a second call reproduces every output bit.

After the module's tests a fixture prints the worst error / bar per kernel and quantity (profiles/gated_edges_err_over_bar.txt holds one run).
A one-rounding bar is reached to within a few per cent by construction (a value just above a power of two that rounds by half a step), so
ratios near 1 on the bf16 outputs say nothing about slack; the column sums and fp32 outputs show the real margin."""
import collections
import ctypes

import pytest
import torch

from tests import gated_cases as G

pytestmark = pytest.mark.gpu
WORST = collections.OrderedDict()
INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def worst_error_over_bar():
    """after the module's tests: the table of profiles/gated_edges_err_over_bar.txt for whatever part of the file was run"""
    yield
    print("\nworst error / bar per kernel and quantity over the cases of tests/test_gated_edges_gpu.py that ran")
    for (kernel, nm), r in WORST.items():
        print(f"GATED_EDGES {kernel:18s} {nm:8s} {r:.3f}")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _p16(*shape):
    return torch.full(shape, G.POISON16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _p32(*shape):
    return torch.full(shape, G.POISON32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _is_poison(t):
    return bool((_bits(t) == (G.POISON16 if t.element_size() == 2 else G.POISON32)).all())


def _at(t, elems):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _judge(bars, kernel, got):
    """every asserted quantity within its bar, every share condition met; records the worst ratio"""
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
            assert s <= G.SHARE, (bars.case.name, nm, s)


@pytest.mark.parametrize("name", G.names("qknorm_rope"))
def test_qknorm_rope_edges(hip, name):
    b = G.bars(name)
    c = b.case
    M, L, H, D = c.M, c.L, c.H, c.D
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    back, upb = c.backing.cuda(), c.up_backing.cuda()
    par = [p.cuda() for p in c.params]
    cos, sin = c.cos_ext.cuda(), c.sin_ext.cuda()            # the kernel's tables are rows [0, L) of these
    nws = lib.vt_qknorm_rope_bwd_workspace_bytes() // 4

    def call():
        out, dq, grads, ws = _p16(M + G.TAIL, 3 * D), _p16(M + G.TAIL, 4 * D), _p32(4, 64), _p32(nws)
        hip.check(lib.vt_qknorm_rope_fwd(ptr(back), M, L, H, ptr(par[0]), ptr(par[1]), ptr(par[2]), ptr(par[3]), c.eps, ptr(cos), ptr(sin), ptr(out), st),
                  "vt_qknorm_rope_fwd")
        hip.check(lib.vt_qknorm_rope_bwd(ptr(back), ptr(upb), M, L, H, ptr(par[0]), ptr(par[2]), c.eps, ptr(cos), ptr(sin), ptr(dq), ptr(grads[0]),
                                         ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(ws), st), "vt_qknorm_rope_bwd")
        torch.cuda.synchronize()
        return out, dq, grads

    out, dq, grads = call()
    assert _same_bits(call(), (out, dq, grads))
    assert torch.equal(_bits(back.cpu()), _bits(c.backing)) and torch.equal(_bits(upb.cpu()), _bits(c.up_backing))
    assert _is_poison(out[M:]) and _is_poison(dq[M:]) and _is_poison(dq[:M, 3 * D:])          # rows behind the tensor, the gate's column block
    assert torch.equal(_bits(out[:M, 2 * D:]), _bits(back[:M, 2 * D:3 * D]))                   # v and its gradient: copies, bit for bit
    assert torch.equal(_bits(dq[:M, 2 * D:3 * D]), _bits(upb[:M, 2 * D:]))
    assert bool(torch.isfinite(dq[:M, :3 * D].float()).all()) and bool(torch.isfinite(grads).all())
    got = {"out": out.cpu(), "dqkvg": dq.cpu()}
    got.update({nm: grads[i].cpu() for i, nm in enumerate(G.QK_COLS)})
    _judge(b, "qknorm_rope", got)
    if c.const:                                               # a constant vector normalises to 0: the output is the rotated bf16(bias)
        for vec, kind in c.special.items():
            if kind != "const":
                continue
            row, head = vec // H, vec % H
            for i in (0, 1):
                n = G.b16(c.params[2 * i + 1].double())
                cs, sn = c.cos_ext[row % L].double(), c.sin_ext[row % L].double()
                want = torch.stack([n[0::2] * cs - n[1::2] * sn, n[0::2] * sn + n[1::2] * cs], -1).reshape(64)
                o = out[row, i * D + head * 64: i * D + head * 64 + 64].double().cpu()
                assert bool(((o - want).abs() <= 2.0 ** -8 * want.abs() + 2.0 ** -20 * (n[0::2].abs() + n[1::2].abs()).repeat_interleave(2)).all()), (vec, i)


def test_qknorm_rope_constant_vectors_give_g_to_db_and_nothing_to_dw(hip):
    """two rows at position 0 (L = 1: the rotation is the identity, g is the upstream gradient itself), every head vector constant:
    x - mean is exactly 0, so dw is exactly 0 and db is exactly the sum of the two gradients (two bf16 values add exactly in fp32)"""
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    M, L, H, D = 2, 1, 3, 192
    g = torch.Generator().manual_seed(5)
    x = torch.full((M, 4 * D), 1.5, dtype=torch.bfloat16)
    x[1] = -0.75
    up = torch.randn(M, 3 * D, generator=g).to(torch.bfloat16)
    n = torch.arange(64, dtype=torch.float32)
    par = [(1 + 0.1 * n).cuda(), (0.1 * n).cuda()]
    cos, sin = (t.cuda() for t in G.rope_tables(2))
    dq, grads, ws = _p16(M, 4 * D), _p32(4, 64), _p32(lib.vt_qknorm_rope_bwd_workspace_bytes() // 4)
    xd, upd = x.cuda(), up.cuda()
    hip.check(lib.vt_qknorm_rope_bwd(ptr(xd), ptr(upd), M, L, H, ptr(par[0]), ptr(par[0]), G.EPS_LN, ptr(cos), ptr(sin), ptr(dq), ptr(grads[0]),
                                     ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(ws), st), "vt_qknorm_rope_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dq[:, :3 * D].float()).all())
    for i in (0, 1):
        assert bool((grads[2 * i] == 0).all())
        want = up[:, i * D:(i + 1) * D].float().reshape(M * H, 64)
        assert float((grads[2 * i + 1].cpu().double() - want.double().sum(0)).abs().max()) <= 2.0 ** -22 * float(want.abs().sum(0).max())


@pytest.mark.parametrize("name", G.names("sigmoid_gate"))
def test_sigmoid_gate_edges(hip, name):
    b = G.bars(name)
    c = b.case
    M, D = c.M, c.D
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    gb, o, dog = c.gate_backing.cuda(), c.o.cuda(), c.dog.cuda()

    def call():
        og, d_o, dgb = _p16(M + G.TAIL, D), _p16(M + G.TAIL, D), _p16(M + G.TAIL, c.dgate_rs)
        if c.entry == "block":
            hip.check(lib.vt_sigmoid_gate_fwd(ptr(o), ptr(gb), M, D, ptr(og), st), "vt_sigmoid_gate_fwd")
            hip.check(lib.vt_sigmoid_gate_bwd(ptr(dog), ptr(o), ptr(gb), M, D, ptr(d_o), ptr(dgb), st), "vt_sigmoid_gate_bwd")
        else:
            hip.check(lib.vt_sigmoid_gate_cols_fwd(ptr(o), _at(gb, c.col), c.gate_rs, M, D, ptr(og), st), "vt_sigmoid_gate_cols_fwd")
            hip.check(lib.vt_sigmoid_gate_cols_bwd(ptr(dog), ptr(o), _at(gb, c.col), c.gate_rs, M, D, ptr(d_o), _at(dgb, c.dcol), c.dgate_rs, st),
                      "vt_sigmoid_gate_cols_bwd")
        torch.cuda.synchronize()
        return og, d_o, dgb

    og, d_o, dgb = call()
    assert _same_bits(call(), (og, d_o, dgb))
    for dev, host in ((gb, c.gate_backing), (o, c.o), (dog, c.dog)):
        assert torch.equal(_bits(dev.cpu()), _bits(host))
    assert _is_poison(og[M:]) and _is_poison(d_o[M:]) and _is_poison(dgb[M:])
    assert _is_poison(dgb[:M, :c.dcol]) and _is_poison(dgb[:M, c.dcol + D:])                  # the other column blocks / the row padding
    _judge(b, c.kernel, {"og": og.cpu(), "d_o": d_o.cpu(), "dgate": dgb.cpu()})
    if c.exhaustive:
        gate = c.gate_backing[:M, c.col:c.col + D].float()
        oo, ogc = c.o[:M], og[:M].cpu()
        nan, ninf, pinf = torch.isnan(gate), gate == -float("inf"), gate == float("inf")
        assert int(nan.sum()) == 254 and int(ninf.sum()) == 1 and int(pinf.sum()) == 1
        assert bool(torch.isnan(ogc.float()[nan]).all()) and bool(torch.isnan(d_o[:M].cpu().float()[nan]).all())
        assert torch.equal(_bits(ogc[ninf]), _bits((oo[ninf].float() * 0.0).to(torch.bfloat16)))   # an exact 0 * o, its sign included
        assert torch.equal(_bits(ogc[pinf]), _bits(oo[pinf]))


@pytest.mark.parametrize("name", G.names("geglu"))
def test_geglu_edges(hip, name):
    b = G.bars(name)
    c = b.case
    M, I, lda = c.M, c.I, c.lda
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    h, da = c.h.cuda(), c.da.cuda()

    def call():
        a, dh = _p16(M + G.TAIL, lda), _p16(M + G.TAIL, 2 * I)
        hip.check(lib.vt_geglu_fwd(ptr(h), M, I, ptr(a), lda, st), "vt_geglu_fwd")
        hip.check(lib.vt_geglu_bwd(ptr(da), lda, ptr(h), M, I, ptr(dh), st), "vt_geglu_bwd")
        torch.cuda.synchronize()
        return a, dh

    a, dh = call()
    assert _same_bits(call(), (a, dh))
    assert torch.equal(_bits(h.cpu()), _bits(c.h)) and torch.equal(_bits(da.cpu()), _bits(c.da))
    assert _is_poison(a[M:]) and _is_poison(dh[M:]) and _is_poison(a[:M, I:])
    _judge(b, "geglu", {"a": a.cpu(), "dh": dh.cpu()})


@pytest.mark.parametrize("name", G.names("stat_gate"))
def test_stat_gate_edges(hip, name):
    b = G.bars(name)
    c = b.case
    M, W, ld, d = c.M, c.W, c.ld, c.d
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    gb, ub = c.g_backing.cuda(), c.u_backing.cuda()
    w2, b2, z, mask_in = c.w2.cuda(), c.b2.cuda(), c.z.cuda(), c.mask_in.cuda()
    lv = hip._levels(c.levels)
    T = M + G.TAIL

    def forward():
        probs, mask, codes, idx = _p32(T), _p32(T), _p32(T, d), _p32(T).view(torch.int32)
        hip.check(lib.vt_stat_gate_forward(ptr(gb), ld, ptr(w2), ptr(b2), ptr(z) if c.has_z else None, M, W, d, lv, c.mode, 0,
                                           ptr(mask_in) if c.mode == G.FORCED else None, ptr(probs), ptr(mask), ptr(codes) if c.has_z else None,
                                           ptr(idx) if c.has_z and c.has_idx else None, st), "vt_stat_gate_forward")
        torch.cuda.synchronize()
        return probs, mask, codes, idx

    probs, mask, codes, idx = forward()
    assert _same_bits(forward(), (probs, mask, codes, idx))
    assert all(_is_poison(t[M:]) for t in (probs, mask, codes, idx))
    if not c.has_z:
        assert _is_poison(codes)
    if not (c.has_z and c.has_idx):
        assert _is_poison(idx)
    p = probs[:M]
    want_mask = (p > 0.5).float() if c.mode == G.THRESHOLD else (torch.ones_like(p) if c.mode == G.ONES else mask_in)
    assert torch.equal(mask[:M], want_mask)                                                  # exact, given the kernel's own probs
    if c.has_z:
        fc, fi = hip.fsq_forward(z * mask[:M, None], c.levels)
        assert torch.equal(_bits(codes[:M]), _bits(fc))
        if c.has_idx:
            assert torch.equal(idx[:M], fi)
    assert c.ambiguity_ok(), int(c.ambiguous_rows.sum())
    _judge(b, "stat_gate", {"probs": p.cpu()})

    pr, mk = c.p.cuda(), c.mask.cuda()                       # the backward's operands: the reference forward's probs and mask
    dcodes, dprobs, dmask = c.dcodes.cuda(), c.dprobs.cuda(), c.dmask.cuda()
    nws = lib.vt_stat_gate_workspace_bytes(W) // 4

    def backward():
        dU, dz, dw2, db2, ws = _p16(T, ld), _p32(T, d), _p32(W + 8), _p32(8), _p32(nws)
        hip.check(lib.vt_stat_gate_backward(ptr(dcodes) if c.has_z else None, ptr(dprobs) if c.has_dprobs else None, ptr(dmask) if c.has_dmask else None,
                                            ptr(z) if c.has_z else None, ptr(mk), ptr(pr), ptr(ub), ptr(gb), ld, ptr(w2), M, W, d, lv, c.ste, ptr(dU),
                                            ptr(dz) if c.has_z else None, ptr(dw2), ptr(db2), ptr(ws), st), "vt_stat_gate_backward")
        torch.cuda.synchronize()
        return dU, dz, dw2, db2

    dU, dz, dw2, db2 = backward()
    assert _same_bits(backward(), (dU, dz, dw2, db2))
    for dev, host in ((gb, c.g_backing), (ub, c.u_backing), (z, c.z), (pr, c.p), (mk, c.mask)):
        assert torch.equal(_bits(dev.cpu()), _bits(host))
    assert _is_poison(dU[M:]) and _is_poison(dU[:M, W:]) and _is_poison(dz[M:]) and _is_poison(dw2[W:]) and _is_poison(db2[1:])
    got = {"dU": dU.cpu(), "dw2": dw2[:W].cpu(), "db2": db2[:1].cpu()}
    if c.has_z:
        assert torch.equal(_bits(dz[:M]), _bits(hip.fsq_backward(z * mk[:, None], dcodes, c.levels) * mk[:, None]))
        got["dz"] = dz[:M].cpu()
    else:
        assert _is_poison(dz)
    _judge(b, "stat_gate", got)


def test_refusals_launch_nothing(hip):
    """every one of these returns VT_ERR_INVALID from the host-side checks and leaves its outputs untouched"""
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    M, W = 16, 1280
    g = torch.zeros(M + 1, W, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(4096, device="cuda")
    outs = [_p32(4096) for _ in range(6)]
    o16 = _p16(M + 1, 4 * W)
    lv6, lv17 = hip._levels([8, 8, 8, 5, 5, 5]), hip._levels([2] * 17)

    def fwd(Wk=768, ld=768, d=6, lv=lv6, mode=G.THRESHOLD, mask_in=None, z=True, codes=True, gp=None):
        return lib.vt_stat_gate_forward(gp or ptr(g), ld, ptr(f), ptr(f), ptr(f) if z else None, M, Wk, d, lv, mode, 0, mask_in, ptr(outs[0]), ptr(outs[1]),
                                        ptr(outs[2]) if codes else None, ptr(outs[3]), st)

    def bwd(Wk=768, ld=768, d=6, lv=lv6, dz=True, dcodes=True):
        return lib.vt_stat_gate_backward(ptr(f) if dcodes else None, ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), ptr(g), ptr(g), ld, ptr(f), M, Wk, d, lv, 1,
                                         ptr(o16), ptr(outs[2]) if dz else None, ptr(outs[4]), ptr(outs[5]), ptr(outs[0]), st)

    for Wk in (0, 64, 192, 1152):
        assert fwd(Wk=Wk, ld=1280) == INVALID and bwd(Wk=Wk, ld=1280) == INVALID, Wk
    assert fwd(ld=760) == INVALID and bwd(ld=760) == INVALID                               # ld < W
    assert fwd(ld=772) == INVALID and bwd(ld=772) == INVALID                               # ld % 8 != 0
    assert fwd(d=17, lv=lv17) == INVALID and bwd(d=17, lv=lv17) == INVALID
    assert fwd(mode=G.FORCED) == INVALID                                                   # FORCED without mask_in
    assert fwd(codes=False) == INVALID and bwd(dz=False) == INVALID and bwd(dcodes=False) == INVALID      # z without codes / dz / dcodes
    assert fwd(gp=_at(g, 4)) == INVALID                                                 # a misaligned g
    D = 64
    assert lib.vt_sigmoid_gate_cols_fwd(ptr(g), ptr(g), D - 8, M, D, ptr(o16), st) == INVALID                                     # gate_rs < D
    assert lib.vt_sigmoid_gate_cols_bwd(ptr(g), ptr(g), ptr(g), D - 8, M, D, ptr(o16), ptr(o16), D, st) == INVALID
    assert lib.vt_sigmoid_gate_cols_bwd(ptr(g), ptr(g), ptr(g), D, M, D, ptr(o16), ptr(o16), D - 8, st) == INVALID
    assert lib.vt_geglu_fwd(ptr(g), M, 64, ptr(o16), 56, st) == INVALID and lib.vt_geglu_bwd(ptr(g), 56, ptr(g), M, 64, ptr(o16), st) == INVALID   # lda < I
    assert lib.vt_qknorm_rope_fwd(ptr(g), M, 5, 1, ptr(f), ptr(f), ptr(f), ptr(f), 1e-5, ptr(f), ptr(f), ptr(o16), st) == INVALID    # M % L != 0
    assert lib.vt_qknorm_rope_bwd(ptr(g), ptr(g), M, 5, 1, ptr(f), ptr(f), 1e-5, ptr(f), ptr(f), ptr(o16), ptr(outs[4]), ptr(outs[4]), ptr(outs[4]),
                                  ptr(outs[4]), ptr(outs[0]), st) == INVALID
    torch.cuda.synchronize()
    assert all(_is_poison(t) for t in outs) and _is_poison(o16)
