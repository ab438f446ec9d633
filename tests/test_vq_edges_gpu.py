"""The quantizer kernels of csrc/vt_vq.hip at their edges, through the C ABI, against the oracle, references and bars of tests/vq_cases.py
(whose power tests/test_vq_cases_cpu.py proves without a kernel).  Common to every call: each output and the workspace is a view of a
larger allocation that holds a poison bit pattern, the workspace view has exactly vt_vq_workspace_bytes, and everything outside the
documented regions keeps its poison (rows behind a tensor, padding columns of the bf16 copies, both sides of the workspace); inputs are
strided views whose padding holds poison and keep their bits.

After the module's tests a fixture prints the worst error / bar of the token backward (profiles/vq_edges_err_over_bar.txt holds one run);
everything else in this file is compared bit for bit."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from oracle import vq_c
from tests import vq_cases as V

pytestmark = pytest.mark.gpu
WORST = collections.OrderedDict()
INVALID = -1
PAD = 64                     # floats of poison on both sides of the workspace view (keeps its 16-byte alignment)


@pytest.fixture(scope="module", autouse=True)
def worst_error_over_bar():
    yield
    print("\nworst error / bar of vq_bwd_tokens_kernel over the cases of tests/test_vq_edges_gpu.py that ran")
    for (l2n, nm), r in WORST.items():
        print(f"VQ_EDGES bwd_tokens l2_normalized={l2n} {nm:7s} {r:.3f}")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _p16(*shape):
    return torch.full(shape, V.POISON16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _p32(*shape):
    return torch.full(shape, V.POISON32, dtype=torch.int32, device="cuda").view(torch.float32)


def _p64(*shape):
    return torch.full(shape, V.POISON64, dtype=torch.int64, device="cuda")


def _is_poison(t):
    t = t.contiguous()
    if t.dtype == torch.int64:
        return bool((t == V.POISON64).all())
    return bool((t.view(torch.int16) == V.POISON16).all()) if t.element_size() == 2 else bool((t.view(torch.int32) == V.POISON32).all())


def _at(t, elems):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return t.cpu().numpy()


class Ws:
    """a workspace view of exactly vt_vq_workspace_bytes inside a poisoned allocation"""

    def __init__(self, hip, N, K, d):
        nbytes = hip.lib().vt_vq_workspace_bytes(N, K, d)
        assert nbytes % 4 == 0 and nbytes // 4 == V.workspace_floats(N, K, d)[0]
        self.n = nbytes // 4
        self.back = _p32(self.n + 2 * PAD)
        self.ptr = _at(self.back, PAD)

    def margins_poison(self):
        return _is_poison(self.back[:PAD]) and _is_poison(self.back[PAD + self.n:])

    def untouched(self):
        return _is_poison(self.back)


def _forward(hip, N, K, d, mode, l2n, W, zback, ldp=64, beta=V.BETA, cbw=V.CBW):
    """vt_vq_forward into poisoned backing buffers; returns the dict of views hip.vq_backward takes, after the containment checks"""
    lib, ptr = hip.lib(), hip.ptr
    T = V.TAIL
    b = {"E": _p32(K + T, d), "wnorm": _p32(K + T), "zn": _p32(N + T, d), "znorm": _p32(N + T), "idx": _p64(N + T), "rz": _p32(N + T, d),
         "rz_pad": _p16(N + T, ldp), "losses": _p32(4 + T)}
    ws = Ws(hip, N, K, d)
    hip.check(lib.vt_vq_forward(ptr(zback), zback.stride(0), ptr(W), N, K, d, 0 if mode == "L" else 1, l2n, V.INV_TAU, beta, cbw, 0, ptr(b["E"]),
                                ptr(b["wnorm"]), ptr(b["zn"]), ptr(b["znorm"]), ptr(b["idx"]), ptr(b["rz"]), ptr(b["rz_pad"]), ldp, ptr(b["losses"]),
                                ws.ptr, hip.stream()), "vt_vq_forward")
    torch.cuda.synchronize()
    assert ws.margins_poison()
    for nm, rows in (("E", K), ("wnorm", K), ("zn", N), ("znorm", N), ("idx", N), ("rz", N), ("rz_pad", N), ("losses", 4)):
        assert _is_poison(b[nm][rows:]), nm                                                    # rows behind the tensor
    assert _is_poison(b["rz_pad"][:N, d:])                                                     # padding columns of the bf16 copy
    o = {nm: t[:rows] for (nm, t), rows in zip(b.items(), (K, K, N, N, N, N, N, 4))}
    assert not _is_poison(o["losses"]) and bool(torch.isfinite(o["losses"]).all())
    return o


@pytest.mark.parametrize("name", V.names())
def test_vq_forward_edges(hip, name):
    c, r = V.CASES[name], V.reference(name)
    N, K, d = c.N, c.K, c.d
    Wn, backing = V.inputs(name)
    W, zback = _dev(Wn), _dev(backing)
    o = _forward(hip, N, K, d, c.mode, c.l2n, W, zback)
    assert torch.equal(zback.cpu().view(torch.int32), torch.from_numpy(np.array(backing)).view(torch.int32))      # inputs keep their bits
    sel = r.sel
    idx = _np(o["idx"])
    assert np.array_equal(_np(o["zn"]), r.zn) and np.array_equal(_np(o["znorm"]), r.znorm)    # every row: the normalisation is cheap
    assert np.array_equal(_np(o["E"]), r.E) and np.array_equal(_np(o["wnorm"]), r.wnorm)
    bad = np.nonzero(idx[sel] != r.idx)[0]
    assert not len(bad), (name, [(int(sel[i]), int(idx[sel[i]]), int(r.idx[i])) for i in bad[:8]])
    rz = _np(o["rz"])
    assert np.array_equal(rz[sel], r.rz)
    assert torch.equal(o["rz_pad"][:, :d].cpu()[torch.from_numpy(sel)], torch.from_numpy(r.rz).to(torch.bfloat16))
    if not c.subset:
        mse = r.mse
        np.testing.assert_allclose(_np(o["losses"])[:3], [V.BETA * mse + V.CBW * mse, mse, mse], rtol=1e-5)
    else:
        # every token, cheaply: the index is in range, rz / rz_pad are the gather of THAT index bit for bit, and its float64 score
        # is within the fp32 bound of the row's best (tests/vq_cases.py: score_gap_and_bound)
        assert idx.min() >= 0 and idx.max() < K
        assert np.array_equal(rz, r.zn + (r.E[idx] - r.zn))
        assert torch.equal(o["rz_pad"][:, :d].cpu(), torch.from_numpy(rz).to(torch.bfloat16))
        gap, bound = V.score_gap_and_bound(o["zn"], o["E"], o["idx"], c.mode)
        worst = int((gap - bound).argmax())
        assert bool((gap <= bound).all()), (name, worst, float(gap[worst]), float(bound[worst]))
        mse = float(((o["E"][o["idx"]].double() - o["zn"].double()) ** 2).mean())
        np.testing.assert_allclose(_np(o["losses"])[:3], [V.BETA * mse + V.CBW * mse, mse, mse], rtol=1e-5)


def _backward(hip, o, N, K, d, l2n, gback, gscal, dz_in=True, dz_pad=True, need_dW=True, ldp=64):
    lib, ptr = hip.lib(), hip.ptr
    T = V.TAIL
    dz, dzp, dW = _p32(N + T, d), _p16(N + T, ldp), _p32(K + T, d)
    ws = Ws(hip, N, K, d)
    hip.check(lib.vt_vq_backward(ptr(gback), gback.stride(0) if gback is not None else 0, ptr(gscal), V.BETA, V.CBW, ptr(o["zn"]), ptr(o["znorm"]),
                                 ptr(o["E"]), ptr(o["wnorm"]), ptr(o["idx"]), N, K, d, l2n, ptr(dz) if dz_in else None, ptr(dzp) if dz_pad else None,
                                 ldp, ptr(dW) if need_dW else None, ws.ptr, hip.stream()), "vt_vq_backward")
    torch.cuda.synchronize()
    assert ws.margins_poison()
    assert _is_poison(dz[N:]) and _is_poison(dzp[N:]) and _is_poison(dzp[:N, d:]) and _is_poison(dW[K:])
    if not dz_in:
        assert _is_poison(dz)
    if not dz_pad:
        assert _is_poison(dzp)
    if not need_dW:
        assert _is_poison(dW) and ws.untouched()                                               # frozen codebook: nothing of the gradient runs
    return dz[:N], dzp[:N, :d], dW[:K]


@pytest.mark.parametrize("N,d,l2n,variant", V.bwd_cases())
def test_vq_token_backward_edges(hip, N, d, l2n, variant):
    K = V.BWD_K
    Wn, zn_, gn = V.bwd_inputs(N, K, d, l2n)
    zb = np.full((N, d + 8), V.PF, dtype=np.float32)
    zb[:, :d] = zn_
    W, zback, gback = _dev(Wn), _dev(zb), _dev(gn)
    o = _forward(hip, N, K, d, "L", l2n, W, zback)
    gscal = torch.tensor(V.GSCAL, dtype=torch.float32).cuda()
    g = None if variant == "no_g_rz" else gback
    dz, dzp, dW = _backward(hip, o, N, K, d, l2n, g, gscal, dz_in=variant != "dz_pad", dz_pad=variant != "dz_in")
    assert torch.equal(gback.cpu().view(torch.int32), torch.from_numpy(np.array(gn)).view(torch.int32))
    want, dW64, bar = V.bwd_reference(zn_, Wn, _np(o["idx"]), None if g is None else gn[:, :d], V.GSCAL, l2n)
    if variant != "dz_pad":
        r = float(((dz.cpu().double() - want).abs() / bar).max())
        WORST[(l2n, "dz_in")] = max(WORST.get((l2n, "dz_in"), 0.0), r)
        print(f"N={N} d={d} l2n={l2n} {variant}: dz_in error / bar = {r:.3f}")
        assert r <= 1.0, r
    if variant != "dz_in":
        r = float(((dzp.cpu().double() - want).abs() / V.bwd_bar_bf16(want, bar)).max())
        WORST[(l2n, "dz_pad")] = max(WORST.get((l2n, "dz_pad"), 0.0), r)
        print(f"N={N} d={d} l2n={l2n} {variant}: dz_pad error / bar = {r:.3f}")
        assert r <= 1.0, r
    if variant == "both":
        assert torch.equal(dzp, dz.to(torch.bfloat16))                                          # the copy is the rounding of the fp32 output
    # the codebook gradient of the same call, bit for bit (non-default codebook_w, all three gscal entries)
    ref = vq_c.codebook_grad(_np(o["zn"]), _np(o["E"]), _np(o["wnorm"]), _np(o["idx"]), V.s_b_fp32(V.GSCAL, N, d), normalize=bool(l2n))
    assert np.array_equal(_np(dW), ref)


@pytest.mark.parametrize("N,K,d,l2n,collapse", V.cbgrad_cases())
def test_vq_codebook_gradient_edges(hip, N, K, d, l2n, collapse):
    Wn, zn_, _ = V.bwd_inputs(N, K, d, l2n, collapse)
    W, zback = _dev(Wn), _dev(zn_)
    o = _forward(hip, N, K, d, "L", l2n, W, zback)
    idx = _np(o["idx"])
    if collapse:
        assert (idx[:collapse] == min(7, K - 1)).all() and collapse == V.cb_plan(N)["slab_len"]   # one code receives every token of slab 0
    if N < K:
        assert np.bincount(idx, minlength=K).min() == 0                                        # and some code receives none
    gscal = torch.tensor(V.GSCAL, dtype=torch.float32).cuda()
    dz, _, dW = _backward(hip, o, N, K, d, l2n, None, gscal, dz_pad=False)
    ref = vq_c.codebook_grad(_np(o["zn"]), _np(o["E"]), _np(o["wnorm"]), idx, V.s_b_fp32(V.GSCAL, N, d), normalize=bool(l2n))
    got = _np(dW)
    bad = np.argwhere(got != ref)
    assert not len(bad), (len(bad), bad[:4].tolist())
    if N in (63, 16385):
        _backward(hip, o, N, K, d, l2n, None, gscal, dz_pad=False, need_dW=False)


@pytest.mark.parametrize("K,d,l2n", [(300, 24, 1), (1, 8, 1), (300, 32, 0)])
def test_vq_prep_codebook_equals_the_forward(hip, K, d, l2n):
    lib, ptr = hip.lib(), hip.ptr
    Wn, zn_, _ = V.bwd_inputs(33, K, d, l2n)
    W = _dev(Wn)
    o = _forward(hip, 33, K, d, "L", l2n, W, _dev(zn_))
    E, wn = _p32(K + V.TAIL, d), _p32(K + V.TAIL)
    ws = Ws(hip, 1, K, d)
    hip.check(lib.vt_vq_prep_codebook(ptr(W), K, d, l2n, ptr(E), ptr(wn), ws.ptr, hip.stream()), "vt_vq_prep_codebook")
    torch.cuda.synchronize()
    assert ws.margins_poison() and _is_poison(E[K:]) and _is_poison(wn[K:])
    assert torch.equal(E[:K].view(torch.int32), o["E"].contiguous().view(torch.int32)) and torch.equal(wn[:K].view(torch.int32), o["wnorm"].view(torch.int32))


@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("which", ["out", "out_pad", "both"])
def test_vq_gather_clamps_and_stays_inside(hip, N, which):
    lib, ptr = hip.lib(), hip.ptr
    K, d, ldp = 300, 24, 64
    E = _dev(vq_c.normalize_rows(V.bwd_inputs(33, K, d, 1)[0])[0])
    idxn = (np.arange(N, dtype=np.int64) * 7919) % K
    for pos, v in zip((0, 5, 100, 200, 256), (-1, K, 2 ** 31, K - 1, -2 ** 40)):               # below, one past, past int32, the last code, far below
        if pos < N:
            idxn[pos] = v
    idx = torch.from_numpy(idxn).cuda()
    out, pad = _p32(N + V.TAIL, d), _p16(N + V.TAIL, ldp)
    hip.check(lib.vt_vq_gather(ptr(E), ptr(idx), N, K, d, ptr(out) if which != "out_pad" else None, ptr(pad) if which != "out" else None, ldp,
                               hip.stream()), "vt_vq_gather")
    torch.cuda.synchronize()
    want = E[idx.clamp(0, K - 1)]
    assert _is_poison(out[N:]) and _is_poison(pad[N:]) and _is_poison(pad[:N, d:])
    if which != "out_pad":
        assert torch.equal(out[:N].view(torch.int32), want.view(torch.int32))
    else:
        assert _is_poison(out)
    if which != "out":
        assert torch.equal(pad[:N, :d], want.to(torch.bfloat16))
    else:
        assert _is_poison(pad)
    assert torch.equal(idx.cpu(), torch.from_numpy(idxn))


def test_refusals_launch_nothing(hip):
    """every one of these returns VT_ERR_INVALID from the host-side checks, sets vt_last_error and leaves every output untouched"""
    lib, ptr, st = hip.lib(), hip.ptr, hip.stream()
    N, K, d = 16, 8, 8
    f = torch.zeros(4096, device="cuda")
    i64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    outs = [_p32(4096) for _ in range(8)]
    o16, o64 = _p16(4096), _p64(64)

    def refused(rc, what):
        assert rc == INVALID, what
        buf = ctypes.create_string_buffer(512)
        lib.vt_last_error(buf, 512)
        assert buf.value.decode().startswith(what), (what, buf.value)

    def fwd(N=N, K=K, d=d, mode=0, l2n=1, ldp=64, z=True, ws=True):
        return lib.vt_vq_forward(ptr(f) if z else None, 32, ptr(f), N, K, d, mode, l2n, 1.0, 0.25, 1.0, 0, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                 ptr(outs[3]), ptr(o64), ptr(outs[4]), ptr(o16), ldp, ptr(outs[5]), ptr(outs[6]) if ws else None, st)

    def bwd(N=N, K=K, d=d, ldp=64, ldg=32, idx=True, dz=True, dzp=True):
        return lib.vt_vq_backward(ptr(f), ldg, ptr(f), 0.25, 1.0, ptr(f), ptr(f), ptr(f), ptr(f), ptr(i64) if idx else None, N, K, d, 1,
                                  ptr(outs[0]) if dz else None, ptr(o16) if dzp else None, ldp, ptr(outs[1]), ptr(outs[6]), st)

    refused(fwd(d=12), "vt_vq_forward")
    refused(bwd(d=12), "vt_vq_backward")
    refused(fwd(K=0), "vt_vq_forward")
    refused(bwd(K=0), "vt_vq_backward")
    refused(fwd(N=0), "vt_vq_forward")
    refused(bwd(N=0), "vt_vq_backward")
    refused(fwd(mode=3), "vt_vq_forward")
    refused(fwd(mode=-1), "vt_vq_forward")
    refused(fwd(mode=1, l2n=0), "vt_vq_forward")
    refused(fwd(mode=2, l2n=0), "vt_vq_forward")
    refused(fwd(ldp=d - 1), "vt_vq_forward")
    refused(bwd(ldp=d - 1), "vt_vq_backward")
    refused(bwd(ldg=d - 1), "vt_vq_backward")
    refused(fwd(z=False), "vt_vq_forward")
    refused(fwd(ws=False), "vt_vq_forward")
    refused(bwd(idx=False), "vt_vq_backward")
    refused(bwd(dz=False, dzp=False), "vt_vq_backward")
    refused(lib.vt_vq_gather(ptr(f), ptr(i64), N, K, d, None, None, 64, st), "vt_vq_gather")
    refused(lib.vt_vq_gather(ptr(f), ptr(i64), N, K, d, ptr(outs[0]), ptr(o16), d - 1, st), "vt_vq_gather")
    refused(lib.vt_vq_gather(ptr(f), ptr(i64), 0, K, d, ptr(outs[0]), None, 64, st), "vt_vq_gather")
    refused(lib.vt_vq_gather(ptr(f), None, N, K, d, ptr(outs[0]), None, 64, st), "vt_vq_gather")
    refused(lib.vt_vq_prep_codebook(ptr(f), 0, d, 1, ptr(outs[0]), ptr(outs[1]), ptr(outs[6]), st), "vt_vq_prep_codebook")
    refused(lib.vt_vq_prep_codebook(None, K, d, 1, ptr(outs[0]), ptr(outs[1]), ptr(outs[6]), st), "vt_vq_prep_codebook")
    torch.cuda.synchronize()
    assert all(_is_poison(t) for t in outs) and _is_poison(o16) and _is_poison(o64)
