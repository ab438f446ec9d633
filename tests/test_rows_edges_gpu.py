"""The row kernels of csrc/vt_layernorm.hip and csrc/vt_rows.hip at the sizes where they take another path: the grid-stride loops (LayerNorm
forward rows > 8192, backward rows > 2048), the 32-lane partial reduction (>= 128 slabs, i.e. rows >= 509), a last workgroup with idle
waves, every supported width, row maps, every optional operand absent in turn, the 64-slab cap and the 4 x 4-row unrolled loop of
vt_colsum, element counts that cross a 256-thread block.  References are float64 torch on the same inputs.

Bounds.  fp32 elementwise results: 64 eps of the largest reference magnitude (a handful of fp32 operations on O(max) operands).  bf16
copies: one bf16 step, 2^-8 relative, on top of that.  Column sums (dgamma, dbeta, dxsum, vt_colsum, vt_sum_slabs): `_sum_bound` --
8 x the spread of sequential float32 column sums of the fp32-rounded terms over row permutations against float64, plus what the terms
themselves may be off (sqrt(rows) x their elementwise bound), capped at a quarter of what dropping the last row would change."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
DIMS = (128, 256, 384, 512, 768, 1024)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sum_bound(terms, term_tol=0.0):
    """terms float64 [rows, width] -> scalar bound on max_c |sum - reference| (see the module docstring)"""
    rows = terms.shape[0]
    ref = terms.sum(0)
    t32 = terms.float()
    spread = 0.0
    for p in range(3):
        order = torch.arange(rows) if p == 0 else torch.randperm(rows, generator=_g(p))
        spread = max(spread, float((t32[order].cumsum(0)[-1].double() - ref).abs().max()))
    bound = 8 * spread + math.sqrt(rows) * term_tol
    return min(bound, 0.25 * float(terms[-1].abs().max())) if rows > 1 else bound


def _bf16_close(got, want, atol):
    """got = bf16 of a value within atol of want"""
    return bool(((got.double() - want).abs() <= 2.0 ** -8 * want.abs() + atol).all())


def _phys(rows, rmap):
    """physical row of every logical row under the map (grp, stride, off), and the physical row count"""
    r = torch.arange(rows)
    if rmap is None:
        return r, rows
    grp, stride, off = rmap
    return (r // grp) * stride + off + r % grp, ((rows + grp - 1) // grp) * stride


def _ln_inputs(rows, dim, rmap, seed):
    g = _g(seed)
    pr, nphys = _phys(rows, rmap)
    x = torch.randn(nphys, dim, generator=g) * 2 + 0.3
    gamma = torch.rand(dim, generator=g) + 0.5
    beta = torch.randn(dim, generator=g) * 0.1
    dy = torch.randn(rows, dim, generator=g).to(torch.bfloat16)
    dres = torch.randn(nphys, dim, generator=g)
    return pr, nphys, x, gamma, beta, dy, dres


@pytest.mark.parametrize("mapped", [False, True], ids=["dense", "rowmap"])
@pytest.mark.parametrize("rows", [1, 3, 5, 509, 2049, 8197])
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_fwd_edges(hip, dim, rows, mapped):
    rmap = (7, 11, 3) if mapped else None
    pr, nphys, x, gamma, beta, _, _ = _ln_inputs(rows, dim, rmap, 1000 + rows + dim)
    xd = x.cuda()
    m = hip.RowMap(*rmap) if mapped else None
    y, mean, rstd = hip.layernorm_fwd(xd, gamma.cuda(), beta.cuda(), 1e-5, rows=rows, xmap=m)
    y2, mean2, rstd2 = hip.layernorm_fwd(xd, gamma.cuda(), beta.cuda(), 1e-5, rows=rows, xmap=m)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    xs = x[pr].double()
    mu = xs.mean(-1)
    rs = 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)
    want = (xs - mu[:, None]) * rs[:, None] * gamma.double() + beta.double()
    xmax = float(xs.abs().max())
    assert float((mean.double().cpu() - mu).abs().max()) <= 16 * EPS * xmax
    assert float((rstd.double().cpu() / rs - 1).abs().max()) <= 64 * EPS
    assert _bf16_close(y.cpu(), want, 64 * EPS * float(want.abs().max()))
    assert torch.equal(xd.cpu(), x)


# every width with every operand; each optional operand absent in turn at two widths (8-byte and 16-byte lanes): it does not depend on the width
BWD_CASES = [(d, "none") for d in DIMS] + [(d, a) for d in (128, 768) for a in ("dres", "dxsum", "dxb")]


@pytest.mark.parametrize("mapped", [False, True], ids=["dense", "rowmap"])
@pytest.mark.parametrize("rows", [1, 3, 5, 509, 2049])
@pytest.mark.parametrize("dim,absent", BWD_CASES)
def test_layernorm_bwd_edges(hip, dim, absent, rows, mapped):
    """dgamma / dbeta / dxsum bound: `_sum_bound` of the float64 terms dy * xh, dy and dres + dx (module docstring).  At rows = 2049, dim = 768
    that is 4.2e-3, 6.1e-5 and 2.0e-3 against sums of magnitude 130 .. 160 (the cap, a quarter of the last row's largest term, is 1.8); at
    rows = 5, dim = 1024: 1.2e-4, 0 (five bf16 values add exactly in fp32, in any order) and 8.0e-5."""
    rmap = (7, 11, 3) if mapped else None
    pr, nphys, x, gamma, beta, dy, dres = _ln_inputs(rows, dim, rmap, 2000 + rows + dim)
    m = hip.RowMap(*rmap) if mapped else None
    xs = x[pr].double()
    mu = xs.mean(-1)
    rs = 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)
    mean, rstd = mu.float().cuda(), rs.float().cuda()       # the forward's outputs, as exact as fp32 holds them
    xh = (xs - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
    a = dy.double() * gamma.double()
    dxr = rstd.double().cpu()[:, None] * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    want = dxr + (dres[pr].double() if absent != "dres" else 0.0)
    sent = 768.0
    dx = torch.full((nphys, dim), sent, device="cuda")
    dxb = torch.full((nphys, dim), sent, device="cuda", dtype=torch.bfloat16) if absent != "dxb" else None
    args = dict(dres=dres.cuda() if absent != "dres" else None, xmap=m, want_dxsum=absent != "dxsum", want_dxb=absent != "dxb")
    out = hip.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda(), mean, rstd, dx=dx, dxb=dxb, **args)
    dx2 = torch.full((nphys, dim), sent, device="cuda")
    dxb2 = torch.full((nphys, dim), sent, device="cuda", dtype=torch.bfloat16) if absent != "dxb" else None
    out2 = hip.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda(), mean, rstd, dx=dx2, dxb=dxb2, **args)
    torch.cuda.synchronize()
    for t, t2 in zip(out, out2):
        assert (t is None and t2 is None) or torch.equal(t, t2)                  # a second call gives identical bits
    _, _, dg, db, ds = out
    tol = 64 * EPS * float(want.abs().max())
    assert float((dx[pr].double().cpu() - want).abs().max()) <= tol
    keep = torch.ones(nphys, dtype=torch.bool)
    keep[pr] = False
    assert torch.all(dx.cpu()[keep] == sent)                                      # unmapped rows: untouched
    if dxb is not None:
        assert _bf16_close(dxb[pr].cpu(), want, tol)
        assert torch.all(dxb.cpu()[keep].float() == sent)
    tg = dy.double() * xh
    assert float((dg.double().cpu() - tg.sum(0)).abs().max()) <= _sum_bound(tg, 64 * EPS * float(tg.abs().max()))
    assert float((db.double().cpu() - dy.double().sum(0)).abs().max()) <= _sum_bound(dy.double())
    if absent == "dxsum":
        assert ds is None
    else:
        assert float((ds.double().cpu() - want.sum(0)).abs().max()) <= _sum_bound(want, tol)


@pytest.mark.parametrize("width", [8, 504, 512, 520, 3072])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_colsum_edges(hip, dtype, width):
    """rows around the 4 x 4-row unrolled loop (1, 4, 13, 16, 17), one slab and its edge (63, 64, 65) and past the 64-slab cap (4097,
    5000); a source wider than the summed width (ld > width, loud columns behind) and a row map"""
    ld = width + 16
    for rows in (1, 4, 13, 16, 17, 63, 64, 65, 4097, 5000):
        src = torch.randn(rows, ld, generator=_g(rows + width)).to(dtype)
        src[:, width:] = 1e4
        got = hip.colsum(src.cuda()[:, :width])
        torch.cuda.synchronize()
        terms = src[:, :width].double()
        err = float((got.double().cpu() - terms.sum(0)).abs().max())
        assert err <= _sum_bound(terms), (rows, err)
    grp, stride, off = 5, 9, 2
    for rows in (13, 4097):
        pr, nphys = _phys(rows, (grp, stride, off))
        src = torch.full((nphys, width), 1e4).to(dtype)
        src[pr] = torch.randn(rows, width, generator=_g(7 + rows + width)).to(dtype)
        got = hip.colsum(src.cuda(), rows=rows, rmap=hip.RowMap(grp, stride, off))
        torch.cuda.synchronize()
        terms = src[pr].double()
        assert float((got.double().cpu() - terms.sum(0)).abs().max()) <= _sum_bound(terms), rows


@pytest.mark.parametrize("n,dim", [(1, 4), (100, 12), (64, 16), (65, 16), (50, 768)])
def test_batch_sum_cast_assemble_edges(hip, n, dim):
    """n * dim / 4 threads: below, across and exactly on a 256-thread block; every optional operand absent in turn"""
    batch, seq, off = 3, n + 5, 2
    g = _g(n * dim)
    f = torch.randn(batch * seq, dim, generator=g)
    pr, _ = _phys(batch * n, (n, seq, off))
    for m, rows_of in ((None, torch.arange(batch * n)), (hip.RowMap(n, seq, off), pr)):
        sel = f[rows_of].reshape(batch, n, dim)
        got = hip.batch_sum(f.cuda(), batch, n, rmap=m)
        want = sel[0].clone()
        for b in range(1, batch):
            want += sel[b]                                                        # the kernel's order, in fp32: the same bits
        c = hip.cast_rows(f.cuda(), rows=batch * n, rmap=m)
        cp = hip.cast_rows(f.cuda(), rows=batch * n, rmap=m, ldd=dim + 8)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want)
        assert float((got.double().cpu() - sel.double().sum(0)).abs().max()) <= 4 * EPS * float(sel.abs().sum(0).max())
        assert torch.equal(c.cpu(), sel.reshape(-1, dim).to(torch.bfloat16))
        assert torch.equal(cp.cpu()[:, :dim], c.cpu()) and torch.all(cp.cpu()[:, dim:] == 0)   # pad columns: never written
    src = torch.randn(batch * n, dim, generator=g)
    tab = torch.randn(n, dim, generator=g)
    vec = torch.randn(dim, generator=g)
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        dst = torch.full((batch * seq, dim), 768.0, device="cuda")
        hip.assemble_rows(dst, seq, off, batch, n, src=src.cuda() if use[0] else None, table=tab.cuda() if use[1] else None,
                          vec=vec.cuda() if use[2] else None)
        torch.cuda.synchronize()
        want = torch.full((batch, seq, dim), 768.0)
        acc = torch.zeros(batch, n, dim)
        if use[0]:
            acc = acc + src.reshape(batch, n, dim)
        if use[1]:
            acc = acc + tab
        if use[2]:
            acc = acc + vec
        want[:, off:off + n] = acc
        assert torch.equal(dst.cpu(), want.reshape(-1, dim)), use


@pytest.mark.parametrize("nslab", [1, 7, 8, 9, 127, 128, 129])
def test_sum_slabs_edges(hip, nslab):
    """both lane counts of the partial reduction (8 below 128 slabs, 32 from there), a width that is no multiple of the 32-column
    workgroup, slabs further apart than they are wide with loud values between them"""
    width, stride = 100, 136
    buf = torch.full((nslab * stride,), 1e4)
    slabs = torch.randn(nslab, width, generator=_g(nslab))
    buf.reshape(nslab, stride)[:, :width] = slabs
    got = hip.sum_slabs(buf.cuda(), nslab, width, slab_stride=stride)
    dense = hip.sum_slabs(slabs.cuda(), nslab, width)
    torch.cuda.synchronize()
    assert torch.equal(got, dense)
    assert float((got.double().cpu() - slabs.double().sum(0)).abs().max()) <= _sum_bound(slabs.double())


@pytest.mark.parametrize("which", ["fp32", "bf16", "both"])
@pytest.mark.parametrize("rows,dim", [(1, 4), (20, 52), (64, 16), (40, 768)])
def test_zero_rows_edges(hip, rows, dim, which):
    grp, stride, off = 5, 9, 3
    pr, nphys = _phys(rows, (grp, stride, off))
    a = torch.full((nphys, dim), 768.0, device="cuda") if which != "bf16" else None
    b = torch.full((nphys, dim), 768.0, device="cuda", dtype=torch.bfloat16) if which != "fp32" else None
    hip.zero_rows(a, b, rows=rows, rmap=hip.RowMap(grp, stride, off))
    torch.cuda.synchronize()
    want = torch.full((nphys, dim), 768.0)
    want[pr] = 0.0
    for t in (a, b):
        if t is not None:
            assert torch.equal(t.float().cpu(), want)
    d = torch.full((rows, dim), 768.0, device="cuda")
    hip.zero_rows(d)                                                              # no map: every row
    assert torch.all(d == 0)


@pytest.mark.parametrize("rows,dim", [(1, 4), (3, 12), (257, 4), (4099, 1024)])    # the last: more float4s than the 4096 x 256 threads of the capped grid
def test_scale_rows_edges(hip, rows, dim):
    src = torch.randn(rows, dim, generator=_g(rows))
    scale = 1.0 / math.sqrt(3.0)
    want = src * torch.tensor(scale, dtype=torch.float32)
    s = src.cuda()
    f = torch.empty_like(s)
    hb = torch.empty(rows, dim, device="cuda", dtype=torch.bfloat16)
    hip.scale_rows(s, scale, dst=f, dstb=hb)
    f_only = torch.empty_like(s)
    hip.scale_rows(s, scale, dst=f_only)
    b_only = torch.empty_like(hb)
    hip.scale_rows(s, scale, dstb=b_only)
    assert torch.equal(s.cpu(), src)
    hip.scale_rows(s, scale, dst=s)                                               # in place
    torch.cuda.synchronize()
    for t in (f, f_only, s):
        assert torch.equal(t.cpu(), want)
    for t in (hb, b_only):
        assert torch.equal(t.cpu(), want.to(torch.bfloat16))
