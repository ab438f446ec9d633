"""vt_attention_cross_fwd / _bwd and the row passes of model_design's CrossAttention layer on the GPU.

The attention kernels are held to the bars of tests/cross_attention_cases.py (derived from float64 references alone; the CPU test
proves their power), in two operand layouts per case that must agree bit for bit:
  wide    q = columns 0..D of a [B Lq, 2D] buffer, k and v = the two halves of one [B Lk, 2D] buffer, dq into columns 0..D of a
          [B Lq, 2D] buffer and dk / dv into the halves of a [B Lk, 2D] buffer
  own_k   q and k from dense [rows, D] buffers of their own, v = columns D..2D of a [B Lk, 2D] buffer, dq dense, dk into columns
          D..2D of a [B Lk, 3D] buffer, dv into columns 0..D of a [B Lk, 2D] buffer
Every column outside an operand holds a loud value, every column outside a gradient a sentinel that must come back bit for bit, and
poison rows sit behind every operand.  Each case prints `BAR <case> <quantity> <error> <tolerance> <error / tolerance>`.
Then: packed-qkv operands reproduce vt_attention_fwd / _bwd bit for bit, a second backward reproduces every bit, the refusals, and
vt_head_rmsnorm_*, vt_sigmoid_gate_cols_*, vt_rmsnorm_any_* against fp32 math and against the entry points they generalise."""
import ctypes

import pytest
import torch

from oracle import inputs as gen
from tests import attention_cases as A
from tests import cross_attention_cases as X

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
LOUD = 64.0


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rb(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _heads(t, B, L, H):
    return t.reshape(B, L, H, 64).permute(0, 2, 1, 3)


def _wide(rows, cols, fill):
    return torch.full((rows, cols), fill, device="cuda", dtype=torch.bfloat16)


def _run(hip, c, layout):
    """-> (results, buffers to compare against their snapshots afterwards)"""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    D = 64 * H
    Mq, Mk, P = B * Lq, B * Lk, A.POISON_ROWS
    qb, kb, vb, dOb = c.q_backing.cuda(), c.k_backing.cuda(), c.v_backing.cuda(), c.dO_backing.cuda()
    if layout == "wide":
        qbuf = _wide(Mq + P, 2 * D, LOUD)
        qbuf[:, :D] = qb
        kvbuf = torch.cat([kb, vb], 1).contiguous()
        q, k, v = qbuf[:Mq, :D], kvbuf[:Mk, :D], kvbuf[:Mk, D:]
        dqbuf, dkvbuf = _wide(Mq + P, 2 * D, SENTINEL), _wide(Mk + P, 2 * D, SENTINEL)
        dq, dk, dv = dqbuf[:Mq, :D], dkvbuf[:Mk, :D], dkvbuf[:Mk, D:]
        ins, outs = [qbuf, kvbuf, dOb], [(dqbuf, [(slice(0, Mq), slice(0, D))]), (dkvbuf, [(slice(0, Mk), slice(0, 2 * D))])]
    else:
        vbuf = _wide(Mk + P, 2 * D, LOUD)
        vbuf[:, D:] = vb
        q, k, v = qb[:Mq], kb[:Mk], vbuf[:Mk, D:]
        dqbuf, dkbuf, dvbuf = _wide(Mq + P, D, SENTINEL), _wide(Mk + P, 3 * D, SENTINEL), _wide(Mk + P, 2 * D, SENTINEL)
        dq, dk, dv = dqbuf[:Mq], dkbuf[:Mk, D:2 * D], dvbuf[:Mk, :D]
        ins = [qb, kb, vbuf, dOb]
        outs = [(dqbuf, [(slice(0, Mq), slice(0, D))]), (dkbuf, [(slice(0, Mk), slice(D, 2 * D))]), (dvbuf, [(slice(0, Mk), slice(0, D))])]
    snap = [t.clone() for t in ins]
    dO = dOb[:Mq]
    o, lse2 = hip.attention_cross_fwd(q, k, v, B, Lq, Lk, H)
    hip.attention_cross_bwd(q, k, v, o, dO, lse2, B, Lq, Lk, H, dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    for t, s in zip(ins, snap):                                              # the operands are read-only
        assert torch.equal(t, s)
    for buf, written in outs:                                                # nothing outside the gradient's own rows and columns was touched
        keep = torch.ones_like(buf, dtype=torch.bool)
        for r, cc in written:
            keep[r, cc] = False
        assert bool((buf[keep] == SENTINEL).all())
    return {"lse2": lse2, "o": o, "dq": dq.contiguous(), "dk": dk.contiguous(), "dv": dv.contiguous()}


@pytest.mark.parametrize("key", X.case_keys(), ids=X.key_id)
def test_cross_attention_case(hip, key):
    bars = X.bars(*key)
    c, ref = bars.case, bars.ref
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    r = _run(hip, c, "wide")
    got = {"lse2": r["lse2"], "o": _heads(r["o"], B, Lq, H), "dq": _heads(r["dq"], B, Lq, H), "dk": _heads(r["dk"], B, Lk, H),
           "dv": _heads(r["dv"], B, Lk, H)}
    failures = []
    for n, t in got.items():
        t = t.double().cpu()
        assert torch.isfinite(t).all(), n
        err = float(A.row_err(n, t, ref.base[n]).max())
        if bars.tol[n] is None:                   # named in cross_attention_cases.NOT_ASSERTED: no bar, the figure is printed all the same
            print(f"BAR {X.key_id(key)} {n} {err:.3e} unasserted -")
            continue
        print(f"BAR {X.key_id(key)} {n} {err:.3e} {bars.tol[n]:.3e} {err / bars.tol[n]:.3f}")
        if not err <= bars.tol[n]:
            failures.append((n, err, bars.tol[n]))
    assert not failures, failures
    # what the formula allows whatever the data: lse2 within log2(Lk) of the row maximum, o a convex combination of the V rows (poison would leave both)
    g = {n: t.double().cpu() for n, t in got.items()}
    top = ref.m.squeeze(-1)
    slack = 1e-4 * top.abs().clamp(min=1.0)
    assert bool((g["lse2"] >= top - slack).all()) and bool((g["lse2"] <= top + torch.log2(torch.tensor(float(Lk))) + slack).all())
    assert bool((g["o"].abs() <= ref.v.abs().amax(2, keepdim=True) * (1 + 2.0 ** -7)).all())
    assert bool((g["dv"].abs() <= ref.dO.abs().sum(2, keepdim=True) * (1 + 2.0 ** -7) + 1e-6).all())
    if c.planted is not None:                                                # o is the planted integer, exactly
        want = torch.gather(ref.v, 2, c.planted[..., None].expand(-1, -1, -1, 64))
        assert torch.equal(g["o"], want)
    r2 = _run(hip, c, "own_k")                                               # the other layout: the same bits
    for n in r:
        assert torch.equal(r[n], r2[n]), n


@pytest.mark.parametrize("L", [65, 200])
def test_packed_operands_reproduce_the_packed_kernels_bit_for_bit(hip, L):
    c = A.build_case("full", "random1", L, 64)
    B, H = c.B, c.H
    D = 64 * H
    qkv, dO = c.qkv.cuda(), c.dO.cuda()
    o, lse2 = hip.attention_fwd(qkv, B, L, H)
    dqkv = hip.attention_bwd(qkv, o, dO, lse2, B, L, H)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    o2, lse2b = hip.attention_cross_fwd(q, k, v, B, L, L, H)
    dqkv2 = torch.full_like(qkv, SENTINEL)
    hip.attention_cross_bwd(q, k, v, o2, dO, lse2b, B, L, L, H, dq=dqkv2[:, :D], dk=dqkv2[:, D:2 * D], dv=dqkv2[:, 2 * D:])
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse2, lse2b) and torch.equal(dqkv, dqkv2)


def test_second_backward_reproduces_every_bit(hip):
    c = X.build_case("random1", 333, 129)
    a, b = _run(hip, c, "wide"), _run(hip, c, "wide")
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_refusals(hip):
    B, Lq, Lk, H, D = 1, 8, 8, 2, 128
    q = torch.zeros(Lq, D + 8, device="cuda", dtype=torch.bfloat16)
    kv = torch.zeros(Lk, 2 * D, device="cuda", dtype=torch.bfloat16)
    o = torch.zeros(Lq, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros(B, H, Lq, device="cuda")
    L, p = hip.lib(), hip.ptr

    def fwd(qp=None, q_rs=D + 8, k_rs=2 * D, hd=64, lq=Lq):
        return L.vt_attention_cross_fwd(qp or p(q), q_rs, p(kv), k_rs, p(kv[:, D:]), 2 * D, B, lq, Lk, H, hd, p(o), p(lse), hip.stream())
    assert fwd() == 0
    # each call is made inside the loop: vt_last_error holds only the latest refusal
    for kw, what in ((dict(hd=32), "head_dim 32"), (dict(k_rs=D - 8), "row stride"), (dict(q_rs=D + 4), "multiple of 8"), (dict(lq=0), "bad shape"), (dict(k_rs=1 << 24), "too large"),
                     (dict(qp=p(q[:, 4:])), "16-byte aligned")):
        assert fwd(**kw) != 0, what
        buf = ctypes.create_string_buffer(512)
        L.vt_last_error(buf, 512)
        assert what in buf.value.decode(), (what, buf.value)
    with pytest.raises(hip.HipError, match="head_dim 32"):
        hip.attention_cross_fwd(q[:, :64], kv[:, :64], kv[:, 64:128], B, Lq, Lk, 2, hd=32)
    with pytest.raises(hip.HipError, match="16-byte aligned"):
        hip.attention_cross_bwd(q[:, :D], kv[:, :D], kv[:, D:], o, o, lse, B, Lq, Lk, H, dq=torch.zeros(Lq, D + 8, device="cuda", dtype=torch.bfloat16)[:, 4:D + 4])
    with pytest.raises(hip.HipError, match="GPU tensors only"):
        hip.attention_cross_fwd(q[:, :D].cpu(), kv[:, :D], kv[:, D:], B, Lq, Lk, H)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ row passes
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("M", [1, 67, 520])
def test_head_rmsnorm_forward_backward(hip, M, H):
    D, eps = 64 * H, 1e-6
    xbuf = torch.full((M, D + 64), LOUD, device="cuda", dtype=torch.bfloat16)
    xbuf[:, :D] = (torch.from_numpy(gen.normal((M, D), 31 + M + H)).cuda() * 1.7).to(torch.bfloat16)
    x = xbuf[:, :D]                                                           # strided rows
    w = 1.0 + torch.from_numpy(gen.normal((64,), 32, 0.2)).cuda()
    dybuf = torch.full((M, D + 8), LOUD, device="cuda", dtype=torch.bfloat16)
    dybuf[:, 8:] = torch.from_numpy(gen.normal((M, D), 33)).cuda().to(torch.bfloat16)
    dy = dybuf[:, 8:]
    y = hip.head_rmsnorm_fwd(x, w, eps, H)
    # fp32 math; the forward with its two roundings, the backward as the derivative of the unrounded formula (vt_hip.h)
    xr = x.float().reshape(M, H, 64).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    u = xr * torch.rsqrt((xr * xr).mean(-1, keepdim=True) + eps)
    ref = u * wr
    yref = rb(rb(u.detach()) * w).reshape(M, D)
    assert torch.equal(y.float(), yref) or bool(((y.float() - yref).abs() <= 2 ** -7 * yref.abs()).all())     # 1 bf16 ulp, element by element
    ref.backward(dy.float().reshape(M, H, 64))
    dx, dw = hip.head_rmsnorm_bwd(dy, x, w, eps, H)
    assert rel(dx, xr.grad.reshape(M, D)) < 4e-3
    assert rel(dw, wr.grad) < 1e-5
    dx2, dw2 = hip.head_rmsnorm_bwd(dy, x, w, eps, H)
    assert torch.equal(dw, dw2) and torch.equal(dx, dx2)                      # no atomics: bit-equal run to run
    snap = dybuf.clone()
    dx3, dw3 = hip.head_rmsnorm_bwd(dy, x, w, eps, H, dx=dy)                  # in place: the same bits, nothing outside the columns touched
    torch.cuda.synchronize()
    assert dx3.data_ptr() == dy.data_ptr() and torch.equal(dy, dx) and torch.equal(dw3, dw)
    assert torch.equal(dybuf[:, :8], snap[:, :8]) and bool((xbuf[:, D:] == LOUD).all())


def test_head_rmsnorm_refusals(hip):
    x = torch.zeros(4, 128, device="cuda", dtype=torch.bfloat16)
    w = torch.ones(64, device="cuda")
    with pytest.raises(hip.HipError, match="row strides"):             # a stride below 64 H
        hip.check(hip.lib().vt_head_rmsnorm_fwd(hip.ptr(x), 120, hip.ptr(w), 1e-6, 4, 2, hip.ptr(torch.empty_like(x)), 128, hip.stream()), "vt_head_rmsnorm_fwd")
    with pytest.raises(hip.HipError, match="GPU tensors only"):
        hip.head_rmsnorm_fwd(x.cpu(), w, 1e-6, 2)
    with pytest.raises(hip.HipError, match="not x's"):
        hip.head_rmsnorm_bwd(x, x, w, 1e-6, 2, dx=x)
    wide = torch.zeros(4, 144, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(hip.HipError, match="overlaps dy"):             # in place means dy itself, not a shifted view of its buffer
        hip.head_rmsnorm_bwd(wide[:, :128], x, w, 1e-6, 2, dx=wide[:, 8:136])
    with pytest.raises(hip.HipError, match="overlaps x"):
        hip.head_rmsnorm_bwd(x, wide[:, :128], w, 1e-6, 2, dx=wide[:, 8:136])


@pytest.mark.parametrize("M,D", [(1, 128), (67, 256), (520, 512)])
def test_sigmoid_gate_cols_equals_sigmoid_gate_on_the_packed_layout(hip, M, D):
    qkvg = torch.from_numpy(gen.normal((M, 4 * D), 41 + M, 2.0)).cuda().to(torch.bfloat16)
    o = torch.from_numpy(gen.normal((M, D), 42)).cuda().to(torch.bfloat16)
    dog = torch.from_numpy(gen.normal((M, D), 43)).cuda().to(torch.bfloat16)
    og = hip.sigmoid_gate_fwd(o, qkvg)
    dqkvg = torch.full_like(qkvg, SENTINEL)
    d_o = hip.sigmoid_gate_bwd(dog, o, qkvg, dqkvg)
    og2 = hip.sigmoid_gate_cols_fwd(o, qkvg[:, 3 * D:])
    dqkvg2 = torch.full_like(qkvg, SENTINEL)
    d_o2 = hip.sigmoid_gate_cols_bwd(dog, o, qkvg[:, 3 * D:], dqkvg2[:, 3 * D:])
    assert torch.equal(og, og2) and torch.equal(d_o, d_o2) and torch.equal(dqkvg, dqkvg2)
    assert bool((dqkvg2[:, :3 * D] == SENTINEL).all())
    # the layer's layout: gate = columns D..2D of [M, 2D]; same arithmetic, same bits
    qg = torch.cat([qkvg[:, :D], qkvg[:, 3 * D:]], 1).contiguous()
    dqg = torch.full_like(qg, SENTINEL)
    assert torch.equal(hip.sigmoid_gate_cols_fwd(o, qg[:, D:]), og)
    assert torch.equal(hip.sigmoid_gate_cols_bwd(dog, o, qg[:, D:], dqg[:, D:]), d_o)
    assert torch.equal(dqg[:, D:], dqkvg[:, 3 * D:]) and bool((dqg[:, :D] == SENTINEL).all())
    ref = o.float() * rb(torch.sigmoid(qkvg[:, 3 * D:].float()))
    assert (og.float() - rb(ref)).abs().max() <= 2 ** -7 * ref.abs().max()


@pytest.mark.parametrize("dim", [128, 256, 512])
@pytest.mark.parametrize("rows", [1, 67, 2048])
def test_rmsnorm_any_forward_backward(hip, dim, rows):
    """the assertions of test_ar_gpu.test_rmsnorm_forward_backward at the design widths"""
    x = torch.from_numpy(gen.normal((rows, dim), 11 + dim)).cuda() * 1.7
    w = 1.0 + torch.from_numpy(gen.normal((dim,), 12, 0.2)).cuda()
    dy = rb(torch.from_numpy(gen.normal((rows, dim), 13)).cuda())
    dres = torch.from_numpy(gen.normal((rows, dim), 14)).cuda()
    y, rstd = hip.rmsnorm_any_fwd(x, w, 1e-5)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    ref = xr * torch.rsqrt((xr * xr).mean(-1, keepdim=True) + 1e-5) * wr
    assert torch.equal(y.float(), rb(ref.detach())) or (y.float() - rb(ref.detach())).abs().max() <= 2 ** -7 * ref.detach().abs().max()   # 1 bf16 ulp
    assert rel(y, ref.detach()) < 4e-3
    assert rel(rstd, torch.rsqrt((x * x).mean(-1) + 1e-5)) < 1e-6
    ref.backward(dy)
    dx, dxb, dw = hip.rmsnorm_any_bwd(dy.to(torch.bfloat16), x, w, rstd, dres=dres, want_bf16=True)
    assert rel(dx, xr.grad + dres) < 1e-5
    assert rel(dxb, xr.grad + dres) < 4e-3
    assert rel(dw, wr.grad) < 1e-5
    dx2, none, dw2 = hip.rmsnorm_any_bwd(dy.to(torch.bfloat16), x, w, rstd)
    assert none is None and rel(dx2, xr.grad) < 1e-5 and torch.equal(dw2, dw)


@pytest.mark.parametrize("rows", [1, 67, 2048])
def test_rmsnorm_any_equals_rmsnorm_where_both_accept(hip, rows):
    dim = 384
    x = torch.from_numpy(gen.normal((rows, dim), 51)).cuda() * 1.7
    w = 1.0 + torch.from_numpy(gen.normal((dim,), 52, 0.2)).cuda()
    dy = torch.from_numpy(gen.normal((rows, dim), 53)).cuda().to(torch.bfloat16)
    y, rstd = hip.rmsnorm_fwd(x, w, 1e-5)
    y2, rstd2 = hip.rmsnorm_any_fwd(x, w, 1e-5)
    assert torch.equal(y, y2) and torch.equal(rstd, rstd2)
    a, b = hip.rmsnorm_bwd(dy, x, w, rstd, want_bf16=True), hip.rmsnorm_any_bwd(dy, x, w, rstd, want_bf16=True)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    with pytest.raises(hip.HipError, match="unsupported"):
        hip.rmsnorm_any_fwd(torch.zeros(4, 192, device="cuda"), torch.ones(192, device="cuda"), 1e-5)
    with pytest.raises(hip.HipError, match="GPU tensors only"):
        hip.rmsnorm_any_fwd(torch.zeros(4, 512), torch.ones(512), 1e-5)


@pytest.mark.parametrize("rows,dim", [(5, 128), (1029, 384), (8197, 128), (9, 2560)])
def test_rmsnorm_any_f32_equals_rmsnorm_any_up_to_the_output_rounding(hip, rows, dim):
    """the fp32 and the bf16 family are instances of one kernel template: the same statistics, the same products, and the only difference the
    rounding of y.  5 rows: a partial block; 1029: one row past a full sweep of the backward's 256 x 4-row grid; 8197: one row past the
    forward's 2048-block cap; 2560: the last width of the dispatch"""
    x = torch.from_numpy(gen.normal((rows, dim), 54)).cuda() * 1.7
    w = 1.0 + torch.from_numpy(gen.normal((dim,), 55, 0.2)).cuda()
    dy = torch.from_numpy(gen.normal((rows, dim), 56)).cuda().to(torch.bfloat16)      # exactly representable in both families' input type
    y, rstd = hip.rmsnorm_any_fwd(x, w, 1e-5)
    y32, rstd32 = hip.rmsnorm_any_f32_fwd(x, w, 1e-5)
    assert torch.equal(rstd32, rstd)
    assert y32.dtype == torch.float32 and torch.equal(y32.to(torch.bfloat16), y)
    dx, _, dw = hip.rmsnorm_any_bwd(dy, x, w, rstd)
    dx32, dw32 = hip.rmsnorm_any_f32_bwd(dy.float(), x, w, rstd)
    assert torch.equal(dx32, dx) and torch.equal(dw32, dw)
