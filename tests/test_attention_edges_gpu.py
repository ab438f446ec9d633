"""The attention kernels at their edges: every case of tests/attention_cases.py (flat, planted, ramp, random; every tile / tail / query-block
shape; kept-query suffixes; causal; decode against a poisoned cache) through hip.attention_* and hip.decode_attention*, against the
float64 reference with the tolerances that module derives from the reference alone: a quarter of the smallest deviation a one-element
miscount makes, at most 0.5 row-relative, and asserted only where that is at least 8 x the rounding noise of a correct kernel (the
quantities a case leaves out are named in attention_cases.NOT_ASSERTED; tests/test_attention_cases_cpu.py holds both to account).  On
top of the tolerances every case is held to the ranges the formula allows whatever the data (`_check_ranges`), which a poison row would
leave.  Each test prints `BAR <case> <quantity> <error> <tolerance> <error / tolerance>` before it asserts.

Measured on an MI355X when these tests were written, largest error / tolerance per kernel and family over the asserted quantities
(lse2, o, dQ, dK, dV; - = not asserted in that family):
    full    flat .003 .102 .116 - .125   planted 0 0 - - 0   ramp .071 .135 .121 .135 .125   random .068 .080 .057 .268 .050
    rows    flat 0 .124 .125 - .119      planted 0 0 - - 0   ramp .146 .127 - .124 .123      random .115 .179 .315 .238 .104
    causal  flat .004 .114 .117 - .122   planted 0 0 - - 0   ramp .217 .125 .119 .126 .124   random .083 .202 .124 .163 .087
    decode  o: flat .106, planted 0, ramp .116, random .118"""
import pytest
import torch

from tests import attention_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _heads(t, B, L, H, hd):
    """[B * L, H * hd] -> [B, H, L, hd]"""
    return t.reshape(B, L, H, hd).permute(0, 2, 1, 3)


def _split(dqkv, B, L, H, hd):
    x = dqkv.reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    return {"dq": x[0], "dk": x[1], "dv": x[2]}


def _run(hip, c, qkv, dO, B=None, q_begin=None):
    B = c.B if B is None else B
    qb = c.q_begin if q_begin is None else q_begin
    if c.causal:
        o, lse2 = hip.attention_causal_fwd(qkv, B, c.L, c.H)
        dqkv = hip.attention_causal_bwd(qkv, o, dO, lse2, B, c.L, c.H)
    else:
        o, lse2 = hip.attention_fwd(qkv, B, c.L, c.H, c.hd, q_begin=qb)
        dqkv = hip.attention_bwd(qkv, o, dO, lse2, B, c.L, c.H, c.hd, q_begin=qb)
    torch.cuda.synchronize()
    return o, lse2, dqkv


def _check(name, got, bars, failures):
    ref = bars.ref.base
    for n, t in got.items():
        t = t.double().cpu()
        assert torch.isfinite(t).all(), (name, n)
        err = float(A.row_err(n, t, ref[n]).max())
        if bars.tol[n] is None:                   # named in attention_cases.NOT_ASSERTED: no bar, the figure is printed all the same
            print(f"BAR {name} {n} {err:.3e} unasserted -")
            continue
        print(f"BAR {name} {n} {err:.3e} {bars.tol[n]:.3e} {err / bars.tol[n]:.3f}")
        if not err <= bars.tol[n]:
            failures.append((n, err, bars.tol[n]))


def _check_ranges(c, ref, got):
    """What the formula allows whatever the data, for every family and every quantity; a poison row (v = 1000, keys of twice the magnitude,
    all outside the sequence's own values) that entered a sum would leave these ranges:
       max_j s_ij <= lse2_i <= max_j s_ij + log2(visible keys);  |o_i| <= max_j |v_j| over the visible keys (a convex combination);
       |dV_j| <= sum_i |dO_i| (P <= 1);  |dK_j| <= 2 scale max|v| sum_i |dO_i|_1 |q_i| (|dS_ij| <= P_ij (|dO_i . v_j| + |dO_i . o_i|))"""
    qb = c.q_begin
    g = {n: t.double().cpu() for n, t in got.items()}
    cnt = ref.vis.sum(-1)
    top = ref.m.squeeze(-1)
    slack = 1e-4 * top.abs().clamp(min=1.0)
    assert bool((g["lse2"] >= top - slack).all()) and bool((g["lse2"] <= top + torch.log2(cnt) + slack).all())
    vabs = ref.v.abs()
    vmax = torch.cummax(vabs, dim=2)[0][:, :, qb:] if c.causal else vabs.amax(2, keepdim=True)
    assert bool((g["o"].abs() <= vmax * (1 + 2.0 ** -7)).all())
    dOabs = ref.dO.abs()
    assert bool((g["dv"].abs() <= dOabs.sum(2, keepdim=True) * (1 + 2.0 ** -7) + 1e-6).all())
    kb = 2 * ref.scale * vabs.amax((2, 3), keepdim=True) * (dOabs.sum(-1, keepdim=True) * ref.qk.abs()).sum(2, keepdim=True)
    assert bool((g["dk"].abs() <= kb * (1 + 2.0 ** -6) + 1e-6).all())


@pytest.mark.parametrize("key", A.case_keys(), ids=A.key_id)
def test_attention_case(hip, key):
    bars = A.bars(*key)
    c = bars.case
    B, L, H, hd, qb = c.B, c.L, c.H, c.hd, c.q_begin
    Lq = L - qb
    backing = c.backing.cuda()                    # the case's rows and, behind them, the poison rows of the same allocation
    qkv = backing[: B * L]
    dO = c.dO.cuda()
    o, lse2, dqkv = _run(hip, c, qkv, dO)
    got = {"lse2": lse2[:, :, qb:], "o": _heads(o, B, Lq, H, hd)}
    got.update(_split(dqkv, B, L, H, hd))
    failures = []
    _check(A.key_id(key), got, bars, failures)
    assert not failures, failures
    _check_ranges(c, bars.ref, got)
    assert torch.equal(backing.cpu(), c.backing)                                             # the operand is read-only
    if c.planted is not None:                                                                # o is the planted integer, exactly
        v = c.qkv64()[2]
        want = torch.gather(v, 2, c.planted[:, :, qb:, None].expand(-1, -1, -1, hd))
        assert torch.equal(got["o"].double().cpu(), want)
    if qb:
        assert torch.all(got["dq"][:, :, :qb] == 0)                                          # queries before q_begin: exactly zero gradient
        # the same kernels as the full call: the kept rows are bit-equal to it (dO of the dropped queries = 0 adds exact zeros to dK / dV)
        dO_full = torch.zeros(B, L, H * hd, device="cuda", dtype=torch.bfloat16)
        dO_full[:, qb:] = dO.reshape(B, Lq, H * hd)
        o_f, lse_f, d_f = _run(hip, c, qkv, dO_full.reshape(B * L, H * hd), q_begin=0)
        assert torch.equal(o, o_f.reshape(B, L, H * hd)[:, qb:].reshape(B * Lq, H * hd))
        assert torch.equal(lse2[:, :, qb:], lse_f[:, :, qb:])
        g_r, g_f = _split(dqkv, B, L, H, hd), _split(d_f, B, L, H, hd)
        assert torch.equal(g_r["dq"][:, :, qb:], g_f["dq"][:, :, qb:])
        assert torch.equal(g_r["dk"], g_f["dk"]) and torch.equal(g_r["dv"], g_f["dv"])
    for b in range(B):                                                                       # a sequence alone = the same sequence in the batch, bit for bit
        o1, lse1, d1 = _run(hip, c, qkv[b * L:(b + 1) * L].clone(), dO[b * Lq:(b + 1) * Lq].clone(), B=1)
        assert torch.equal(o1, o[b * Lq:(b + 1) * Lq]), b
        assert torch.equal(lse1[0, :, qb:], lse2[b, :, qb:]), b
        assert torch.equal(d1, dqkv[b * L:(b + 1) * L]), b


@pytest.mark.parametrize("family,n_keys", A.decode_keys(), ids=lambda v: str(v))
def test_decode_case(hip, family, n_keys):
    c = A.decode_case(family, n_keys)
    d = c.bars()
    B, H, Lmax = c.B, c.H, c.Lmax
    q, kc, vc = c.q.cuda(), c.kc.cuda(), c.vc.cuda()
    o = hip.decode_attention(q, kc, vc, n_keys)
    torch.cuda.synchronize()
    assert torch.equal(kc.cpu(), c.kc) and torch.equal(vc.cpu(), c.vc)
    ref = c.reference()
    err = float(A.row_err("o", o.double().cpu(), ref).max())
    if d["tol"] is None:                          # named in attention_cases.DECODE_NOT_ASSERTED
        print(f"BAR {c.name} o {err:.3e} unasserted -")
    else:
        print(f"BAR {c.name} o {err:.3e} {d['tol']:.3e} {err / d['tol']:.3f}")
        assert err <= d["tol"], (err, d["tol"])
    if c.planted is not None:
        want = torch.gather(c.vc[:B].double(), 2, c.planted[:, :, None, None].expand(-1, -1, 1, 64)).squeeze(2)
        assert torch.equal(o.double().cpu(), want)
    vmax = c.vc[:B, :, :n_keys].double().abs().amax(2)                                       # a convex combination of the visible V rows: poison
    assert bool((o.double().cpu().abs() <= vmax * (1 + 2.0 ** -7)).all())                    # (v = 1000) would leave their range
    # the step variant at pos = n_keys - 1: the new token's k / v arrive in the projection row, the cache row at pos holds poison until then
    pos = n_keys - 1
    qkv = torch.cat([q.reshape(B, H * 64), kc[:B, :, pos].reshape(B, H * 64), vc[:B, :, pos].reshape(B, H * 64)], 1).contiguous()
    kc2, vc2 = kc.clone(), vc.clone()
    kc2[:B, :, pos], vc2[:B, :, pos] = 64.0, A.POISON_V
    o2 = hip.decode_attention_step(qkv, kc2, vc2, torch.tensor([pos], device="cuda", dtype=torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(kc2, kc) and torch.equal(vc2, vc)                                     # row pos = the new k / v; every other row untouched
    assert torch.equal(o2.reshape(B, H, 64), o)
