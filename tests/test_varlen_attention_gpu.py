"""vt_attention_varlen_fwd / _bwd (packed variable-length attention, grouped KV heads) and vt_qknorm_rope_gqa_* on the GPU.

The kernels are the tile code of vt_attention_cross_* behind another address computation, so most of what is asserted here is BIT equality:
  1. one sequence, Hq == Hkv                 == vt_attention_cross_* with B = 1 (o, lse2, dq, dk, dv)
  2. a packed launch                         == the concatenation of per-sequence launches of the same entry point, for both packings and
                                                every head pair; operands are views of backing allocations with poison rows behind them,
                                                outputs are pre-filled with a sentinel: every owned row is written and nothing else is
  3. grouped (4, 2) and (6, 2)               == the (Hq, Hq) run on K / V whose head columns are expanded by repeat_interleave, in o, lse2, dq;
                                                dk / dv against the float64 reference within the Bars of tests/varlen_attention_cases.py
                                                (the random1 case of the packing), and, as an extra, against the expanded run's per-head
                                                shares element by element (see _group_sum_bound)
  4. every case of tests/varlen_attention_cases.py (four families x three packings x three head pairs), every asserted quantity against
     its Bars tolerance, NOT_ASSERTED honoured; prints `BAR <case> <quantity> <error> <tolerance> <error / tolerance>`
  5. a second identical backward reproduces every bit
  6. the row pass: with Hq == Hkv and a [M, 4D] input bit-identical to vt_qknorm_rope_fwd / _bwd called with L = M; the grouped layout
     against fp32 math with the same rounding points at the tolerances of tests/test_titok_gpu.py; rows past M and columns outside the
     three blocks untouched
Shapes: the packings put every boundary on a different row offset, with lengths at the tile (64), half-tile and block (128) edges.
Measured on an MI355X: every bit equality holds; grouped dk / dv lie at 0.77 - 0.91 of the element-wise bound (GROUPSUM lines).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import inputs as gen
from oracle.larp_oracle import _rb
from tests import attention_cases as A
from tests import varlen_attention_cases as V

pytestmark = pytest.mark.gpu

PACKINGS, HEADS = V.PACKINGS, V.HEADS
POISON_ROWS = 8
SENTINEL = 0x7FC1                   # a bf16 NaN payload no kernel produces, as int16


@pytest.fixture(scope="module")
def vt():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd as v
    v.hip.lib()
    return v


def cu_of(lengths):
    return [0] + list(np.cumsum(lengths))


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def operands(lengths, Hq, Hkv, seed):
    """q | k | v as the three column blocks of ONE backing projection [M + POISON_ROWS, 64 (Hq + 2 Hkv)] (N(0, 1); the rows behind M hold a
    loud key and v = 1000), dO likewise behind its own poison -> (q, k, v, dO) device views of M rows"""
    M = int(sum(lengths))
    W = 64 * (Hq + 2 * Hkv)
    back = torch.from_numpy(gen.normal((M + POISON_ROWS, W), seed)).to(torch.bfloat16)
    back[M:, : 64 * (Hq + Hkv)] = 4.0
    back[M:, 64 * (Hq + Hkv):] = 1000.0
    dO = torch.from_numpy(gen.normal((M + POISON_ROWS, 64 * Hq), seed + 1)).to(torch.bfloat16)
    dO[M:] = 1000.0
    back, dO = back.cuda(), dO.cuda()
    D, G = 64 * Hq, 64 * Hkv
    return back[:M, :D], back[:M, D:D + G], back[:M, D + G:], dO[:M].contiguous()


def sentinel(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def run(vt, q, k, v, dO, cu, Hq, Hkv):
    """forward + backward into sentinel-filled backings -> dict of the owned views, after checking that nothing else was written"""
    M, D, G = q.shape[0], 64 * Hq, 64 * Hkv
    o_back = sentinel(M + POISON_ROWS, D)
    lse_back = torch.full((Hq * M + 64,), float("nan"), device="cuda")
    o, lse2 = vt.hip.attention_varlen_fwd(q, k, v, cu, Hq, Hkv, o=o_back[:M], lse2=lse_back[: Hq * M].view(Hq, M))
    gback = sentinel(M + POISON_ROWS, D + 2 * G + 64)                    # dq | dk | dv | 64 spare columns
    dq, dk, dv = vt.hip.attention_varlen_bwd(q, k, v, o, dO, lse2, cu, Hq, Hkv, dq=gback[:M, :D], dk=gback[:M, D:D + G], dv=gback[:M, D + G:D + 2 * G])
    torch.cuda.synchronize()
    assert bool((bits(o_back[M:]) == SENTINEL).all()) and bool(torch.isnan(lse_back[Hq * M:]).all())
    assert bool((bits(gback[M:]) == SENTINEL).all()) and bool((bits(gback[:, D + 2 * G:]) == SENTINEL).all())
    out = dict(o=o, lse2=lse2, dq=dq, dk=dk, dv=dv)
    for n, t in out.items():                                             # every owned element written, finite
        assert bool(torch.isfinite(t.float()).all()), n
    return out


@pytest.mark.parametrize("L", (1, 65, 200, 333))
def test_single_sequence_equals_cross_kernels(vt, L):
    H = 2
    q, k, v, dO = operands((L,), H, H, 7100 + L)
    got = run(vt, q, k, v, dO, [0, L], H, H)
    o, lse2 = vt.hip.attention_cross_fwd(q, k, v, 1, L, L, H)
    dq, dk, dv = vt.hip.attention_cross_bwd(q, k, v, o, dO, lse2, 1, L, L, H)
    want = dict(o=o, lse2=lse2.reshape(H, L), dq=dq, dk=dk, dv=dv)
    for n in want:
        assert same_bits(got[n], want[n]), n


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"h{h[0]}-{h[1]}")
@pytest.mark.parametrize("lengths", PACKINGS[:2], ids=("rising", "reversed"))
def test_packed_equals_separate_sequences(vt, lengths, heads):
    Hq, Hkv = heads
    q, k, v, dO = operands(lengths, Hq, Hkv, 7200 + 10 * Hq + len(lengths) + lengths[0])
    cu = cu_of(lengths)
    got = run(vt, q, k, v, dO, cu, Hq, Hkv)
    for b, L in enumerate(lengths):
        r = slice(cu[b], cu[b + 1])
        one = run(vt, q[r], k[r], v[r], dO[r], [0, L], Hq, Hkv)          # neighbours do not exist for this launch
        for n in ("o", "dq", "dk", "dv"):
            assert same_bits(got[n][r], one[n]), (n, b, L)
        assert same_bits(got["lse2"][:, r], one["lse2"]), ("lse2", b, L)


def case_operands(c):
    """the case's backings on the device as ONE projection-like buffer q | k | v (poison rows behind it) -> (q, k, v, dO) views of M rows"""
    M = c.M
    back = torch.cat([c.q_backing, c.k_backing, c.v_backing], 1).contiguous().cuda()
    D, G = 64 * c.Hq, 64 * c.Hkv
    return back[:M, :D], back[:M, D:D + G], back[:M, D + G:], c.dO_backing.cuda()[:M]


def by_head(t, H):
    """[M, 64 H] -> float64 [H, M, 64] on the CPU, the layout of the references"""
    return t.reshape(t.shape[0], H, 64).permute(1, 0, 2).double().cpu()


def assert_bars(bars, got, label, only=None):
    c, failures = bars.case, []
    ref = {"lse2": got["lse2"].double().cpu(), "o": by_head(got["o"], c.Hq), "dq": by_head(got["dq"], c.Hq), "dk": by_head(got["dk"], c.Hkv),
           "dv": by_head(got["dv"], c.Hkv)}
    for n in only or (V.FWD_Q + V.BWD_Q):
        err = float(A.row_err(n, ref[n], bars.ref.base[n]).max())
        if bars.tol[n] is None:                   # named in varlen_attention_cases.NOT_ASSERTED: no bar, the figure is printed all the same
            print(f"BAR {label} {n} {err:.3e} unasserted -")
            continue
        print(f"BAR {label} {n} {err:.3e} {bars.tol[n]:.3e} {err / bars.tol[n]:.3f}")
        if not err <= bars.tol[n]:
            failures.append((n, err, bars.tol[n]))
    assert not failures, failures


@pytest.mark.parametrize("key", V.case_keys(), ids=V.key_id)
def test_varlen_attention_case(vt, key):
    bars = V.bars(*key)
    c = bars.case
    q, k, v, dO = case_operands(c)
    got = run(vt, q, k, v, dO, c.cu, c.Hq, c.Hkv)
    assert_bars(bars, got, V.key_id(key))


@pytest.mark.parametrize("heads", ((4, 2), (6, 2)), ids=lambda h: f"h{h[0]}-{h[1]}")
@pytest.mark.parametrize("lengths", PACKINGS, ids=("rising", "reversed", "one200"))
def test_grouped_equals_head_expanded(vt, lengths, heads):
    Hq, Hkv = heads
    g = Hq // Hkv
    bars = V.bars("random1", lengths, heads)                             # N(0, 1) operands, poison rows behind them
    q, k, v, dO = case_operands(bars.case)
    cu = cu_of(lengths)
    M = q.shape[0]
    got = run(vt, q, k, v, dO, cu, Hq, Hkv)
    kx = k.reshape(M, Hkv, 64).repeat_interleave(g, dim=1).reshape(M, 64 * Hq).contiguous()
    vx = v.reshape(M, Hkv, 64).repeat_interleave(g, dim=1).reshape(M, 64 * Hq).contiguous()
    exp = run(vt, q, kx, vx, dO, cu, Hq, Hq)
    for n in ("o", "lse2", "dq"):
        assert same_bits(got[n], exp[n]), n
    assert bars.tol["dk"] is not None and bars.tol["dv"] is not None
    assert_bars(bars, got, "grouped-" + V.key_id(("random1", lengths, heads)), only=("dk", "dv"))      # against the float64 reference
    for n in ("dk", "dv"):                                               # extra: against the expanded run's per-head shares
        share = exp[n].float().reshape(M, Hkv, g, 64)                    # every query head's share, each rounded to bf16 by the expanded run
        err, bound = _group_sum_bound(got[n].float().reshape(M, Hkv, 64), share)
        print(f"GROUPSUM {n} heads={heads} lengths={len(lengths)}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (n, float((err / bound).max()))
        assert float(share.abs().sum(2).max()) > 1.0                     # the bound is not vacuous: the shares are O(1) and larger


def _group_sum_bound(grouped, share):
    """grouped = bf16(S), S the fp32 sum over the group's heads of a_j (in one accumulator, ascending heads); share_j = bf16(a_j).
    bf16 carries 8 significant bits (7 stored), so round-to-nearest has unit roundoff u = 2^-8: |bf16(x) - x| <= u |x|.  Hence
    |a_j - share_j| <= u |a_j| <= u (1 + 2u) |share_j| and |grouped - S| <= u |S| <= u (1 + 2u) sum_j |share_j| + u^2 (...), together
    |grouped - sum_j share_j| <= 2 u (1 + 2u) sum_j |share_j|: the bound below takes 2^-7 x 1.02 x sum_j |share_j|.  The fp32 re-association
    between one accumulator and g of them is of the order 2^-22 of that and inside the 2 %.  (No bf16 underflow: the inputs are N(0, 1).)"""
    total = share.sum(2)
    mag = share.abs().sum(2)
    return (grouped - total).abs(), 2.0 ** -7 * 1.02 * mag + 1e-30


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"h{h[0]}-{h[1]}")
def test_backward_is_reproducible(vt, heads):
    Hq, Hkv = heads
    lengths = PACKINGS[0]
    q, k, v, dO = operands(lengths, Hq, Hkv, 7400 + Hq)
    cu = cu_of(lengths)
    a = run(vt, q, k, v, dO, cu, Hq, Hkv)
    b = run(vt, q, k, v, dO, cu, Hq, Hkv)
    for n in a:
        assert same_bits(a[n], b[n]), n


def test_varlen_attend_function_and_cpu_refusal(vt):
    Hq, Hkv = 4, 2
    lengths = (65, 1, 130)
    q, k, v, dO = operands(lengths, Hq, Hkv, 7500)
    cu = cu_of(lengths)
    want = run(vt, q, k, v, dO, cu, Hq, Hkv)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    for cu_arg in (cu, torch.tensor(cu, dtype=torch.int32), torch.tensor(cu, device="cuda")):      # list, CPU tensor, device tensor
        for t in leaves:
            t.grad = None
        o = vt.functional.VarlenAttend.apply(*leaves, cu_arg, Hq, Hkv)
        o.backward(dO)
        assert same_bits(o, want["o"])
        for t, n in zip(leaves, ("dq", "dk", "dv")):
            assert same_bits(t.grad, want[n]), n
    with pytest.raises(vt.hip.HipError):
        vt.hip.attention_varlen_fwd(q.cpu(), k.cpu(), v.cpu(), cu, Hq, Hkv)
    with pytest.raises(vt.hip.HipError):                                 # an empty sequence is refused by the library
        vt.hip.attention_varlen_fwd(q, k, v, [0, 65, 65, 196], Hq, Hkv)


# ---------------------------------------------------------------------------------------------------------------------------------
# the row pass
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm_params(seed):
    return [torch.from_numpy(a) for a in (1 + gen.normal((64,), seed, 0.1), gen.normal((64,), seed + 1, 0.1), 1 + gen.normal((64,), seed + 2, 0.1),
                                          gen.normal((64,), seed + 3, 0.1))]


def _tables(M, seed):
    ang = torch.from_numpy(gen.normal((M, 32), seed, 2.0)).double()
    return ang, torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


@pytest.mark.parametrize("M", (1, 77, 200))
def test_row_pass_equals_dense_pass_bit_for_bit(vt, M):
    H = 4
    D = 64 * H
    _, cos, sin = _tables(M, 7600 + M)
    cos, sin = cos.cuda(), sin.cuda()
    qkvg = torch.from_numpy(gen.normal((M, 4 * D), 7601 + M, 1.5)).to(torch.bfloat16).cuda()
    up = torch.from_numpy(gen.normal((M, 3 * D), 7602 + M)).to(torch.bfloat16).cuda()
    par = [p.cuda() for p in _norm_params(7610)]
    want = vt.hip.qknorm_rope_fwd(qkvg, M, H, *par, 1e-5, cos, sin)                        # L = M: row m at table row m
    got = vt.hip.qknorm_rope_gqa_fwd(qkvg[:, :3 * D], H, H, *par, 1e-5, cos, sin)
    assert same_bits(got, want)
    dw = sentinel(M, 4 * D)
    gw = vt.hip.qknorm_rope_bwd(qkvg, up, M, H, par[0], par[2], 1e-5, cos, sin, dw)
    dg = sentinel(M, 4 * D)
    _, gg = vt.hip.qknorm_rope_gqa_bwd(qkvg[:, :3 * D], up, H, H, par[0], par[2], 1e-5, cos, sin, dqkv=dg[:, :3 * D])
    assert same_bits(dg, dw)                                                               # the gate columns keep the sentinel in both
    for a, b in zip(gg, gw):
        assert same_bits(a, b)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("heads", ((4, 2), (6, 2)), ids=lambda h: f"h{h[0]}-{h[1]}")
def test_row_pass_grouped_layout(vt, heads):
    """against fp32 math with the autocast rounding points (transformer.py:54-58, rope.py:18-24), at the tolerances tests/test_titok_gpu.py
    uses for vt_qknorm_rope_*; the input and both outputs are views of wider, longer backings that keep their sentinel"""
    Hq, Hkv = heads
    M = 135
    D, G = 64 * Hq, 64 * Hkv
    W = D + 2 * G
    ang, cos, sin = _tables(M, 7700 + Hq)
    x0 = torch.from_numpy(gen.normal((M, W), 7701 + Hq, 1.5)).to(torch.bfloat16)
    up = torch.from_numpy(gen.normal((M, W), 7702 + Hq)).to(torch.bfloat16)
    par = _norm_params(7710)
    x = x0.float().requires_grad_(True)
    pr = [p.clone().requires_grad_(True) for p in par]

    def rot(t):                                                                            # [M, h, 64] by table row m
        c = torch.view_as_complex(t.double().reshape(M, -1, 32, 2)) * torch.polar(torch.ones_like(ang), ang)[:, None]
        return torch.view_as_real(c).flatten(-2).float()

    qn = _rb(F.layer_norm(x[:, :D].reshape(M, Hq, 64), (64,), pr[0], pr[1], 1e-5), True)
    kn = _rb(F.layer_norm(x[:, D:D + G].reshape(M, Hkv, 64), (64,), pr[2], pr[3], 1e-5), True)
    ref = torch.cat([_rb(rot(qn), True).reshape(M, D), _rb(rot(kn), True).reshape(M, G), x[:, D + G:]], dim=1)
    (ref * up.float()).sum().backward()

    dev = [p.cuda() for p in par]
    in_back = sentinel(M + 3, W + 64)
    in_back[:M, :W] = x0.cuda()
    out_back = sentinel(M + 3, W + 128)
    out = vt.hip.qknorm_rope_gqa_fwd(in_back[:M, :W], Hq, Hkv, *dev, 1e-5, cos.cuda(), sin.cuda(), out=out_back[:M, :W])
    assert rel(out, ref) < 3e-3 and float((out.float().cpu() - ref.detach()).abs().max()) < 0.04
    assert same_bits(out[:, D + G:], in_back[:M, D + G:W])                                 # v is a copy
    assert bool((bits(out_back[M:]) == SENTINEL).all()) and bool((bits(out_back[:, W:]) == SENTINEL).all())
    d_back = sentinel(M + 3, W + 64)
    dqkv, grads = vt.hip.qknorm_rope_gqa_bwd(in_back[:M, :W], up.cuda(), Hq, Hkv, dev[0], dev[2], 1e-5, cos.cuda(), sin.cuda(), dqkv=d_back[:M, :W])
    assert rel(dqkv, x.grad) < 6e-3
    assert bool((bits(d_back[M:]) == SENTINEL).all()) and bool((bits(d_back[:, W:]) == SENTINEL).all())
    for g, p in zip(grads, pr):
        assert rel(g, p.grad) < 5e-3
