"""The data movement of the packed `titok` model (csrc/vt_packed.hip) on the GPU.  The kernels only move data, so equality is exact:
vt_patchify_clips / vt_unpatchify_clips against einops.rearrange (the reference's own patching, blocks.py:128 and :214-220) and against
vt_patchify; vt_packed_scatter / vt_packed_gather against the torch.cat / split constructions of blocks.py:132-142 and :197-209.

Every output lies in a buffer with sentinel-filled slack behind it, which must stay untouched; every input has NaN poison behind it, which
must not be read (a read would show in the exact comparisons).  vt_packed_segment_colsum adds, so it is held to the worst-case bound of
fp32 summation in ANY order, per column |got - float64 sum| <= R * 2^-24 * sum |x_r| over the R summed rows, and two runs must agree in
every bit; mutants (the other segment, the last sequence dropped) show that the bound is live on these inputs."""
import math

import pytest
import torch

from oracle import inputs as gen
from tests import titok_reference as R

pytestmark = pytest.mark.gpu

PT, P = 4, 8
SENTINEL = -12345.0
SLACK = 1024                                   # elements behind every buffer
COUNTS = {                                     # name -> (lead counts, sequence lengths)
    "case": (list(R.TOKENS), R.lengths()),     # [1, 65, 7, 128] over [2, 77, 15, 148]
    "one": ([1], [2]),
}


def vt():
    import video_tokenizer_amd
    return video_tokenizer_amd


def guarded(shape, dtype, fill):
    """a contiguous device tensor of `shape` at the head of a larger buffer whose tail holds `fill`; -> (view, tail)"""
    n = math.prod(shape)
    buf = torch.full((n + SLACK,), fill, device="cuda", dtype=dtype)
    return buf[:n].view(*shape), buf[n:]


def poisoned(t):
    """a device copy of t with NaN behind it"""
    view, _ = guarded(tuple(t.shape), t.dtype, float("nan"))
    view.copy_(t)
    return view


def untouched(tail):
    return bool((tail == SENTINEL).all())


def clip_list(sizes, seed):
    return [torch.from_numpy(gen.normal((3,) + tuple(s), seed + i)) for i, s in enumerate(sizes)]


def rows_of(vid):
    from einops import rearrange
    return rearrange(vid, "c (nt pt) (nh ph) (nw pw) -> (nt nh nw) (c pt ph pw)", pt=PT, ph=P, pw=P)


def clip_of(rows, size):
    from einops import rearrange
    T, H, W = size
    return rearrange(rows, "(nt nh nw) (c pt ph pw) -> c (nt pt) (nh ph) (nw pw)", nt=T // PT, nh=H // P, nw=W // P, pt=PT, ph=P, pw=P)


CLIP_SETS = {
    "case": list(R.CLIP_SIZES),
    "one clip": [(8, 16, 24)],
    "64 one-patch clips": [(4, 8, 8)] * 64,
    "two blocks in a clip": [(4, 8, 8), (8, 32, 40)],          # 3840 units = 15 workgroups of 256 for the second clip
}


@pytest.mark.parametrize("which", sorted(CLIP_SETS))
def test_patchify_clips_equals_the_reference_rearrange(which):
    sizes = CLIP_SETS[which]
    clips = clip_list(sizes, 7000)
    want = torch.cat([rows_of(v) for v in clips], 0).to(torch.bfloat16)
    out, tail = guarded(tuple(want.shape), torch.bfloat16, SENTINEL)
    got = vt().hip.patchify_clips([poisoned(v) for v in clips], PT, P, out=out)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and untouched(tail)
    assert torch.equal(vt().hip.patchify_clips([v.cuda() for v in clips], PT, P).cpu(), want)      # the wrapper's own allocation


@pytest.mark.parametrize("which", sorted(CLIP_SETS))
def test_unpatchify_clips_inverts_exactly(which):
    sizes = CLIP_SETS[which]
    G = sum((T // PT) * (H // P) * (W // P) for T, H, W in sizes)
    rows = torch.from_numpy(gen.normal((G, R.KP), 7100))
    outs = [guarded((3,) + tuple(s), torch.float32, SENTINEL) for s in sizes]
    got = vt().hip.unpatchify_clips(poisoned(rows), sizes, 3, PT, P, out=[o for o, _ in outs])
    torch.cuda.synchronize()
    split = rows.split([(T // PT) * (H // P) * (W // P) for T, H, W in sizes], 0)
    for g, r, s, (_, tail) in zip(got, split, sizes, outs):
        assert torch.equal(g.cpu(), clip_of(r, s)) and untouched(tail), s
    fresh = vt().hip.unpatchify_clips(rows.cuda(), sizes, 3, PT, P)
    assert all(torch.equal(a, b) for a, b in zip(fresh, got))
    back = vt().hip.patchify_clips(fresh, PT, P)                        # the round trip, up to the bf16 rounding of the rows
    assert torch.equal(back.cpu(), rows.to(torch.bfloat16))


def test_patchify_clips_equals_vt_patchify_on_square_clips():
    hip = vt().hip
    sizes = [(4, 8, 8), (8, 16, 16), (4, 32, 32)]
    clips = [v.cuda() for v in clip_list(sizes, 7200)]
    got = hip.patchify_clips(clips, PT, P)
    want = torch.cat([hip.patchify(v.unsqueeze(0).contiguous(), PT, P) for v in clips], 0)
    assert torch.equal(got, want)
    rows = torch.from_numpy(gen.normal((got.shape[0], R.KP), 7300)).cuda()
    back = hip.unpatchify_clips(rows, sizes, 3, PT, P)
    r0 = 0
    for v, (T, S, _) in zip(back, sizes):
        g = (T // PT) * (S // P) ** 2
        assert torch.equal(v, hip.unpatchify(rows[r0:r0 + g].contiguous(), 1, 3, T, S, PT, P)[0])
        r0 += g


def _packed_case(name, D, seed):
    lead, lens = COUNTS[name]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    x = torch.from_numpy(gen.normal((cu[-1], D), seed))
    vec = torch.from_numpy(gen.normal((1, D), seed + 1))
    return lead, lens, cu, x, vec


def _segments(x, lead, lens, which):
    return [seq[:n] if which == 0 else seq[n:] for n, seq in zip(lead, x.split(lens, 0))]


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("name", sorted(COUNTS))
@pytest.mark.parametrize("which", [0, 1])
def test_scatter_equals_the_cat_construction(name, D, which):
    hip = vt().hip
    lead, lens, cu, x, vec = _packed_case(name, D, 7400)
    src = torch.cat(_segments(x, lead, lens, which), 0)                 # any compact rows of the right count
    for v in (vec, None):
        fill = vec if v is not None else torch.zeros(1, D)
        parts = []
        for n, L, rows in zip(lead, lens, src.split([n if which == 0 else L - n for n, L in zip(lead, lens)], 0)):
            other = fill.repeat(L - n if which == 0 else n, 1)            # blocks.py:133-134 (which = tail) and :198-199 (which = lead)
            parts.append(torch.cat([rows, other] if which == 0 else [other, rows], 0))
        want = torch.cat(parts, 0)
        out, tail = guarded((cu[-1], D), torch.float32, SENTINEL)
        got = hip.packed_scatter(poisoned(src), cu, lead, which, vec=poisoned(v) if v is not None else None, out=out)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want) and untouched(tail), (name, D, which, v is None)


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("name", sorted(COUNTS))
@pytest.mark.parametrize("which", [0, 1])
def test_gather_equals_split_slice_cat(name, D, which):
    hip = vt().hip
    lead, lens, cu, x, _ = _packed_case(name, D, 7500)
    want = torch.cat(_segments(x, lead, lens, which), 0)                # blocks.py:140-142 / :207-209
    out, tail = guarded(tuple(want.shape), torch.float32, SENTINEL)
    got = hip.packed_gather(poisoned(x), cu, lead, which, out=out)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and untouched(tail)
    back = hip.packed_scatter(got, cu, lead, which)                     # scatter with zeros = the gather's backward
    keep = torch.zeros(cu[-1], dtype=torch.bool)
    for a, n, L in zip(cu, lead, lens):
        keep[a:a + n] = True
    keep = keep if which == 0 else ~keep
    assert torch.equal(back.cpu(), x * keep.unsqueeze(1))


def _colsum_error(got, rows):
    """(|got - float64 sum|, the bound R * 2^-24 * sum |x_r|) per column"""
    r64 = rows.double()
    return (got.double() - r64.sum(0)).abs(), rows.shape[0] * 2.0 ** -24 * r64.abs().sum(0)


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("name", sorted(COUNTS))
@pytest.mark.parametrize("which", [0, 1])
def test_segment_colsum_within_the_fp32_summation_bound(name, D, which):
    hip = vt().hip
    lead, lens, cu, x, _ = _packed_case(name, D, 7600)
    xd = poisoned(x)
    out = hip.packed_segment_colsum(xd, cu, lead, which)
    again = hip.packed_segment_colsum(xd, cu, lead, which)
    torch.cuda.synchronize()
    assert torch.equal(out, again)                                      # a fixed order: two runs give equal bits
    err, bound = _colsum_error(out.cpu(), torch.cat(_segments(x, lead, lens, which), 0))
    print(f"COLSUM {name} D={D} which={which} max err/bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("which", [0, 1])
def test_segment_colsum_bound_is_live(which):
    """mutants of the expected rows: the other segment, and the chosen segment without the last sequence, both break the bound"""
    hip = vt().hip
    lead, lens, cu, x, _ = _packed_case("case", 128, 7600)
    out = hip.packed_segment_colsum(x.cuda(), cu, lead, which).cpu()
    right = _segments(x, lead, lens, which)
    for mutant in (torch.cat(_segments(x, lead, lens, 1 - which), 0), torch.cat(right[:-1], 0)):
        err, bound = _colsum_error(out, mutant)
        assert not bool((err <= bound).all())
    err, bound = _colsum_error(out, torch.cat(right, 0))
    assert bool((err <= bound).all())


def test_functions_route_gradients():
    """PackedScatter / PackedGather are each other's backward, plus the segment column sum for vec; exact against autograd on the CPU
    construction except the column sum, which is held to its bound"""
    F_ = vt().functional
    lead, lens, cu, x, vec = _packed_case("case", 128, 7700)
    w = torch.from_numpy(gen.normal((cu[-1], 128), 7702))
    src = torch.cat(_segments(x, lead, lens, 1), 0)
    s_d, v_d = src.cuda().requires_grad_(True), vec.cuda().requires_grad_(True)
    out = F_.PackedScatter.apply(s_d, v_d, cu, lead, 1)
    (out * w.cuda()).sum().backward()
    assert torch.equal(s_d.grad.cpu(), torch.cat(_segments(w, lead, lens, 1), 0)) and v_d.grad.shape == vec.shape
    err, bound = _colsum_error(v_d.grad.cpu().reshape(-1), torch.cat(_segments(w, lead, lens, 0), 0))
    assert bool((err <= bound).all())
    p_d = x.cuda().requires_grad_(True)
    g = F_.PackedGather.apply(p_d, cu, lead, 0)
    wl = torch.cat(_segments(w, lead, lens, 0), 0)
    (g * wl.cuda()).sum().backward()
    keep = torch.zeros(cu[-1], dtype=torch.bool)
    for a, n in zip(cu, lead):
        keep[a:a + n] = True
    assert torch.equal(p_d.grad.cpu(), w * keep.unsqueeze(1))
    clips = [v.cuda().requires_grad_(True) for v in clip_list(R.CLIP_SIZES, 7800)]
    rows = F_.PatchRowsClips.apply(PT, P, *clips)
    wr = torch.from_numpy(gen.normal(tuple(rows.shape), 7801))
    (rows.float() * wr.cuda()).sum().backward()
    for v, r, s in zip(clips, wr.split(R.grid_sizes(), 0), R.CLIP_SIZES):     # the gradient of bf16 rows arrives in bf16
        assert torch.equal(v.grad.cpu(), clip_of(r.to(torch.bfloat16).float(), s))
    rd = wr.cuda().requires_grad_(True)
    outs = F_.UnpatchifyClips.apply(rd, R.CLIP_SIZES, 3, PT, P)
    ws = clip_list(R.CLIP_SIZES, 7900)
    sum((o * v.cuda()).sum() for o, v in zip(outs, ws)).backward()
    assert torch.equal(rd.grad.cpu(), torch.cat([rows_of(v) for v in ws], 0).to(torch.bfloat16).float())
