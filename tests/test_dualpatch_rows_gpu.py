"""vt_patchify_dual / vt_unpatchify_dual (csrc/vt_patch.hip) on the GPU.  The kernels only move data (patchify rounds once to bf16), so
equality is exact: against an einops.rearrange restatement of Conv3d patch extraction per temporal segment (kernel = stride = (pt, ph, pw),
weight flattening (c, dt, dy, dx), token order (t, h, w)), against vt_patchify / vt_unpatchify on contiguous slices of square clips, and
against their own inverse.

Every output lies in a buffer with sentinel-filled slack behind it, which must stay untouched; every input has NaN poison behind it, which
must not be read (a read would show in the exact comparisons).  The kernels' grid covers the lanes exactly (no cap), so no shape beyond a
cap exists; the shapes are the edges of the index arithmetic: W / 8 odd, non-square, 16 lanes in all, ph != pw, pt0 > 1, T0 = 2 pt0, pw = 16."""
import math

import pytest
import torch

from oracle import inputs as gen

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SLACK = 1024                                   # elements behind every buffer
SHAPES = {                                     # (B, C, T, H, W; T0, pt0, pt1, ph, pw)
    "W/8 odd, non-square": (2, 3, 7, 16, 24, 1, 1, 3, 8, 8),
    "16 lanes": (1, 1, 2, 8, 8, 1, 1, 1, 8, 8),
    "ph != pw, pt0 > 1": (2, 3, 6, 32, 16, 2, 2, 2, 16, 8),
    "T0 = 2 pt0, pw = 16": (3, 2, 8, 16, 16, 4, 2, 4, 8, 16),
}
SQUARE = {
    "one frame, then threes": (2, 3, 7, 16, 16, 1, 1, 3, 8, 8),
    "T0 = 2 pt0": (3, 2, 8, 16, 16, 4, 2, 4, 8, 8),
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


def rows_of(seg, pt, ph, pw):
    from einops import rearrange
    return rearrange(seg, "b c (nt pt) (nh ph) (nw pw) -> (b nt nh nw) (c pt ph pw)", pt=pt, ph=ph, pw=pw)


def video_of(rows, B, C, T, H, W, pt, ph, pw):
    from einops import rearrange
    return rearrange(rows, "(b nt nh nw) (c pt ph pw) -> b c (nt pt) (nh ph) (nw pw)", b=B, nt=T // pt, nh=H // ph, nw=W // pw, c=C, pt=pt, ph=ph, pw=pw)


def row_shapes(s):
    B, C, T, H, W, T0, pt0, pt1, ph, pw = s
    n0, n1 = vt().hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)
    return (B * n0, C * pt0 * ph * pw), (B * n1, C * pt1 * ph * pw)


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_patchify_dual_equals_the_conv3d_patch_extraction(which):
    s = SHAPES[which]
    B, C, T, H, W, T0, pt0, pt1, ph, pw = s
    v = torch.from_numpy(gen.normal((B, C, T, H, W), 9000))
    want0, want1 = rows_of(v[:, :, :T0], pt0, ph, pw).to(torch.bfloat16), rows_of(v[:, :, T0:], pt1, ph, pw).to(torch.bfloat16)
    assert (tuple(want0.shape), tuple(want1.shape)) == row_shapes(s)
    (o0, tail0), (o1, tail1) = (guarded(sh, torch.bfloat16, SENTINEL) for sh in row_shapes(s))
    got0, got1 = vt().hip.patchify_dual(poisoned(v), T0, pt0, pt1, ph, pw, rows0=o0, rows1=o1)
    torch.cuda.synchronize()
    assert torch.equal(got0.cpu(), want0) and torch.equal(got1.cpu(), want1) and untouched(tail0) and untouched(tail1)
    fresh0, fresh1 = vt().hip.patchify_dual(v.cuda(), T0, pt0, pt1, ph, pw)                  # the wrapper's own allocation
    assert torch.equal(fresh0.cpu(), want0) and torch.equal(fresh1.cpu(), want1)


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_unpatchify_dual_inverts_exactly_and_writes_every_element_once(which):
    s = SHAPES[which]
    B, C, T, H, W, T0, pt0, pt1, ph, pw = s
    sh0, sh1 = row_shapes(s)
    r0, r1 = torch.from_numpy(gen.normal(sh0, 9100)), torch.from_numpy(gen.normal(sh1, 9101))
    want = torch.cat([video_of(r0, B, C, T0, H, W, pt0, ph, pw), video_of(r1, B, C, T - T0, H, W, pt1, ph, pw)], dim=2)
    out, tail = guarded((B, C, T, H, W), torch.float32, SENTINEL)
    got = vt().hip.unpatchify_dual(poisoned(r0), poisoned(r1), *s, video=out)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and untouched(tail)              # no sentinel is left inside: every element was written
    assert torch.equal(vt().hip.unpatchify_dual(r0.cuda(), r1.cuda(), *s).cpu(), want)


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_round_trip_is_the_video_rounded_to_bf16(which):
    s = SHAPES[which]
    B, C, T, H, W, T0, pt0, pt1, ph, pw = s
    v = torch.from_numpy(gen.normal((B, C, T, H, W), 9200)).cuda()
    r0, r1 = vt().hip.patchify_dual(v, T0, pt0, pt1, ph, pw)
    back = vt().hip.unpatchify_dual(r0.float(), r1.float(), *s)
    assert torch.equal(back, v.to(torch.bfloat16).float())


@pytest.mark.parametrize("which", sorted(SQUARE))
def test_square_clips_equal_the_one_segment_kernels_on_contiguous_slices(which):
    hip = vt().hip
    s = SQUARE[which]
    B, C, T, S, _, T0, pt0, pt1, p, _ = s
    v = torch.from_numpy(gen.normal((B, C, T, S, S), 9300)).cuda()
    got0, got1 = hip.patchify_dual(v, T0, pt0, pt1, p, p)
    assert torch.equal(got0, hip.patchify(v[:, :, :T0].contiguous(), pt0, p)) and torch.equal(got1, hip.patchify(v[:, :, T0:].contiguous(), pt1, p))
    sh0, sh1 = row_shapes(s)
    r0, r1 = torch.from_numpy(gen.normal(sh0, 9400)).cuda(), torch.from_numpy(gen.normal(sh1, 9401)).cuda()
    want = torch.cat([hip.unpatchify(r0, B, C, T0, S, pt0, p), hip.unpatchify(r1, B, C, T - T0, S, pt1, p)], dim=2)
    assert torch.equal(hip.unpatchify_dual(r0, r1, *s), want)
