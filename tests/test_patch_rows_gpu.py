"""vt_patchify / vt_unpatchify (csrc/vt_patch.hip, the one-segment case of its kernel) on the GPU at the edges of their index arithmetic.
The kernels only move data (patchify rounds once to bf16), so equality is exact: against an einops.rearrange restatement of Conv3d patch
extraction (kernel = stride = (pt, p, p), weight flattening (c, dt, dy, dx), token order (t, h, w)) and against their own inverse.

Every output lies in a buffer with sentinel-filled slack behind it, which must stay untouched; every input has NaN poison behind it, which
must not be read (a read would show in the exact comparisons).  The grid covers the lanes exactly (no cap, no stride loop), so no shape
beyond a cap exists."""
import pytest
import torch

from oracle import inputs as gen
from tests.test_dualpatch_rows_gpu import guarded, poisoned, rows_of, untouched, video_of, vt, SENTINEL

pytestmark = pytest.mark.gpu

SHAPES = {                                     # (B, C, T, S, pt, p)
    "48 lanes, one partly filled block, W/8 = 1": (1, 3, 2, 8, 2, 8),
    "W/8 odd": (2, 3, 4, 24, 2, 8),
    "pt = 1, p = 16: two lanes per patch row": (2, 2, 3, 32, 1, 16),
    "C = 1, T = pt": (3, 1, 4, 16, 4, 8),
}


def row_shape(s):
    B, C, T, S, pt, p = s
    return B * (T // pt) * (S // p) ** 2, C * pt * p * p


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_patchify_equals_the_conv3d_patch_extraction(which):
    s = SHAPES[which]
    B, C, T, S, pt, p = s
    v = torch.from_numpy(gen.normal((B, C, T, S, S), 9500))
    want = rows_of(v, pt, p, p).to(torch.bfloat16)
    assert tuple(want.shape) == row_shape(s)
    out, tail = guarded(row_shape(s), torch.bfloat16, SENTINEL)
    got = vt().hip.patchify(poisoned(v), pt, p, rows=out)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and untouched(tail)
    assert torch.equal(vt().hip.patchify(v.cuda(), pt, p).cpu(), want)                        # the wrapper's own allocation


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_unpatchify_inverts_exactly_and_writes_every_element_once(which):
    s = SHAPES[which]
    B, C, T, S, pt, p = s
    r = torch.from_numpy(gen.normal(row_shape(s), 9600))
    want = video_of(r, B, C, T, S, S, pt, p, p)
    out, tail = guarded((B, C, T, S, S), torch.float32, SENTINEL)
    got = vt().hip.unpatchify(poisoned(r), B, C, T, S, pt, p, video=out)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and untouched(tail)              # no sentinel is left inside: every element was written
    assert torch.equal(vt().hip.unpatchify(r.cuda(), B, C, T, S, pt, p).cpu(), want)


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_round_trip_is_the_video_rounded_to_bf16(which):
    s = SHAPES[which]
    B, C, T, S, pt, p = s
    v = torch.from_numpy(gen.normal((B, C, T, S, S), 9700)).cuda()
    back = vt().hip.unpatchify(vt().hip.patchify(v, pt, p).float(), B, C, T, S, pt, p)
    assert torch.equal(back, v.to(torch.bfloat16).float())
