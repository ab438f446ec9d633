"""The weight packer of csrc/vt_pack.hip (vt_pack_weight, vt_pack_weights_grouped) at its edges: extents below, at and above the 32- and
64-element tile edges, a row permutation, either output alone, leading dimensions beyond the extent, and a source that is not 16-byte
aligned (which sends its launch from the 64x64 kernel to the 32x32 one).  The pack is a cast and a transpose, so every case is compared
for exact equality with `w[perm].to(torch.bfloat16)` and its transpose from torch on the CPU.  Every destination is allocated one row
and `pad` columns larger than what the job may write and filled with a sentinel, which must survive everywhere outside the packed block."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
EXTENTS = (1, 31, 32, 33, 63, 64, 65, 100)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


class Job:
    """one pack job: its source on the GPU, its sentinel-filled destinations, and the check of what a launch left in them"""

    def __init__(self, N, K, seed, perm=False, want_b=True, want_t=True, pad=0, offset=0):
        g = torch.Generator().manual_seed(seed)
        self.N, self.K, self.pad = N, K, pad
        self.buf = torch.randn(N * K + offset, generator=g).cuda()
        self.w = self.buf[offset:].view(N, K)                      # offset = 1: 4-byte aligned only
        self.perm = torch.randperm(N, generator=g).to(torch.int32).cuda() if perm else None
        self.wb = torch.full((N + 1, K + pad), SENTINEL, dtype=torch.bfloat16, device="cuda") if want_b else None
        self.wt = torch.full((K + 1, N + pad), SENTINEL, dtype=torch.bfloat16, device="cuda") if want_t else None

    def fill(self, j):
        p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        j.w, j.N, j.K, j.row_perm = p(self.w), self.N, self.K, p(self.perm)
        j.wb, j.ldd, j.wt, j.lddT = p(self.wb), self.K + self.pad, p(self.wt), self.N + self.pad

    def check(self):
        src = self.w.cpu()
        if self.perm is not None:
            src = src[self.perm.cpu().long()]
        for got, want in ((self.wb, src.to(torch.bfloat16)), (self.wt, src.t().to(torch.bfloat16))):
            if got is None:
                continue
            got, (r, c) = got.cpu(), want.shape
            assert torch.equal(got[:r, :c], want), (self.N, self.K)
            assert bool((got[r:] == SENTINEL).all()) and bool((got[:, c:] == SENTINEL).all()), (self.N, self.K)


def pack_single(hip, job):
    j = hip.PackJob()
    job.fill(j)
    hip.check(hip.lib().vt_pack_weight(j.w, j.N, j.K, j.row_perm, j.wb, j.ldd, j.wt, j.lddT, hip.stream()), "vt_pack_weight")


def pack_grouped(hip, jobs):
    arr = (hip.PackJob * len(jobs))()
    for j, job in zip(arr, jobs):
        job.fill(j)
    hip.check(hip.lib().vt_pack_weights_grouped(arr, len(jobs), hip.stream()), "vt_pack_weights_grouped")


def run(hip, jobs, grouped):
    if grouped:
        pack_grouped(hip, jobs)
    else:
        for job in jobs:
            pack_single(hip, job)
    torch.cuda.synchronize()
    for job in jobs:
        job.check()


@pytest.mark.parametrize("N", EXTENTS)
def test_pack_weight_at_every_extent(hip, N):
    """one launch per K; N and K both multiples of 4 take the 64x64 tiles (part tiles at 32 and 100), every other pair the 32x32 ones"""
    run(hip, [Job(N, K, 100 * N + K) for K in EXTENTS], grouped=False)


def test_pack_weights_grouped_mixed_extents(hip):
    """all 64 (N, K) pairs in one call: two launches of 32 jobs, each mixed, so on 32x32 tiles"""
    run(hip, [Job(N, K, 100 * N + K) for N, K in itertools.product(EXTENTS, EXTENTS)], grouped=True)


def test_pack_weights_grouped_extents_of_the_64_tile_kernel(hip):
    """the nine pairs with N and K multiples of 4, padded by 8: one launch on 64x64 tiles, half tiles at 32 and ragged ones at 100"""
    run(hip, [Job(N, K, 100 * N + K, pad=8) for N, K in itertools.product((32, 64, 100), repeat=2)], grouped=True)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [64, 65])                 # 64x64 tiles / 32x32 tiles
def test_pack_row_perm_one_output_and_padding(hip, K, grouped):
    """a row permutation, wb only, wt only, and leading dimensions beyond the extent (by 8, and by 3 where the tiles are 32x32 anyway)"""
    pad = 8 if K % 4 == 0 else 3
    run(hip, [Job(100, K, 1, perm=True), Job(100, K, 2, perm=True, pad=pad), Job(100, K, 3, want_t=False, pad=pad),
              Job(100, K, 4, want_b=False, pad=pad), Job(64, K, 5, perm=True, want_b=False), Job(33 if K % 4 else 32, K, 6, want_t=False)],
        grouped=grouped)


@pytest.mark.parametrize("grouped", [False, True])
def test_pack_source_one_element_into_its_buffer(hip, grouped):
    """aligned extents, but the second source starts one fp32 element into its buffer: it cannot be read 16 bytes at a time, so its
    launch (grouped: the whole group) takes the 32x32 tiles"""
    run(hip, [Job(64, 64, 11, pad=8), Job(64, 64, 12, offset=1, pad=8), Job(100, 32, 13, perm=True, offset=1), Job(32, 100, 14)], grouped=grouped)
