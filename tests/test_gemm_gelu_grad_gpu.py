"""The two epilogues of vt_gemm_nt that move gelu' from the fc2 input-gradient GEMM into the fc1 forward:
VT_EPI_BF16_GELU_GRAD (out = bf16 gelu'(u), out2 = bf16 gelu(u), one evaluation) and VT_EPI_BF16_MULAUX (out = bf16(h * aux), with
the per-slab column sums), against the older GELU / DGELU pair, against fp64 and against exact restatements."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def _every_bf16_magnitude_cpu(M, K):
    """[M, K] bf16 on the CPU (tests/gated_cases.py builds its GEGLU gate half from it): every exponent from 2^-40 to 2^20 in both signs, zeros, the GELU table's edge patterns, rows that stay inside the table
    (the inputs of test_ops_gpu's GELU table test, restated)"""
    rng = np.random.default_rng(5)
    exps = rng.integers(-40, 21, size=(M, K))
    vals = np.ldexp(1.0 + rng.integers(0, 128, size=(M, K)) / 128.0, exps) * rng.choice([-1.0, 1.0], size=(M, K))
    vals[::7, ::5] = 0.0
    vals[1::7, ::5] = -0.0
    vals[0, :8] = [2.0 ** -16, -2.0 ** -16, 2.0 ** -17 * 1.9921875, 15.9375, -15.9375, 16.0, -16.0, 2.0 ** -16 * 1.0078125]   # the table's edges
    vals[2:6] = rng.normal(size=(4, K))          # rows that stay inside the table
    # (added to the restated inputs) the edges of the (gelu, gelu') pair table of the 192x192 kernel, |u| in [2^-12, 16)
    vals[6, :8] = [2.0 ** -12, -2.0 ** -12, 2.0 ** -13 * 1.9921875, -2.0 ** -13 * 1.9921875, 2.0 ** -12 * 1.0078125, 15.9375, 16.0, -16.0]
    return torch.from_numpy(vals.astype(np.float32)).to(torch.bfloat16)


def _every_bf16_magnitude(M, K):
    return _every_bf16_magnitude_cpu(M, K).cuda()


def _bits(t):
    return t.view(torch.int16)


def _rand_bf16(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [192, 196], ids=["16_byte_read_back", "8_byte_read_back"])
def test_gelu_grad_bits_on_every_bf16_magnitude(hip, N):
    """B = identity rows, so u is exactly A (N = 196: the last 4 columns of u are zero, and the 192x192 kernel reads its image back 8
    bytes per lane).  On the 128x128 and the 192x192 kernel: out2 carries the bits of EPI_BF16_GELU's g; out is the same on both kernels
    and carries the bits of the gelu' inside EPI_BF16_DGELU (an accumulator of exactly 1.0 times gelu'(aux)); and out is within one
    bf16 rounding plus the erf approximation's own error (Abramowitz-Stegun 7.1.26, 1.5e-7 on erf) of fp64 Phi(u) + u phi(u)."""
    M, K = 384, 192
    a = _every_bf16_magnitude(M, K)
    b = torch.eye(N, K, dtype=torch.bfloat16).cuda()
    u = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    u[:, :K] = a
    one_a = torch.zeros(M, 64, dtype=torch.bfloat16, device="cuda")
    one_b = torch.zeros(N, 64, dtype=torch.bfloat16, device="cuda")
    one_a[:, 0] = 1.0
    one_b[:, 0] = 1.0
    outs = {}
    for tile in (1, 2):
        u_old, g_old = hip.gemm_nt(a, b, epi=hip.EPI_BF16_GELU, tile=tile, splitk=1)
        dg, g = hip.gemm_nt(a, b, epi=hip.EPI_BF16_GELU_GRAD, tile=tile, splitk=1)
        dg_old = hip.gemm_nt(one_a, one_b, epi=hip.EPI_BF16_DGELU, aux=u, tile=tile, splitk=1)
        torch.cuda.synchronize()
        assert torch.equal(u_old, u)
        assert torch.equal(_bits(g), _bits(g_old)), tile
        assert torch.equal(_bits(dg), _bits(dg_old)), tile
        outs[tile] = dg
    assert torch.equal(_bits(outs[1]), _bits(outs[2]))
    x = u.double()
    ref = 0.5 * (1.0 + torch.erf(x / np.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
    err = (outs[2].double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 4e-7 * x.abs().clamp(min=1.0)
    print(f"gelu' against fp64: worst err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


MULAUX_SHAPES = [(384, 384, 128), (200, 196, 128), (100, 64, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [1, 2, 6], ids=["tile128", "tile192", "tile192_one_tile_per_wg"])
@pytest.mark.parametrize("M,N,K", MULAUX_SHAPES)
def test_mulaux_is_an_exact_restatement(hip, M, N, K, tile):
    """out = bf16(h * aux) with h what EPI_BF16 writes: the fp32 product of two bf16 values is exact, so the restatement in torch is
    equal bit for bit.  colsum_partial does not change out, fills every slab row (no NaN left) and holds the column sums of the rounded
    output.  The column sums are checked on non-negative operands: their fp32 sum over 192 rows (about 30 additions deep) is then within
    30 * 2^-24 = 1.8e-6 of the sum itself, inside the rtol of 1e-5; with signed operands a sum that cancels to near zero has no such
    relative bound in fp32 whatever the kernel does."""
    for sign_free in (True, False):
        A, B, aux = _rand_bf16((M, K), 11, 0.5), _rand_bf16((N, K), 12, 0.5), _rand_bf16((M, N), 13)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(14)).cuda()
        if not sign_free:
            A, B, aux, bias = A.abs(), B.abs(), aux.abs(), bias.abs()
        h = hip.gemm_nt(A, B, epi=hip.EPI_BF16, bias=bias, tile=tile, splitk=1)
        out = hip.gemm_nt(A, B, epi=hip.EPI_BF16_MULAUX, bias=bias, aux=aux, tile=tile, splitk=1)
        slabs = (M + 191) // 192
        part = torch.full((slabs, N), float("nan"), device="cuda")
        out_cs = hip.gemm_nt(A, B, epi=hip.EPI_BF16_MULAUX, bias=bias, aux=aux, colsum_partial=part, tile=tile, splitk=1)
        torch.cuda.synchronize()
        assert torch.equal(out, (h.float() * aux.float()).to(torch.bfloat16))
        assert torch.equal(_bits(out_cs), _bits(out))
        assert not torch.isnan(part).any()
        if not sign_free:
            want = torch.stack([out[t * 192:(t + 1) * 192].double().sum(0) for t in range(slabs)])
            np.testing.assert_allclose(part.double().cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=0)


# N, ldo, ldo2 and the read-back width of the 192x192 kernel that they select (16 bytes per lane needs N, ldo and -- where there is an
# out2 -- ldo2 to be multiples of 8; each of the three alone sends the launch to 8 bytes per lane)
READ_BACK_CASES = [(192, 192, 192, "16 bytes"), (196, 196, 196, "8 bytes through N"), (192, 196, 192, "8 bytes through ldo"),
                   (192, 192, 196, "8 bytes through ldo2")]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [64, 256], ids=["one_k_tile", "four_k_tiles_ring_wraps"])
@pytest.mark.parametrize("M", [192, 200])
def test_read_back_width_dispatch_of_the_192_tile_kernel(hip, M, K):
    """The 192x192 kernel reads its staged bf16 image back 16 or 8 bytes per lane, chosen per launch from N, ldo and ldo2.  For every
    epilogue that takes this read-back, persistent (tile 2) and one tile per workgroup (tile 6): each output equals the 128x128 kernel's
    (tile 1) on the same operands -- the same summation order and the same per-element arithmetic, so bit for bit, no tolerance -- and
    every element of the destination buffers outside [0, M) x [0, N) still holds the bit pattern the buffer was filled with (the
    buffers are two tiles of rows deep, so a store past M or N would land in them).
    What this does not see: WHICH width a launch took (the hardware accepts a 16-byte store at an 8-byte-aligned address, and the 8-byte
    walk is right for every launch), and the per-element arithmetic on its own (tile 1 calls the same epi_values; the other tests of
    this file hold it to fp64 and to exact restatements).  Checked here, independently of tile 1: the walk over the staged image and the
    stores, in both widths' code, at the shapes that select each."""
    sentinel = 0x7FC5                                   # a NaN no kernel produces
    depth = 392

    def buffer(ld):
        b = torch.empty(depth, ld, dtype=torch.bfloat16, device="cuda")
        _bits(b).fill_(sentinel)
        return b

    for N, ldo, ldo2, what in READ_BACK_CASES:
        A, B, aux = _rand_bf16((M, K), 41, 0.5), _rand_bf16((N, K), 42, 0.5), _rand_bf16((M, N), 43)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(44)).cuda()
        for epi in (hip.EPI_BF16, hip.EPI_BF16_GELU, hip.EPI_BF16_GELU_GRAD, hip.EPI_BF16_MULAUX):
            two = epi in (hip.EPI_BF16_GELU, hip.EPI_BF16_GELU_GRAD)
            if what.endswith("ldo2") and not two:
                continue                                # no out2: the same launch as the first case

            def run(tile):
                bufs = [buffer(ldo)] + ([buffer(ldo2)] if two else [])
                hip.gemm_nt(A, B, epi=epi, bias=bias, aux=aux if epi == hip.EPI_BF16_MULAUX else None, out=bufs[0][:M, :N],
                            out2=bufs[1][:M, :N] if two else None, tile=tile, splitk=1)
                return bufs

            want = run(1)
            for tile in (2, 6):
                got = run(tile)
                torch.cuda.synchronize()
                for g, w in zip(got, want):
                    where = (what, epi, tile, M, K)
                    assert torch.equal(g[:M, :N], w[:M, :N]), where
                    assert torch.equal(_bits(g)[:M, :N], _bits(w)[:M, :N]), where
                    assert bool((_bits(g)[M:] == sentinel).all()) and bool((_bits(g)[:M, N:] == sentinel).all()), where


@pytest.mark.gpu
def test_new_epilogues_on_the_other_dispatch_paths(hip):
    """The 4-deep ring and split K of the 128x128 kernel, the M <= 64 weight-streaming kernel and the scalar tail of N % 4 != 0 run
    the same epilogues: MULAUX restates EPI_BF16 of the same path exactly, GELU_GRAD carries the bits of the 128x128 kernel's."""
    for (M, N, K), kw in [((200, 196, 256), dict(tile=16, splitk=1)), ((200, 196, 256), dict(tile=1, splitk=2)),
                          ((40, 196, 128), dict(tile=7, splitk=1)), ((200, 198, 128), dict(tile=1, splitk=1)),
                          ((200, 198, 128), dict(tile=2, splitk=1))]:
        A, B = _rand_bf16((M, K), 21, 0.5), _rand_bf16((N, K), 22, 0.5)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(24)).cuda()

        def rows():     # [M, N] bf16 with a row stride that is a multiple of 4 elements, as the C ABI asks
            return torch.zeros(M, (N + 3) // 4 * 4, dtype=torch.bfloat16, device="cuda")[:, :N]
        aux = rows()
        aux.copy_(_rand_bf16((M, N), 23))
        h = hip.gemm_nt(A, B, epi=hip.EPI_BF16, bias=bias, out=rows(), **kw)
        out = hip.gemm_nt(A, B, epi=hip.EPI_BF16_MULAUX, bias=bias, aux=aux, out=rows(), **kw)
        u, g = hip.gemm_nt(A, B, epi=hip.EPI_BF16_GELU, bias=bias, out=rows(), out2=rows(), **kw)
        dg, g2 = hip.gemm_nt(A, B, epi=hip.EPI_BF16_GELU_GRAD, bias=bias, out=rows(), out2=rows(), **kw)
        one_a = torch.zeros(M, 64, dtype=torch.bfloat16, device="cuda")
        one_b = torch.zeros(N, 64, dtype=torch.bfloat16, device="cuda")
        one_a[:, 0] = 1.0
        one_b[:, 0] = 1.0
        dg_ref = hip.gemm_nt(one_a, one_b, epi=hip.EPI_BF16_DGELU, aux=u, out=rows(), tile=1, splitk=1)
        torch.cuda.synchronize()
        assert torch.equal(u, h), kw
        assert torch.equal(out, (h.float() * aux.float()).to(torch.bfloat16)), kw
        assert torch.equal(g2, g) and not torch.isnan(g.float()).any(), kw     # (no NaN among these inputs: value equality is bit equality up to the sign of zero)
        assert torch.equal(_bits(g2.contiguous()), _bits(g.contiguous())), kw
        assert torch.equal(_bits(dg.contiguous()), _bits(dg_ref.contiguous())), kw


@pytest.mark.gpu
def test_chain_against_the_old_pair(hip):
    """fc1 forward then fc2 input gradient, old pair (GELU -> DGELU) against new pair (GELU_GRAD -> MULAUX) on the same operands: the
    new chain rounds gelu'(u) to bf16 before the product, so the results differ by at most that one rounding (2^-8 relative) carried
    through the final rounding: 2^-7 |old|.  Where the fp32 gelu'(u) is exactly representable in bf16 they are equal: u >= 8 (1 - 6e-16 and
    the pdf term 4e-14 both vanish against 1.0f) and u <= -16 (exp(-u^2 / 2) underflows fp32, so both terms are 0).  For -16 < u <= -8 the
    fp32 gelu'(u) is a tiny NON-zero number (-4e-14 at u = -8) that bf16 rounds like any other, so those elements are held to the bound only."""
    M, N, K = 384, 384, 128
    X, W1 = _rand_bf16((M, K), 31, 1.5), _rand_bf16((N, K), 32, 0.5)
    b1 = (torch.randn(N, generator=torch.Generator().manual_seed(33)) * 2.0).cuda()
    dY, W2t = _rand_bf16((M, K), 34, 0.5), _rand_bf16((N, K), 35, 0.5)
    outs = {}
    for tile in (1, 2):
        u, g = hip.gemm_nt(X, W1, epi=hip.EPI_BF16_GELU, bias=b1, tile=tile, splitk=1)
        dg, g2 = hip.gemm_nt(X, W1, epi=hip.EPI_BF16_GELU_GRAD, bias=b1, tile=tile, splitk=1)
        old = hip.gemm_nt(dY, W2t, epi=hip.EPI_BF16_DGELU, aux=u, tile=tile, splitk=1)
        new = hip.gemm_nt(dY, W2t, epi=hip.EPI_BF16_MULAUX, aux=dg, tile=tile, splitk=1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g2), _bits(g))
        diff = (new.double() - old.double()).abs()
        assert (diff <= 2.0 ** -7 * old.double().abs() + 1e-30).all(), float((diff / old.double().abs().clamp(min=1e-30)).max())
        exact = (u.float() >= 8.0) | (u.float() <= -16.0)
        assert int((u.float() >= 8.0).sum()) > 100 and int((u.float() <= -16.0).sum()) > 100
        assert torch.equal(_bits(new)[exact], _bits(old)[exact])
        outs[tile] = new
    assert torch.equal(_bits(outs[1]), _bits(outs[2]))


def test_host_side_validation_of_the_new_epilogues():
    """Argument validation runs on the host before any launch (no GPU needed): GELU_GRAD without out2 and MULAUX without aux are
    refused with a message that names the field, and colsum_partial is still refused with the plain bf16 epilogue."""
    import video_tokenizer_amd.hip as h
    lib = h.lib()
    buf = ctypes.create_string_buffer(512)

    def call(**fields):
        p = h.GemmNT()
        p.A = p.B = p.out = 4096                   # non-null, 16-byte aligned, never dereferenced
        p.M, p.N, p.K, p.lda, p.ldb, p.ldo = 192, 192, 64, 64, 64, 192
        p.splitk = 1
        for k, v in fields.items():
            setattr(p, k, v)
        rc = lib.vt_gemm_nt(ctypes.byref(p), None)
        lib.vt_last_error(buf, 512)
        return rc, buf.value

    rc, msg = call(epi=h.EPI_BF16_GELU_GRAD)
    assert rc == -1 and b"out2" in msg, msg
    rc, msg = call(epi=h.EPI_BF16_MULAUX)
    assert rc == -1 and b"aux" in msg, msg
    rc, msg = call(epi=h.EPI_BF16, colsum_partial=4096)
    assert rc == -1 and b"colsum_partial" in msg, msg
    rc, msg = call(epi=h.EPI_BF16_GELU, colsum_partial=4096, out2=4096, ldo2=192)
    assert rc == -1 and b"colsum_partial" in msg, msg
