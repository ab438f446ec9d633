"""vt_gemm_nt, vt_gemm_tn_grouped and vt_decode_norm_linear against the cases of tests/gemm_cases.py: exact integer data compared by bits
on every kernel path (tile 1 / 16 / 2 / 6 / 7 / auto, forced split-K), transcendental epilogues against float64 under an analytic bar,
NaN behind every operand, NaN sentinels around every output.  tests/test_gemm_cases_cpu.py shows that these cases catch a wrong kernel."""
import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def dev(buf):
    """(allocation on the GPU, the operand: its leading rows x cols)"""
    alloc, r, k = buf
    a = alloc.cuda()
    return a, (a[:k] if a.dim() == 1 else a[:r, :k])


class NTRun:
    """a case's operands on the GPU, uploaded once; call(tile, splitk) runs one kernel path into fresh sentinel outputs"""

    def __init__(self, hip, c):
        self.hip, self.c = hip, c
        b = G.nt_buffers(c.name)
        self.outs = {k: b.pop(k) for k in ("out", "out2", "colsum") if k in b}
        self.ins = {k: dev(v) for k, v in b.items()}

    def call(self, tile, splitk=1, **over):
        hip, c = self.hip, self.c
        outs = {k: dev(v) for k, v in self.outs.items()}
        view = lambda d, k: d[k][1] if k in d else None
        kw = dict(epi=c.epi, bias=view(self.ins, "bias"), out=view(outs, "out"), out2=view(outs, "out2"), residual=view(self.ins, "residual"),
                  rowmod=view(self.ins, "rowmod"), rowmod_period=c.rowmod, aux=view(self.ins, "aux"), omap=hip.RowMap(*c.omap) if c.omap else None,
                  round_bf16=c.round_bf16, colsum_partial=view(outs, "colsum"), tile=tile, out_scale=c.out_scale, splitk=splitk)
        kw.update(over)
        try:
            hip.gemm_nt(kw.pop("A", self.ins["A"][1]), self.ins["B"][1], **kw)
        finally:
            torch.cuda.synchronize()
            self.got = {k: v[0].cpu() for k, v in outs.items()}
        return self.got


@pytest.mark.parametrize("c", G.NT_CASES + G.GELU_CASES, ids=lambda c: c.name)
def test_gemm_nt_case_on_every_path(hip, c):
    ref = G.nt_reference(c)
    run = NTRun(hip, c)
    for tile, splitk in G.nt_paths(c):
        G.check_nt(c, ref, run.call(tile, splitk), f"{c.name} tile {tile} splitk {splitk}")


def test_gemm_nt_refusals_leave_the_output_untouched(hip):
    def refused(c, tile=1, **over):
        run = NTRun(hip, c)
        with pytest.raises(hip.HipError):
            run.call(tile, **over)
        for name, a in run.got.items():
            G.assert_bits(a, G.sentinel(a.shape, a.dtype), f"{c.name} refused, {name}")

    bf, f32 = G.NT_BY_NAME["bf16_129x196x448"], G.NT_BY_NAME["f32_map40_129x130x64"]
    for tile in (1, 2):
        refused(bf, tile, out_scale=0.5)                                                    # out_scale with a bf16 epilogue
        refused(bf, tile, omap=hip.RowMap(40, 48, 0))                                       # a row map on a bf16 epilogue
        A = NTRun(hip, bf).ins["A"][0]
        refused(bf, tile, A=A.as_strided((bf.M, bf.K), (bf.K - 8, 1)))                      # lda < K
        o = G.sentinel((f32.M + 50, f32.N + 4), torch.float32).cuda()                       # ldo = 134
        with pytest.raises(hip.HipError):
            run = NTRun(hip, f32)
            run.call(tile, out=o[: G.out_rows_of(f32)[1], : f32.N])
        G.assert_bits(o.cpu(), G.sentinel(o.shape, o.dtype), "ldo % 4 != 0 refused")
        G.assert_bits(run.got["out2"], G.sentinel(run.got["out2"].shape, torch.bfloat16), "ldo % 4 != 0 refused, out2")
    refused(G.NT_BY_NAME["bf16_65x130x256"], 7)                                             # the skinny kernel with M = 65


@pytest.mark.parametrize("tile,splitk,family", G.RANDOM_PATHS, ids=[f"tile{t}_splitk{s}_{f}" for t, s, f in G.RANDOM_PATHS])
def test_gemm_nt_random_operands_against_float64(hip, tile, splitk, family):
    for M, N, K in G.RANDOM_SHAPES[family]:
        for std in G.RANDOM_STDS:
            r = G.random_case(M, N, K, std)
            A, B = r["A"].cuda(), r["B"].cuda()
            for epi, bound in ((hip.EPI_F32, r["bound32"]), (hip.EPI_BF16, r["bound16"])):
                o = torch.empty(M, G.ceil4(N), device="cuda", dtype=torch.float32 if epi == hip.EPI_F32 else torch.bfloat16)[:, :N]
                out = hip.gemm_nt(A, B, epi, out=o, tile=tile, splitk=splitk).double().cpu()
                err = (out - r["ref"]).abs()
                ok = err <= bound
                assert bool(ok.all()), (M, N, K, std, epi, int((~ok).sum()), float((err / bound).nan_to_num(1e30).max()))


# ------------------------------------------------------------------------------------------------ TN
def tn_problem(c, tile):
    b = G.tn_buffers(c.name)
    d = G.tn_inputs(c.name)
    pl, ql, ldo, orows = G.tn_dims(c)
    out = dev(b["out"])
    pr = dict(A=dev(b["A"])[1], B=dev(b["B"])[1], out=out[1], p_lim=pl, q_lim=ql, tile=tile)
    if c.perm:
        pr["row_perm"] = d["perm"].cuda()
    return pr, out[0]


@pytest.mark.parametrize("tile", G.TN_TILES)
@pytest.mark.parametrize("c", G.TN_CASES, ids=lambda c: c.name)
def test_gemm_tn_case(hip, c, tile):
    pr, alloc = tn_problem(c, tile)
    hip.gemm_tn_grouped([pr])
    torch.cuda.synchronize()
    G.assert_bits(alloc.cpu(), G.tn_reference(c), f"{c.name} tile {tile}")


@pytest.mark.parametrize("tile", G.TN_TILES)
@pytest.mark.parametrize("order", ["largest_first", "smallest_first"])
def test_gemm_tn_four_problems_in_one_launch(hip, order, tile):
    cases = G.TN_GROUP if order == "largest_first" else G.TN_GROUP[::-1]
    prs = [tn_problem(c, tile) for c in cases]
    hip.gemm_tn_grouped([p for p, _ in prs])
    torch.cuda.synchronize()
    for c, (_, alloc) in zip(cases, prs):
        G.assert_bits(alloc.cpu(), G.tn_reference(c), f"{c.name} in a group of four ({order}), tile {tile}")


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("c", G.DECODE_CASES, ids=lambda c: c.name)
def test_decode_norm_linear_case(hip, c):
    b = G.decode_buffers(c.name)
    x, W, out = dev(b["x"]), dev(b["W"]), dev(b["out"])
    nw = dev(b["norm_w"])[1] if c.norm else None
    # x and W are contiguous [M, K] / [N, K] operands: the rows behind them (NaN) belong to the same allocation
    hip.decode_norm_linear(x[1], nw, G.DECODE_EPS if c.norm else 0.0, W[1], mode=c.mode, out=out[1])
    torch.cuda.synchronize()
    exp, bar = G.decode_reference(c)
    G.check_output(out[0].cpu(), torch.arange(c.M), exp.shape[1], exp, bar, c.name)
