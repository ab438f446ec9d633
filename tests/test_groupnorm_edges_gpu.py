"""vt_groupnorm_fwd / vt_groupnorm_bwd through the C ABI against the cases of tests/groupnorm_cases.py: every output under its derived bar, NaN
behind every operand, sentinels behind every output, a second call bit-identical.  tests/test_groupnorm_cases_cpu.py shows that these cases
catch a wrong kernel."""
import pytest
import torch

from tests import groupnorm_cases as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def operand(t):
    a = N.poisoned(t).cuda()
    return a, a[:t.numel()].view(t.shape)


@pytest.mark.parametrize("c", N.CASES, ids=lambda c: c.name)
def test_groupnorm_case(hip, c):
    d, q = N.inputs(c.name), N.bars(c.name)
    keep = {k: operand(v) for k, v in d.items()}
    x, dz, gamma, beta = (keep[k][1] for k in ("x", "dz", "gamma", "beta"))
    n = c.B * c.P * c.C

    def fwd():
        y, mean, rstd = N.out_alloc(n, torch.bfloat16).cuda(), N.out_alloc(c.B * c.G, torch.float32).cuda(), N.out_alloc(c.B * c.G, torch.float32).cuda()
        ws = torch.empty(hip.lib().vt_groupnorm_workspace_bytes(c.B, c.P, c.C, c.G), dtype=torch.uint8, device="cuda")
        hip.check(hip.lib().vt_groupnorm_fwd(hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), N.EPS, c.B, c.P, c.C, c.G, c.swish, hip.ptr(y), hip.ptr(mean),
                                             hip.ptr(rstd), hip.ptr(ws), hip.stream()), "vt_groupnorm_fwd")
        return dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu())

    sm, sr = (operand(t) for t in N.saved_stats(c, d))

    def bwd():
        dx, dg, db = N.out_alloc(n, torch.bfloat16).cuda(), N.out_alloc(c.C, torch.float32).cuda(), N.out_alloc(c.C, torch.float32).cuda()
        ws = torch.empty(hip.lib().vt_groupnorm_workspace_bytes(c.B, c.P, c.C, c.G), dtype=torch.uint8, device="cuda")
        hip.check(hip.lib().vt_groupnorm_bwd(hip.ptr(dz), hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(sm[1]), hip.ptr(sr[1]), c.B, c.P, c.C, c.G,
                                             c.swish, hip.ptr(dx), hip.ptr(dg), hip.ptr(db), hip.ptr(ws), hip.stream()), "vt_groupnorm_bwd")
        return dict(dx=dx.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())

    for run in (fwd, bwd):
        got, again = run(), run()
        for name, alloc in got.items():
            r = N.check(q[name], alloc, f"{c.name} {name}")
            print(f"{c.name} {name}: ratio {r if r is None else round(r, 3)}")
            N.assert_bits(again[name], alloc, f"{c.name} {name}: second call")
