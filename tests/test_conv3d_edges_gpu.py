"""vt_conv3d_fwd, vt_conv3d_dgrad and vt_conv3d_wgrad (with vt_conv3d_pack_weight in front) against the cases of tests/conv3d_cases.py: exact
integer data compared by bits, random data against float64 under the analytic bar, NaN behind every operand, sentinels behind every output,
a second call bit-identical.  Then the upsample pair and the layout pair by bits against F.interpolate / permute.
tests/test_conv3d_cases_cpu.py shows that these cases catch a wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv3d_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def operand(t, shape):
    """a bf16 / fp32 operand on the GPU as the head of a NaN-tailed allocation"""
    a = K.poisoned(t).cuda()
    return a, a[:t.numel()].view(shape)


class Run:
    """the operands of one case on the GPU, in the kernels' layouts"""

    def __init__(self, hip, c, d):
        self.hip, self.c = hip, c
        self.To, self.Ho, self.Wo = K.out_dims(c)
        self.n_out, self.n_in = c.B * self.To * self.Ho * self.Wo * c.cout, c.B * c.T * c.H * c.W * c.cin
        self.keep = []

        def up(t, shape):
            a, v = operand(t, shape)
            self.keep.append(a)
            return v

        self.x = up(K.channels_last(d["x"], c.cin), (c.B, c.T, c.H, c.W, c.cin))
        self.dy = up(K.channels_last(d["dy"], c.cout), (c.B, self.To, self.Ho, self.Wo, c.cout))
        self.res = up(K.channels_last(d["res"], c.cout), (c.B, self.To, self.Ho, self.Wo, c.cout)) if d["res"] is not None else None
        cout_real, cin_real = d["w"].shape[:2]
        self.w = up(d["w"].float(), d["w"].shape)
        bias = torch.zeros(c.cout, dtype=torch.float32)
        bias[:cout_real] = d["bias"].float()
        self.bias = up(bias, (c.cout,))
        self.lims = (cout_real, cin_real)

    def fwd(self):
        out = K.out_alloc(self.n_out, torch.bfloat16).cuda()
        wp = self.hip.conv3d_pack_weight(self.w, self.c.cout, self.c.cin)
        self.hip.conv3d_fwd(self.x, wp, self.bias, self.c.cout, self.c.stride, residual=self.res, out=out)
        return out.cpu()

    def dgrad(self):
        dx = K.out_alloc(self.n_in, torch.bfloat16).cuda()
        wp = self.hip.conv3d_pack_weight(self.w, self.c.cout, self.c.cin, for_dgrad=True)
        self.hip.conv3d_dgrad(self.dy, wp, (self.c.T, self.c.H, self.c.W), self.c.cin, self.c.stride, dx=dx)
        return dx.cpu()

    def wgrad(self):
        n = self.lims[0] * self.lims[1] * 27
        dw = K.out_alloc(n, torch.float32).cuda()
        self.hip.conv3d_wgrad(self.x, self.dy, self.c.stride, *self.lims, dw=dw)
        return dw.cpu()


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_conv3d_exact_case_by_bits(hip, c):
    d = K.inputs(c.name)
    run = Run(hip, c, d)
    exp = {"fwd": K.channels_last(K.fwd_reference(c, d), c.cout).double(), "dgrad": K.channels_last(K.dgrad_reference(c, d), c.cin).double(),
           "wgrad": K.wgrad_reference(c, d)}
    for kind in ("fwd", "dgrad", "wgrad"):
        got, again = getattr(run, kind)(), getattr(run, kind)()
        K.check_alloc(got, exp[kind].numel(), exp[kind], None, f"{c.name} {kind}")
        K.assert_bits(again, got, f"{c.name} {kind}: second call")


@pytest.mark.parametrize("c", K.RANDOM_CASES, ids=lambda c: c.name)
def test_conv3d_random_case_under_the_analytic_bar(hip, c):
    d = K.random_inputs(c.name)
    cc = K.Case(c.name, c.B, c.T, c.H, c.W, c.cin, c.cout, c.stride, False, c.cin, c.cout, 1)
    run = Run(hip, cc, d)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    for kind, fn, lay in (("fwd", K.fwd_bar, cl), ("dgrad", K.dgrad_bar, cl), ("wgrad", K.wgrad_bar, lambda t: t)):
        ref, bar = fn(c, d)
        got, again = getattr(run, kind)(), getattr(run, kind)()
        K.check_alloc(got, ref.numel(), lay(ref), lay(bar), f"{c.name} {kind}")
        K.assert_bits(again, got, f"{c.name} {kind}: second call")


@pytest.mark.parametrize("scale", [(2, 2, 2), (1, 2, 2)])
def test_upsample_pair_by_bits(hip, scale):
    B, T, H, W, C = 2, 3, 5, 7, 48
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, T, H, W, generator=g).to(torch.bfloat16)
    up = F.interpolate(x.float(), scale_factor=scale, mode="nearest")
    xa, xv = operand(x.permute(0, 2, 3, 4, 1).contiguous(), (B, T, H, W, C))
    out = K.out_alloc(up.numel(), torch.bfloat16).cuda()
    hip.upsample_nearest_fwd(xv, scale, out=out)
    K.check_alloc(out.cpu(), up.numel(), up.permute(0, 2, 3, 4, 1).double(), None, "upsample fwd")
    # backward: the children are quarter-integers, so their fp32 sum is exact in any order and rounds once
    dout = (torch.randint(-64, 65, up.shape, generator=g).double() / 4).to(torch.bfloat16)
    t, h, w = scale
    exp = dout.double().reshape(B, C, T, t, H, h, W, w).sum((3, 5, 7))
    da, dv = operand(dout.permute(0, 2, 3, 4, 1).contiguous(), (B, T * t, H * h, W * w, C))
    dx = K.out_alloc(x.numel(), torch.bfloat16).cuda()
    hip.upsample_nearest_bwd(dv, scale, dx=dx)
    got = dx.cpu()
    K.check_alloc(got, x.numel(), exp.permute(0, 2, 3, 4, 1), None, "upsample bwd")
    hip.upsample_nearest_bwd(dv, scale, dx=dx)
    K.assert_bits(dx.cpu(), got, "upsample bwd: second call")


def test_layout_pair_by_bits(hip):
    B, C, T, H, W = 2, 3, 3, 5, 7
    v = torch.randn(B, C, T, H, W, generator=torch.Generator().manual_seed(3))
    va, vv = operand(v, v.shape)
    out = K.out_alloc(B * T * H * W * 16, torch.bfloat16).cuda()
    hip.video_to_channels_last(vv, 16, out=out)
    exp = torch.zeros(B, T, H, W, 16, dtype=torch.bfloat16)
    exp[..., :C] = v.permute(0, 2, 3, 4, 1).to(torch.bfloat16)
    K.check_alloc(out.cpu(), exp.numel(), exp.double(), None, "video -> channels last")
    # back: the pad channels hold NaN here and must not be read into the video
    x = torch.full((B, T, H, W, 16), K.NAN, dtype=torch.bfloat16)
    x[..., :C] = exp[..., :C]
    xa, xv = operand(x, x.shape)
    back = K.out_alloc(v.numel(), torch.float32).cuda()
    hip.channels_last_to_video(xv, C, video=back)
    K.check_alloc(back.cpu(), v.numel(), v.to(torch.bfloat16).double(), None, "channels last -> video")
