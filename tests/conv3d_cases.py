"""Edge cases, references and reference mutants of the 3x3x3 convolution kernels (csrc/vt_conv3d.hip: vt_conv3d_fwd, vt_conv3d_dgrad,
vt_conv3d_wgrad and the weight pack in front of them).  torch on the CPU only: no GPU and no built library.  The pattern is that of
tests/gemm_cases.py; tests/test_conv3d_cases_cpu.py proves that the cases discriminate, tests/test_conv3d_edges_gpu.py runs the kernels.

EXACT FAMILY (CASES).  Operands are small integers held in bf16, drawn from a generator seeded by the case's name: activations and output
gradients in [-2, 2], weights in [-3, 3] times the per-case integer `bscale`; bias and residual are multiples of 1/4.  Every fp32 sum is then
exact in any order (workspace partials of the weight gradient included), so each expected output is a bit pattern.  The references evaluate
tap by tap in float64 and assert that every value they round is representable in fp32: the exactness is checked, not assumed.
    forward : out = bf16(acc + bias), with a residual out = bf16(float(bf16(acc + bias)) + float(res))
    dgrad   : dx = bf16(sum), the transposed convolution of dy
    wgrad   : dW fp32 [Cout, Cin, 3, 3, 3] over all B T' H' W' output positions
    shapes (T, H, W): (1,1,1), (1,4,4), (3,5,7), (2,9,17), (4,16,16) and (5,18,35), which crosses the 2 x 8 x 16 position tile of the stride-1
    kernel, the 2 x 2 x 16 tile of the strided forward and the 8 x 16 / 2 x 16 tiles of the weight gradient in every axis; B in {1, 2} with
    different content per clip; strides (1,1,1), (1,2,2), (2,2,2) on odd and even extents; (Cin, Cout) in {(16,16), (16,32), (32,32), (64,128),
    (128,64), (128,1024), (1024,128)} and the padded 3-channel ends (3 -> 16 in, 16 -> 3 out: the operand has 16 channels, the parameter 3);
    with and without residual.
POISON AND CONTAINMENT.  Every operand is the leading part of a larger allocation whose remainder is NaN; every output allocation is prefilled
with the sentinels of tests/gemm_cases.py, and everything outside the addressed part must keep its bits (`poisoned`, `out_alloc`, `check_alloc`).
RANDOM FAMILY (RANDOM_CASES): x ~ N(0,1), w and dy ~ N(0,4) in bf16 at three ragged shapes, for each of the three kernels.  Judged per
element against the float64 result on the bf16 values: |err| <= K 2^-23 (|x| (*) |w|) + 2^-8 |ref| with K = 27 Cin (27 Cout for dgrad; the
second term for bf16 outputs only), and for the weight gradient K = positions without the second term: gemm_cases' rule, which holds for
any order of the same sums.
MUTANTS (`MUTANTS`): the reference with one kernel-level error -- tap_drop(k), pad_clamped, halo_from_next_clip, w_wraps_into_next_row,
stride_phase_off_by_one, cin_slab_drop, bias_shift, residual_before_round (forward), wgrad_partial_drop (weight gradient), dgrad_unflipped
(input gradient).  `applies(mutant, case)` says where a mutant can show at all (a stride mutant needs a stride, a clip mutant two clips ...);
a mutant is CAUGHT on a case when it changes an expected bit.
    exemptions (EXEMPT, exact and capped at 5 % of the applicable pairs by the CPU test): see the table below."""
import collections
import functools
import zlib

import torch

from tests.gemm_cases import SENT16, SENT32, assert_bits, bits, is_f32, rbf, sentinel  # noqa: F401  (shared with the GPU test)

NAN = float("nan")
TAIL = 96                      # poison / sentinel elements behind every allocation
STRIDES = ((1, 1, 1), (1, 2, 2), (2, 2, 2))

Case = collections.namedtuple("Case", "name B T H W cin cout stride res cin_real cout_real bscale")


def _c(B, thw, cin, cout, stride=(1, 1, 1), res=False, cin_real=None, cout_real=None, bscale=1):
    T, H, W = thw
    name = f"b{B}_{T}x{H}x{W}_c{cin_real or cin}to{cout_real or cout}_s{''.join(map(str, stride))}" + ("_res" if res else "")
    return Case(name, B, T, H, W, cin, cout, stride, res, cin_real or cin, cout_real or cout, bscale)


S1, S122, S222 = STRIDES
CASES = [
    # every shape at the smallest channel pair, B = 1 and 2, the three strides on odd and even extents
    _c(1, (1, 1, 1), 16, 16, bscale=5), _c(2, (1, 1, 1), 16, 16, S222, bscale=5), _c(1, (1, 1, 1), 32, 32, S122, res=True, bscale=3),
    _c(1, (1, 4, 4), 16, 16, res=True, bscale=5), _c(2, (1, 4, 4), 16, 32, S122, bscale=5), _c(1, (1, 4, 4), 32, 32, S222, bscale=3),
    _c(2, (3, 5, 7), 16, 16, bscale=5), _c(1, (3, 5, 7), 16, 32, S122, res=True, bscale=5), _c(2, (3, 5, 7), 32, 32, S222, bscale=3),
    _c(1, (2, 9, 17), 32, 32, res=True, bscale=3), _c(2, (2, 9, 17), 16, 16, S122, bscale=5), _c(1, (2, 9, 17), 16, 32, S222, res=True, bscale=5),
    _c(1, (4, 16, 16), 16, 32, bscale=5), _c(2, (4, 16, 16), 32, 32, S122, res=True, bscale=3), _c(1, (4, 16, 16), 16, 16, S222, bscale=5),
    _c(2, (5, 18, 35), 16, 16, res=True, bscale=5), _c(1, (5, 18, 35), 16, 16, S122, bscale=5), _c(1, (5, 18, 35), 16, 32, S222, bscale=5),
    # the wider channel pairs: several K slabs, N fragments of 1, 2 and 4, one and many N tiles
    _c(2, (3, 5, 7), 64, 128, res=True, bscale=3), _c(1, (2, 9, 17), 128, 64, S122, bscale=1), _c(1, (3, 5, 7), 128, 64, S222, res=True, bscale=1),
    _c(2, (1, 4, 4), 128, 1024, bscale=1), _c(1, (1, 4, 4), 1024, 128, res=True, bscale=1), _c(1, (3, 5, 7), 64, 128, S222, bscale=3),
    _c(1, (1, 4, 4), 1024, 128, S122, bscale=1),
    # the padded 3-channel ends, both directions
    _c(2, (3, 5, 7), 16, 32, cin_real=3, bscale=7), _c(1, (2, 9, 17), 32, 16, cout_real=3, bscale=5), _c(1, (4, 16, 16), 16, 16, cin_real=3, bscale=7),
    _c(2, (1, 4, 4), 16, 16, cout_real=3, bscale=5),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

RandomCase = collections.namedtuple("RandomCase", "name B T H W cin cout stride")
RANDOM_CASES = [RandomCase("rand_b2_3x7x19_c32to48_s111", 2, 3, 7, 19, 32, 48, S1), RandomCase("rand_b1_4x9x21_c64to32_s122", 1, 4, 9, 21, 64, 32, S122),
                RandomCase("rand_b1_5x11x18_c48to64_s222", 1, 5, 11, 18, 48, 64, S222)]


def out_dims(c):
    return tuple((n - 1) // s + 1 for n, s in zip((c.T, c.H, c.W), c.stride))


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float64 tensors in torch's logical shapes: x [B, Cin_real, T, H, W], w [Cout_real, Cin_real, 3, 3, 3], bias [Cout_real],
    res / dy [B, Cout_real, T', H', W'] (all bf16-representable; bias fp32-representable)"""
    c, g = BY_NAME[name], _gen(name)
    To, Ho, Wo = out_dims(c)
    d = dict(x=_ints(g, (c.B, c.cin_real, c.T, c.H, c.W), -2, 2), w=_ints(g, (c.cout_real, c.cin_real, 3, 3, 3), -3, 3) * c.bscale,
             bias=_ints(g, (c.cout_real,), -16, 16) / 4, dy=_ints(g, (c.B, c.cout_real, To, Ho, Wo), -2, 2))
    d["res"] = _ints(g, (c.B, c.cout_real, To, Ho, Wo), -32, 32) / 4 if c.res else None
    return d


@functools.lru_cache(maxsize=None)
def random_inputs(name):
    c = next(r for r in RANDOM_CASES if r.name == name)
    g = _gen(name)
    To, Ho, Wo = out_dims(c)
    n = lambda shape, std: (torch.randn(shape, generator=g) * std).to(torch.bfloat16).double()
    return dict(x=n((c.B, c.cin, c.T, c.H, c.W), 1.0), w=n((c.cout, c.cin, 3, 3, 3), 2.0), bias=n((c.cout,), 1.0).float().double(),
                dy=n((c.B, c.cout, To, Ho, Wo), 2.0), res=None)


# ---- references ----------------------------------------------------------------------------------------------------------------------------
def _pad(x, mutant):
    """x [B, C, T, H, W] with one position of padding per side: zeros, or what a mutant would read there"""
    B, C, T, H, W = x.shape
    p = torch.zeros(B, C, T + 2, H + 2, W + 2, dtype=x.dtype)
    p[:, :, 1:-1, 1:-1, 1:-1] = x
    if mutant == "pad_clamped":
        p = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1), mode="replicate")
    elif mutant == "halo_from_next_clip":          # the frame behind a clip's last is the next clip's first, the one before its first the previous clip's last
        flat = x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
        for b in range(B):
            if b + 1 < B:
                p[b, :, T + 1, 1:-1, 1:-1] = flat[(b + 1) * T]
            if b > 0:
                p[b, :, 0, 1:-1, 1:-1] = flat[b * T - 1]
    elif mutant == "w_wraps_into_next_row":        # the position right of a row's end is the next row's first, left of its start the previous row's last
        p[:, :, 1:-1, 1:H, W + 1] = x[:, :, :, 1:, 0]
        p[:, :, 1:-1, 2:H + 1, 0] = x[:, :, :, :-1, W - 1]
    return p


def _tap_view(p, c, kt, kh, kw, phase=0):
    """the padded source at tap (kt, kh, kw) for every output position: [B, C, T', H', W']"""
    To, Ho, Wo = out_dims(c)
    st, sh, sw = c.stride
    off = [k + (phase if s > 1 else 0) for k, s in zip((kt, kh, kw), c.stride)]
    if phase:
        p = torch.nn.functional.pad(p, (0, 1, 0, 1, 0, 1))
    return p[:, :, off[0]:off[0] + (To - 1) * st + 1:st, off[1]:off[1] + (Ho - 1) * sh + 1:sh, off[2]:off[2] + (Wo - 1) * sw + 1:sw]


def conv_acc(c, x, w, mutant=None):
    """sum over taps and input channels in float64: [B, Cout, T', H', W']"""
    p = _pad(x, mutant)
    acc = 0
    for t in range(27):
        kt, kh, kw = t // 9, t // 3 % 3, t % 3
        if mutant == f"tap_drop({t})":
            continue
        wt = w[:, :, kt, kh, kw]
        if mutant == "cin_slab_drop":              # the last 32-channel slab of the source (the only one below 33 channels) never arrives
            wt = wt.clone()
            wt[:, (x.shape[1] - 1) // 32 * 32:] = 0
        acc = acc + torch.einsum("bcthw,oc->bothw", _tap_view(p, c, kt, kh, kw, 1 if mutant == "stride_phase_off_by_one" else 0), wt)
    return acc


def fwd_reference(c, d, mutant=None, exact=True):
    acc = conv_acc(c, d["x"], d["w"], mutant)
    bias = d["bias"].roll(-4) if mutant == "bias_shift" and len(d["bias"]) > 4 else d["bias"].roll(-1) if mutant == "bias_shift" else d["bias"]
    v = acc + bias.view(1, -1, 1, 1, 1)
    if exact:
        assert is_f32(v), c.name
    if d["res"] is None:
        return rbf(v)
    s = (v if mutant == "residual_before_round" else rbf(v)) + d["res"]
    if exact:
        assert is_f32(s), c.name
    return rbf(s)


def dgrad_acc(c, dy, w, mutant=None):
    To, Ho, Wo = out_dims(c)
    st, sh, sw = c.stride
    B, Cin = dy.shape[0], w.shape[1]
    ext = [max(n + 2, (o - 1) * s + 3) for n, o, s in zip((c.T, c.H, c.W), (To, Ho, Wo), c.stride)]
    p = torch.zeros(B, Cin, *ext, dtype=torch.float64)
    for t in range(27):
        kt, kh, kw = t // 9, t // 3 % 3, t % 3
        wt = w[:, :, 2 - kt, 2 - kh, 2 - kw] if mutant == "dgrad_unflipped" else w[:, :, kt, kh, kw]
        p[:, :, kt:kt + (To - 1) * st + 1:st, kh:kh + (Ho - 1) * sh + 1:sh, kw:kw + (Wo - 1) * sw + 1:sw] += torch.einsum("bothw,oc->bcthw", dy, wt)
    return p[:, :, 1:c.T + 1, 1:c.H + 1, 1:c.W + 1]


def dgrad_reference(c, d, mutant=None, exact=True):
    v = dgrad_acc(c, d["dy"], d["w"], mutant)
    if exact:
        assert is_f32(v), c.name
    return rbf(v)


def wgrad_reference(c, d, mutant=None, exact=True):
    dy = d["dy"]
    if mutant == "wgrad_partial_drop":             # the last quarter of the output positions (at least one) never reaches the sum
        flat = dy.permute(0, 2, 3, 4, 1).reshape(-1, dy.shape[1]).clone()
        flat[len(flat) - max(1, len(flat) // 4):] = 0
        dy = flat.reshape(dy.shape[0], *dy.shape[2:], dy.shape[1]).permute(0, 4, 1, 2, 3)
    p = _pad(d["x"], None)
    dw = torch.zeros_like(d["w"])
    for t in range(27):
        kt, kh, kw = t // 9, t // 3 % 3, t % 3
        dw[:, :, kt, kh, kw] += torch.einsum("bothw,bcthw->oc", dy, _tap_view(p, c, kt, kh, kw))    # (+=: a sum that starts at +0 is never -0)
    if exact:
        assert is_f32(dw) and float(dw.abs().max()) < 2 ** 24, c.name
    return dw


def fwd_bar(c, d):
    """per element: K 2^-23 (|x| (*) |w|) + 2^-8 |ref| around the float64 value before the output rounding, K = 27 Cin"""
    ref = conv_acc(c, d["x"], d["w"]) + d["bias"].view(1, -1, 1, 1, 1)
    mag = conv_acc(c, d["x"].abs(), d["w"].abs()) + d["bias"].abs().view(1, -1, 1, 1, 1)
    return ref, 27 * d["x"].shape[1] * 2.0 ** -23 * mag + 2.0 ** -8 * ref.abs()


def dgrad_bar(c, d):
    ref = dgrad_acc(c, d["dy"], d["w"])
    return ref, 27 * d["w"].shape[0] * 2.0 ** -23 * dgrad_acc(c, d["dy"].abs(), d["w"].abs()) + 2.0 ** -8 * ref.abs()


def wgrad_bar(c, d):
    ref = wgrad_reference(c, d, exact=False)
    To, Ho, Wo = out_dims(c)
    mag = wgrad_reference(c, dict(d, x=d["x"].abs(), dy=d["dy"].abs()), exact=False)
    return ref, c.B * To * Ho * Wo * 2.0 ** -23 * mag


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
FWD_MUTANTS = tuple(f"tap_drop({t})" for t in range(27)) + ("pad_clamped", "halo_from_next_clip", "w_wraps_into_next_row", "stride_phase_off_by_one",
                                                            "cin_slab_drop", "bias_shift", "residual_before_round")
MUTANTS = {"fwd": FWD_MUTANTS, "wgrad": ("wgrad_partial_drop",), "dgrad": ("dgrad_unflipped",)}
REFERENCES = {"fwd": fwd_reference, "wgrad": wgrad_reference, "dgrad": dgrad_reference}


def _tap_reaches(n, s, k):
    """whether tap k of an axis of n positions and stride s reads inside the clip for some output position"""
    return any(0 <= o * s + k - 1 < n for o in range((n - 1) // s + 1))


def applies(mutant, c):
    """whether the mutant can change anything on the case at all"""
    if mutant.startswith("tap_drop"):              # a tap whose source is padding for every output position reads zeros either way
        t = int(mutant[9:-1])
        return all(_tap_reaches(n, s, k) for n, s, k in zip((c.T, c.H, c.W), c.stride, (t // 9, t // 3 % 3, t % 3)))
    if mutant == "dgrad_unflipped":                # mirrors the taps: the centre tap alone is its own mirror image
        return (c.T, c.H, c.W) != (1, 1, 1)
    if mutant == "pad_clamped":
        return True
    if mutant == "halo_from_next_clip":
        return c.B > 1
    if mutant == "w_wraps_into_next_row":
        return c.H > 1
    if mutant == "stride_phase_off_by_one":
        return c.stride != S1
    if mutant == "residual_before_round":
        return c.res
    return True


# (mutant, case) pairs that apply but change no bit, each with its reason; exact: the CPU test fails on a missing AND on a superfluous entry
EXEMPT = {
    ("residual_before_round", "b1_1x1x1_c32to32_s122_res"): "one position, 32 outputs: one rounding and two give the same bits on every one of them",
}


# ---- buffers: what the GPU test uploads, in the kernels' layouts ---------------------------------------------------------------------------
def channels_last(t, cpad):
    """[B, C, T, H, W] float64 -> bf16 [B, T, H, W, cpad], channels C.. zero"""
    B, C = t.shape[:2]
    out = torch.zeros(B, *t.shape[2:], cpad, dtype=torch.float64)
    out[..., :C] = t.permute(0, 2, 3, 4, 1)
    return out.to(torch.bfloat16)


def logical(flat, B, thw, c_abi, c_real):
    """the first B T H W c_abi elements of an allocation as [B, c_real, T, H, W], and the pad channels [B, T, H, W, c_abi - c_real]"""
    v = flat[:B * thw[0] * thw[1] * thw[2] * c_abi].reshape(B, *thw, c_abi)
    return v[..., :c_real].permute(0, 4, 1, 2, 3), v[..., c_real:]


def poisoned(t):
    """t flattened into the head of an allocation whose tail is NaN"""
    a = torch.full((t.numel() + TAIL,), NAN, dtype=t.dtype)
    a[:t.numel()] = t.reshape(-1)
    return a


def out_alloc(n, dtype):
    return sentinel((n + TAIL,), dtype)


def check_alloc(alloc, n, exp, bar, what):
    """alloc: a whole flat output allocation after the call (CPU).  Its first n elements against exp (flat float64, or the exact dtype) by bits --
    or under `bar`, where a NaN fails --, the tail against the sentinel."""
    head = alloc[:n]
    if bar is None:
        assert_bits(head, exp.reshape(-1).to(torch.float32).to(alloc.dtype), what)
    else:
        ok = (head.double() - exp.reshape(-1)).abs() <= bar.reshape(-1)
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0])
            raise AssertionError(f"{what}: {int((~ok).sum())} of {n} elements outside the bar, first at {i}: got {head[i].item()!r} expected "
                                 f"{exp.reshape(-1)[i].item()!r} bar {bar.reshape(-1)[i].item():.3e}")
    assert_bits(alloc[n:], sentinel((alloc.numel() - n,), alloc.dtype), what + " (behind the addressed part)")
