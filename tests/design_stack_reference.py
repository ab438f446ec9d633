"""CPU restatement of model_design's transformer block, stack and the three modules built on it (models/model_design/base/transformer.py:30-85,
148-216; base/blocks.py) for the tests, written from the formulae, and the deterministic inputs of their fixture
(tests/golden/make_golden_design_stack.py writes the reference's outputs for them; tests/test_design_stack_cpu.py / test_design_stack_gpu.py
replay them).  TEST INFRASTRUCTURE ONLY.  The cross-attention layer is tests/design_reference.py's.

    block:  x <- x + s_sa * SelfAttn(x);  [x <- x + s_ca * CrossAttn(x, context)];  x <- x + s_ffn * ffn(x)         s_*: 0-dim parameters
    SelfAttn: xn = RMSNorm(x); q, k, v = chunk(to_qkv xn); gate = to_gate xn; q, k <- rotary(head RMSNorm(q or k));
              out_proj(softmax(q k^T / 8) v * sigmoid(gate))
    ffn:    xn = RMSNorm(x); a, g = chunk(ffn.1 xn); ffn.3(gelu(g) * a)
    stack:  blocks, then final_norm (fp32 out)

`emulate_bf16=True` rounds where autocast(bf16) materialises bf16 tensors -- the rounding points of the HIP path: every Linear's operands and
output, the two roundings of the head norm, the rotation, the attention output, sigmoid / gelu and their products, and the residual product
`s * f(x)`, which torch forms in bf16 (the 0-dim scale is converted to bf16 first, measured on the CPU and on the device).
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import inputs as gen
from oracle.larp_oracle import _rb, linear
from tests import design_reference as C

EPS = C.EPS
rel_l2 = C.rel_l2
ATTN_NAMES = ("norm.weight", "to_qkv.weight", "to_gate.weight", "q_norm.weight", "k_norm.weight", "out_proj.weight")

STACK_CASES = {
    # L = 70 = 6 query tokens + grid (2, 4, 8), ragged against 64; inner = 96 is no multiple of 64; dcontext accumulates over two layers
    "xs2": dict(dim=128, heads=2, mlp_ratio=1, num_layers=2, cross=True, B=2, tokens=6, grid=(2, 4, 8), Lk=33, seed=5100),
    # L = 68 = 4 + grid (1, 8, 8), the shape of the first-frame table; inner = 352
    "s1": dict(dim=128, heads=2, mlp_ratio=4, num_layers=1, cross=False, B=2, tokens=4, grid=(1, 8, 8), Lk=0, seed=5200),
}
# the reference's Encoder, FirstFrameEncoder and UnifiedDecoder at 'tiny' (width 256, 4 heads, 4 layers; 2 in the first-frame encoder)
MOD = dict(model_size="tiny", in_grid=(4, 32, 32), patch_size=(4, 8, 8), tokens=8, cond_tokens=4, B=2, token_size=6, seed=5300)
MOD_WIDTH, MOD_HEADS, MOD_LAYERS, MOD_MLP = 256, 4, 4, 4.0
SMALL_GRAD = 4096            # the fixture keeps the module parameters' gradients of at most this many elements


def inner_dim(dim, mult, mult_of=32):
    inner = int(mult * (2 / 3) * dim)
    return mult_of * ((inner + mult_of - 1) // mult_of)


def stack_param_shapes(dim, mlp_ratio, num_layers, cross, prefix=""):
    """name -> shape in the order of the reference's state_dict()"""
    inner = inner_dim(dim, mlp_ratio)
    out = {}
    for i in range(num_layers):
        p = f"{prefix}layers.{i}."
        out[p + "res_scale_sa"] = ()
        out[p + "res_scale_ffn"] = ()
        if cross:
            out[p + "res_scale_ca"] = ()
        for n, s in zip(ATTN_NAMES, ((dim,), (3 * dim, dim), (dim, dim), (64,), (64,), (dim, dim))):
            out[p + "self_attn." + n] = s
        out[p + "ffn.0.weight"], out[p + "ffn.1.weight"], out[p + "ffn.3.weight"] = (dim,), (2 * inner, dim), (dim, inner)
        if cross:
            for n, s in zip(C.PARAM_NAMES, ((dim,), (dim,), (dim, dim), (2 * dim, dim), (dim, dim), (64,), (64,), (dim, dim))):
                out[p + "cross_attn." + n] = s
    out[prefix + "final_norm.weight"] = (dim,)
    return out


def make_params(shapes, seed):
    """deterministic values by position in `shapes`: norm weights 1 + 0.2 N(0, 1), residual scales in [0.45, 1.15] (away from their
    initialisation 1 / sqrt(2 i + 1)), query tokens N(0, 1) / sqrt(width), biases 0.02 N(0, 1), matrices xavier-uniform"""
    out = {}
    for j, (n, shp) in enumerate(shapes.items()):
        s = seed + 7 * j
        if shp == ():
            v = gen.uniform((1,), s, 0.45, 1.15).reshape(())
        elif n.endswith("tokens"):
            v = gen.normal(shp, s) * shp[-1] ** -0.5
        elif n.endswith("bias"):
            v = 0.02 * gen.normal(shp, s)
        elif len(shp) == 1:
            v = 1.0 + 0.2 * gen.normal(shp, s)
        else:
            v = gen.xavier_uniform((shp[0], int(np.prod(shp[1:]))), s).reshape(shp)
        out[n] = np.asarray(v, dtype=np.float32)
    return out


def tables(tokens, grid):
    from video_tokenizer_amd.titok import rope_tables
    return rope_tables(tokens, list(grid), head_dim=64)


def stack_inputs(name):
    c = STACK_CASES[name]
    L = c["tokens"] + math.prod(c["grid"])
    I = {"x": gen.normal((c["B"], L, c["dim"]), c["seed"] + 1).astype(np.float32), "w": gen.normal((c["B"], L, c["dim"]), c["seed"] + 3).astype(np.float32)}
    if c["cross"]:
        I["context"] = gen.normal((c["B"], c["Lk"], c["dim"]), c["seed"] + 2).astype(np.float32)
    I.update(make_params(stack_param_shapes(c["dim"], c["mlp_ratio"], c["num_layers"], c["cross"]), c["seed"] + 100))
    return I


# ---------------------------------------------------------------------------------------------------------------- the formulae
def rotate(t, cos, sin, emu):
    """t [B, L, H, 64]; pair j of a head is (t[2j], t[2j+1]); tables [L, 32]"""
    a, b = t[..., 0::2], t[..., 1::2]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return _rb(torch.stack([a * c - b * s, a * s + b * c], dim=-1).flatten(-2), emu)


def self_attention(x, P, pre, heads, cos, sin, emu):
    xn = C.rmsnorm(x, P[pre + "norm.weight"])
    q, k, v = linear(xn, P[pre + "to_qkv.weight"], None, emu).chunk(3, dim=-1)
    gate = linear(xn, P[pre + "to_gate.weight"], None, emu)
    q = rotate(C.head_rmsnorm(q, P[pre + "q_norm.weight"], heads, emu), cos, sin, emu).transpose(1, 2)
    k = rotate(C.head_rmsnorm(k, P[pre + "k_norm.weight"], heads, emu), cos, sin, emu).transpose(1, 2)
    v = v.unflatten(-1, (heads, 64)).transpose(1, 2)
    att = torch.softmax((q @ k.transpose(-2, -1)) * 0.125, dim=-1)
    o = _rb(att @ v, emu).transpose(1, 2).flatten(-2)
    og = _rb(o * _rb(torch.sigmoid(gate), emu), emu)
    return linear(og, P[pre + "out_proj.weight"], None, emu)


def ffn(x, P, pre, emu):
    xn = C.rmsnorm(x, P[pre + "0.weight"])
    a, g = linear(xn, P[pre + "1.weight"], None, emu).chunk(2, dim=-1)
    return linear(_rb(_rb(F.gelu(g), emu) * a, emu), P[pre + "3.weight"], None, emu)


def residual(x, s, y, emu):
    return x + _rb(_rb(s, emu) * y, emu)


def stack(x, P, prefix, heads, num_layers, cross, cos, sin, context=None, emu=False):
    for i in range(num_layers):
        p = f"{prefix}layers.{i}."
        x = residual(x, P[p + "res_scale_sa"], self_attention(x, P, p + "self_attn.", heads, cos, sin, emu), emu)
        if cross and context is not None:
            sub = {n: P[p + "cross_attn." + n] for n in C.PARAM_NAMES}
            x = residual(x, P[p + "res_scale_ca"], C.cross_attention(x, context, sub, heads, emu), emu)
        x = residual(x, P[p + "res_scale_ffn"], ffn(x, P, p + "ffn.", emu), emu)
    return C.rmsnorm(x, P[prefix + "final_norm.weight"])


def pooled_scale_grads(grads, names):
    """the gradients of the 0-dim residual scales among `names`, in that order, as one vector"""
    return torch.stack([grads[n].reshape(()) for n in names if n.rsplit(".", 1)[-1].startswith("res_scale_")])


def run_stack(name, emulate_bf16=False):
    """-> tensor name -> fp32 torch tensor for the loss sum(y * w): y, dx, [dcontext], d_<parameter> of every matrix / vector parameter and
    d_res_scales (the scalars pooled into one vector)"""
    c = STACK_CASES[name]
    I = {k: torch.from_numpy(v) for k, v in stack_inputs(name).items()}
    names = list(stack_param_shapes(c["dim"], c["mlp_ratio"], c["num_layers"], c["cross"]))
    x = I["x"].clone().requires_grad_(True)
    ctx = I["context"].clone().requires_grad_(True) if c["cross"] else None
    P = {n: I[n].clone().requires_grad_(True) for n in names}
    cos, sin = tables(c["tokens"], c["grid"])
    y = stack(x, P, "", c["heads"], c["num_layers"], c["cross"], cos, sin, ctx, emulate_bf16)
    (y * I["w"]).sum().backward()
    return collect(y, {"dx": x.grad, "dcontext": ctx.grad if ctx is not None else None}, {n: P[n].grad for n in names}, names)


def collect(y, input_grads, grads, names, small_only=False, y_name="y"):
    out = {y_name: y.detach().float()}
    out.update({k: v.float() for k, v in input_grads.items() if v is not None})
    for n in names:
        if n.rsplit(".", 1)[-1].startswith("res_scale_"):
            continue
        if not small_only or grads[n].numel() <= SMALL_GRAD:
            out["d_" + n] = grads[n].float()
    out["d_res_scales"] = pooled_scale_grads(grads, names).float()
    return out


# ---------------------------------------------------------------------------------------------------------------- the modules
def mod_shapes():
    """name -> shape of the three modules' parameters in the reference's state_dict() order, per module"""
    W, ts = MOD_WIDTH, MOD["token_size"]
    pt, ph, pw = MOD["patch_size"]
    enc = {"patch_embed.weight": (W, 3, pt, ph, pw), "patch_embed.bias": (W,), "query_tokens.tokens": (1, MOD["tokens"], W)}
    enc.update(stack_param_shapes(W, MOD_MLP, MOD_LAYERS, False, "transformer."))
    enc.update({"proj_out.weight": (ts, W), "proj_out.bias": (ts,)})
    ffe = {"patch_embed.weight": (W, 3, ph, pw), "patch_embed.bias": (W,), "query_tokens.tokens": (1, MOD["cond_tokens"], W)}
    ffe.update(stack_param_shapes(W, MOD_MLP, max(MOD_LAYERS // 2, 2), False, "transformer."))
    ffe.update({"proj_out.weight": (ts, W), "proj_out.bias": (ts,)})
    grid = [a // b for a, b in zip(MOD["in_grid"], MOD["patch_size"])]
    dec = {"proj_in.weight": (W, ts), "proj_in.bias": (W,), "proj_cond.weight": (W, ts), "proj_cond.bias": (W,), "cond_adapter.0.weight": (W,),
           "cond_adapter.1.weight": (W, W), "cond_adapter.3.weight": (W, W), "query_tokens.tokens": (1, math.prod(grid), W)}
    dec.update(stack_param_shapes(W, MOD_MLP, MOD_LAYERS, True, "transformer."))
    dec.update({"proj_out.weight": (3 * pt * ph * pw, W), "proj_out.bias": (3 * pt * ph * pw,)})
    return {"encoder": enc, "first_frame_encoder": ffe, "decoder": dec}


def mod_inputs():
    B, s = MOD["B"], MOD["seed"]
    T, S, _ = MOD["in_grid"]
    I = {"video": gen.video_clips(B, T, S, s + 1).astype(np.float32),
         "w_main": gen.normal((B, MOD["tokens"], MOD["token_size"]), s + 2).astype(np.float32),
         "w_first": gen.normal((B, MOD["cond_tokens"], MOD["token_size"]), s + 3).astype(np.float32),
         "w_pred": gen.normal((B, 3, T, S, S), s + 4).astype(np.float32)}
    for k, (mod, shapes) in enumerate(mod_shapes().items()):
        I.update({f"{mod}.{n}": v for n, v in make_params(shapes, s + 1000 * (k + 1)).items()})
    return I


def _sub(I, mod):
    return {n[len(mod) + 1:]: v for n, v in I.items() if n.startswith(mod + ".")}


def conv_embed(x, w, b, emu):
    """Conv3d / Conv2d with kernel = stride under autocast: bf16 operands, bf16 output; -> [B, tokens, width]"""
    conv = F.conv3d if w.dim() == 5 else F.conv2d
    y = _rb(conv(_rb(x, emu), _rb(w, emu), b, stride=tuple(w.shape[2:])), emu)
    return y.flatten(2).transpose(1, 2)


def encoder(video, P, tokens, grid, layers, emu):
    tok = conv_embed(video, P["patch_embed.weight"], P["patch_embed.bias"], emu)
    h = torch.cat([P["query_tokens.tokens"].expand(video.shape[0], -1, -1), tok], dim=1)
    cos, sin = tables(tokens, grid)
    h = stack(h, P, "transformer.", MOD_HEADS, layers, False, cos, sin, None, emu)
    return linear(h[:, :tokens], P["proj_out.weight"], P["proj_out.bias"], emu)


def decoder(main_q, first_q, P, emu):
    grid = [a // b for a, b in zip(MOD["in_grid"], MOD["patch_size"])]
    x = linear(main_q, P["proj_in.weight"], P["proj_in.bias"], emu)
    c = linear(first_q, P["proj_cond.weight"], P["proj_cond.bias"], emu)
    u = _rb(c * torch.rsqrt(torch.mean(c * c, dim=-1, keepdim=True) + EPS), emu) * P["cond_adapter.0.weight"]
    t = linear(_rb(F.silu(linear(u, P["cond_adapter.1.weight"], None, emu)), emu), P["cond_adapter.3.weight"], None, emu)
    context = _rb(c + t, emu)
    B = main_q.shape[0]
    h = torch.cat([x, P["query_tokens.tokens"].expand(B, -1, -1)], dim=1)
    cos, sin = tables(MOD["tokens"], grid)
    h = stack(h, P, "transformer.", MOD_HEADS, MOD_LAYERS, True, cos, sin, context, emu)
    rows = linear(h[:, MOD["tokens"]:], P["proj_out.weight"], P["proj_out.bias"], emu)
    (t_, hh, ww), (pt, ph, pw) = grid, MOD["patch_size"]
    rows = rows.reshape(B, t_, hh, ww, pt, ph, pw, 3).permute(0, 7, 1, 4, 2, 5, 3, 6)
    return rows.reshape(B, 3, t_ * pt, hh * ph, ww * pw)


def run_mod(codes, emulate_bf16=False):
    """codes: (main_q, first_q) of the fixture (the reference's own quantised codes).  -> "<module>/<tensor>" -> fp32 tensor: the pre-FSQ
    tokens of both encoders under the losses sum(tokens * w_main / w_first), pred_frames for the fixture's codes under sum(pred * w_pred),
    the input gradients, the parameter gradients of at most SMALL_GRAD elements and the pooled residual-scale gradients"""
    I = {k: torch.from_numpy(v) for k, v in mod_inputs().items()}
    grid = [a // b for a, b in zip(MOD["in_grid"], MOD["patch_size"])]
    out = {}
    for mod, w, tokens, g, layers in (("encoder", "w_main", MOD["tokens"], grid, MOD_LAYERS),
                                      ("first_frame_encoder", "w_first", MOD["cond_tokens"], [1] + grid[1:], max(MOD_LAYERS // 2, 2))):
        P = {n: v.clone().requires_grad_(True) for n, v in _sub(I, mod).items()}
        video = I["video"].clone().requires_grad_(True)
        tok = encoder(video if mod == "encoder" else video[:, :, 0], P, tokens, g, layers, emulate_bf16)
        (tok * I[w]).sum().backward()
        res = collect(tok, {"dvideo": video.grad}, {n: p.grad for n, p in P.items()}, list(P), small_only=True, y_name="tokens")
        out.update({f"{mod}/{k}": v for k, v in res.items()})
    P = {n: v.clone().requires_grad_(True) for n, v in _sub(I, "decoder").items()}
    mq, fq = (torch.as_tensor(t).clone().requires_grad_(True) for t in codes)
    pred = decoder(mq, fq, P, emulate_bf16)
    (pred * I["w_pred"]).sum().backward()
    res = collect(pred, {"dmain_q": mq.grad, "dfirst_q": fq.grad}, {n: p.grad for n, p in P.items()}, list(P), small_only=True, y_name="pred_frames")
    out.update({f"decoder/{k}": v for k, v in res.items()})
    return out


# ---------------------------------------------------------------------------------------------------------------- the fixture
GOLDEN_FILES = ("design_stack.npz", "design_stack_2.npz", "design_stack_3.npz", "design_stack_4.npz", "design_stack_5.npz")


def load_golden():
    """the fixture, merged over its files: "<case>/<tensor>", "<case>/<tensor>_bf16_dist", "rope/...", "state_dict/..." -> numpy"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for f in GOLDEN_FILES:
        with np.load(os.path.join(here, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out
