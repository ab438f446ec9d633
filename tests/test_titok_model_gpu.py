"""The packed `titok` encoder, decoder and model on the GPU against the fixture the reference's own code wrote
(tests/golden/make_golden_titok.py), and against themselves.

Tolerance, from the reference alone (the rule of tests/test_varlen_layer_gpu.py and tests/test_design_gpu.py): for both cases and both
stages, every stored tensor -- z and d_clips and the encoder's parameter gradients; pred, d_codes and the decoder's -- is within 2 x the
distance of the reference's OWN autocast-bf16 CPU run from its fp32 run (`<tensor>_bf16_dist` in the fixture).  Each stage prints
`RATIO <case> <stage> <tensor> <distance> <bf16_dist> <ratio>` first.  A second step reproduces every bit.

The rest is exact: the four clips in one packed call equal four one-clip calls; a block equals x + Attn(x) and x1 + ffd(x1) composed from
varlen.Attn and plain hip.* calls; forward equals decode(encode(.)); the whole-model backward equals the two stages chained by hand.

Measured ratios on an MI355X (distance / bf16_dist, bar 2); per stage the outputs, the input-side gradients, mask_token, and the largest
and smallest over all stored tensors (the full table is in DESIGN.md 5i):
  A enc: z 0.972, d_clips 1.011, d_mask_token 0.966; largest 1.361 (attn_layer.0.k_norm.bias), smallest 0.720 (proj_out.bias)
  A dec: pred 1.098, d_codes 0.766, d_mask_token 1.078; largest 1.507 (attn_layer.1.q_norm.weight), smallest 0.554 (attn_layer.0.q_norm.weight)
  B enc: z 0.990, d_clips 1.019, d_mask_token 1.074 (the largest); smallest 0.492 (attn_layer.0.q_norm.weight)
  B dec: pred 1.074, d_codes 0.955, d_mask_token 1.089 (the largest); smallest 0.723 (proj_out.bias)
"""
import pytest
import torch

from oracle import inputs as gen
from tests import titok_reference as R

pytestmark = pytest.mark.gpu

DIMS_A = R.CASES["A"]["dims"]


def vt():
    import video_tokenizer_amd
    return video_tokenizer_amd


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _build(case, stage):
    dims = R.CASES[case]["dims"]
    m = vt().varlen.TiTokEncoder(out_channels=R.TOKEN_SIZE, _dims=dims) if stage == "enc" else vt().varlen.TiTokDecoder(in_channels=R.TOKEN_SIZE, _dims=dims)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage).items()}, strict=True)     # the reference's keys
    return m.cuda()


def _step(m, case, stage, golden):
    w_z, w_p = R.cotangents(case)
    m.zero_grad(set_to_none=True)
    if stage == "enc":
        vids = [torch.from_numpy(v).cuda().requires_grad_(True) for v in R.clips(case)]
        z = m(vids, list(R.TOKENS))
        (z * torch.from_numpy(w_z).cuda()).sum().backward()
        out = {"z": z.detach(), "d_clips": R.flat([v.grad for v in vids])}
    else:
        c = torch.from_numpy(golden[f"{case}/codes"]).cuda().requires_grad_(True)
        pred = m(c, list(R.TOKENS), [list(s) for s in R.CLIP_SIZES])
        assert [tuple(p.shape) for p in pred] == [(3,) + s for s in R.CLIP_SIZES]
        sum((p * torch.from_numpy(w).cuda()).sum() for p, w in zip(pred, w_p)).backward()
        out = {"pred": R.flat([p.detach() for p in pred]), "d_codes": c.grad}
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    out.update({"d_" + n: named[n].grad for n in R.stored_params(case, stage)})
    return out


@pytest.mark.parametrize("stage", R.STAGES)
@pytest.mark.parametrize("case", list(R.CASES))
def test_stage_matches_the_reference_within_its_own_bf16_distance(golden, case, stage):
    m = _build(case, stage)
    out = _step(m, case, stage, golden)
    failures = []
    for t in R.tensors(case, stage):
        want = torch.from_numpy(golden[f"{case}/{stage}/{t}"])
        assert out[t] is not None and tuple(out[t].shape) == tuple(want.shape) and out[t].dtype == torch.float32, t
        d, bar = R.rel_l2(out[t].cpu(), want), float(golden[f"{case}/{stage}/{t}_bf16_dist"])
        print(f"RATIO {case} {stage} {t} {d:.3e} {bar:.3e} {d / bar:.3f}")
        if not d <= 2 * bar:
            failures.append((t, d, bar))
    assert not failures, failures
    again = _step(m, case, stage, golden)                               # a second step reproduces every bit
    for t in R.tensors(case, stage):
        assert torch.equal(out[t], again[t]), t


def test_packed_equals_per_clip(golden, monkeypatch):
    """bit for bit: the row passes and GEMMs work row by row, the attention is bit-exact per sequence, the data movement is exact.  The
    automatic GEMM dispatch takes another kernel, with another summation order, for launches of at most 64 rows (the small clips here):
    all forwards are pinned to the 128x128 tile kernel so that a row's sum has one order (as in tests/test_varlen_layer_gpu.py)."""
    monkeypatch.setattr(vt().hip, "GEMM_TILE", 1)
    case = "A"
    enc, dec = _build(case, "enc"), _build(case, "dec")
    vids = [torch.from_numpy(v).cuda() for v in R.clips(case)]
    codes = torch.from_numpy(golden[f"{case}/codes"]).cuda()
    with torch.no_grad():
        z = enc(vids, list(R.TOKENS))
        pred = dec(codes, list(R.TOKENS), list(R.CLIP_SIZES))
        r0 = 0
        for b, n in enumerate(R.TOKENS):
            assert torch.equal(z[r0:r0 + n], enc([vids[b]], [n])), b
            one = dec(codes[r0:r0 + n].contiguous(), [n], [R.CLIP_SIZES[b]])
            assert len(one) == 1 and torch.equal(pred[b], one[0]), b
            r0 += n


def test_block_equals_residual_compositions():
    """one layer of ResidualAttentionBlock = x1 = x + Attn(x), then x1 + ffd(x1), bit for bit: the GEMM epilogues round first and add second"""
    V, hip = vt().varlen, vt().hip
    D, heads = 128, [2, 1]
    blk = V.ResidualAttentionBlock(D, heads, 4.0, 1)
    with torch.no_grad():
        for i, p in enumerate(blk.parameters()):
            p.copy_(torch.from_numpy(gen.normal(tuple(p.shape), 8100 + i, 0.1 if p.dim() == 1 else p.shape[-1] ** -0.5)) + (1.0 if p.dim() == 1 and i % 2 == 0 else 0.0))
    blk = blk.cuda()
    attn = V.Attn(D, heads).cuda()
    attn.load_state_dict(blk.attn_layer[0].state_dict(), strict=True)
    cu = R.cu_seqlens()
    _, cos, sin = V.rope_freqs(R.grids(), R.TOKENS, device="cuda")
    x = torch.from_numpy(gen.normal((cu[-1], D), 8200)).cuda()
    f = blk.ffd_layer[0]
    with torch.no_grad():
        got = blk(x, (cos, sin), cu, max(R.lengths()))
        x1 = x + attn(x, (cos, sin), cu, None)
        inner = f[4].in_features
        w1, _ = hip.pack_weight(f[1].weight.detach().float().contiguous())
        w2, _ = hip.pack_weight(f[4].weight.detach().float().contiguous(), k_pad=(inner + 63) // 64 * 64)
        xn, _, _ = hip.layernorm_fwd(x1, f[0].weight.detach(), f[0].bias.detach(), f[0].eps)
        a = hip.geglu_fwd(hip.gemm_nt(xn, w1, hip.EPI_BF16), lda=(inner + 63) // 64 * 64)
        y = hip.gemm_nt(a, w2, hip.EPI_F32, round_bf16=True)
        assert torch.equal(f(x1), y)                                    # the Sequential on its own is ffd(x)
        assert torch.equal(got, x1 + y)


def _small_model():
    torch.manual_seed(0)
    m = vt().TiTok(_geometry=dict(dims=DIMS_A), junk=1).cuda()
    with torch.no_grad():                                               # biases and affines away from their initial 0 / 1
        for i, p in enumerate(m.parameters()):
            if p.dim() == 1:
                p.add_(torch.from_numpy(gen.normal(tuple(p.shape), 8300 + i, 0.1)).cuda())
    return m


def test_whole_model_is_its_stages_chained():
    m = _small_model()
    sizes = [(4, 16, 16), (4, 16, 16)]
    x = [torch.from_numpy(gen.uniform((3,) + s, 8400 + i)).cuda() for i, s in enumerate(sizes)]
    counts = [m.TOKENS] * len(x)
    w = torch.from_numpy(gen.normal((len(x), 3) + sizes[0], 8500)).cuda()
    out = m(x)["pred_frames"]
    assert tuple(out.shape) == (2, 3, 4, 16, 16)
    (out * w).sum().backward()
    whole = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert all(g is not None for g in whole.values())

    x_q, info = m.encode(x, counts)
    pred = m.decode(x_q, counts, sizes)
    assert torch.equal(torch.stack(pred, 0), out)                       # forward = decode(encode(.))
    z = m.encoder(x, counts)
    codes, d = m.quantize(z)
    assert torch.equal(codes, x_q) and torch.equal(torch.cat(list(info["indices"])), d["indices"])
    assert [tuple(i.shape) for i in info["indices"]] == [(m.TOKENS,)] * 2
    again = m.decode_indices(info["indices"], sizes)
    assert all(torch.equal(a, b) for a, b in zip(again, pred))          # the codes are exact functions of the indices

    m.zero_grad(set_to_none=True)                                       # the decoder stage alone, from a leaf ...
    leaf = x_q.detach().clone().requires_grad_(True)
    (torch.stack(m.decode(leaf, counts, sizes), 0) * w).sum().backward()
    for n, p in m.decoder.named_parameters():
        assert torch.equal(p.grad, whole["decoder." + n]), n
    m.zero_grad(set_to_none=True)                                       # ... and the encoder stage with the cotangent it delivers
    codes.backward(leaf.grad)                                           # through the FSQ backward
    for n, p in m.encoder.named_parameters():
        assert torch.equal(p.grad, whole["encoder." + n]), n


def test_make_builds_the_base_geometry_whatever_the_keywords(golden):
    with torch.device("meta"):
        m = vt().make({"name": "titok", "args": dict(bottleneck=None, prior_model=None, encoder_hidden_size=3, decoder_depth=1, num_latent_tokens=5)})
    assert list(m.state_dict()) == str(golden["titok/state_dict_keys"]).split("\n")
    assert (m.encoder.width, m.encoder.num_layers, m.decoder.num_layers, m.encoder.heads, m.decoder.heads) == (768, 12, 12, [12, 4], [12, 4])
    with pytest.raises(ValueError, match="encode"):
        _small_model()([torch.zeros(3, 4, 8, 8, device="cuda"), torch.zeros(3, 4, 16, 8, device="cuda")])
