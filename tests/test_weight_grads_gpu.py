"""functional._WeightGrads on the GPU, and the layer Functions with one weight frozen.

The queue: two problems with a ragged row count (M = 130) on integer-valued bf16 data, where every product and every partial sum is an
integer below 2^24, so the fp32 result has one value whatever the summation order: it must equal hip.gemm_tn_grouped on hand-padded copies
and the float64 product, both bit for bit.

Frozen subsets: with one weight frozen, every other gradient is `torch.equal` to the all-trainable run's and the frozen weight's .grad is
None.  The transposed GEMMs of one backward are separate outputs of one grouped launch, so a problem that leaves the group changes the
others only if it moves the launch to the other tile generation (vt_gemm_tn_grouped takes 192x192 tiles when every problem of the group has
at least 192 rows and columns, 128x128 tiles otherwise).  The shapes here keep the generation where it is:
  * varlen.Attn at width 128, 2 query heads on 1 K / V head, two sequences of 72 rows (M = 144, ragged): both problems have 128 columns,
    so every launch takes 128x128 tiles, whoever leaves;
  * one LARP_AR block, 2 x 72 rows, at width 384 with 6 heads -- vt_rmsnorm_* accepts the llama-abs widths only, 384 is the smallest, so
    this block cannot run at width 128: its four problems ([384, 384], [1152, 384], [384, 1024], [2048, 384]) all have at least 192 rows
    and columns, so every launch takes 192x192 tiles, whoever leaves.
CrossAttentionLayer at this geometry (width 128, 2 heads, 70 rows) is asserted by tests/test_design_gpu.py::
test_frozen_parameters_skip_their_gradient (to_q frozen beside a trainable to_gate: the half-needed concatenated weight), and
SelfAttentionLayer and FeedForwardLayer by tests/test_design_stack_gpu.py::test_stack_frozen_parameters_skip_their_gradient (to_gate frozen
beside to_qkv, out_proj, ffn.1): they are not repeated here."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_queue_pads_ragged_rows_and_equals_the_exact_product():
    import video_tokenizer_amd as vt
    from video_tokenizer_amd.functional import _WeightGrads
    g = torch.Generator().manual_seed(130)
    M, Mp = 130, 192
    shapes = ((136, 72), (200, 128))
    ops = [(torch.randint(-4, 5, (M, P), generator=g).to(torch.bfloat16).cuda(), torch.randint(-4, 5, (M, Q), generator=g).to(torch.bfloat16).cuda())
           for P, Q in shapes]
    wg = _WeightGrads()
    outs = [wg.add(dY, X) for dY, X in ops]
    wg.run()
    by_hand = []
    for (dY, X), (P, Q) in zip(ops, shapes):
        a, b = torch.zeros(Mp, P, device="cuda", dtype=torch.bfloat16), torch.zeros(Mp, Q, device="cuda", dtype=torch.bfloat16)
        a[:M].copy_(dY)
        b[:M].copy_(X)
        by_hand.append(dict(A=a, B=b, out=torch.empty(P, Q, device="cuda")))
    vt.hip.gemm_tn_grouped(by_hand)
    torch.cuda.synchronize()
    for out, job, (dY, X), (P, Q) in zip(outs, by_hand, ops, shapes):
        assert out.shape == (P, Q) and out.dtype == torch.float32
        assert torch.equal(out, job["out"]), (P, Q)
        assert torch.equal(out.cpu().double(), dY.cpu().double().t() @ X.cpu().double()), (P, Q)


# ------------------------------------------------------------------------------------------------------------------ one weight frozen
def _varlen_attn():
    import video_tokenizer_amd as vt
    torch.manual_seed(21)
    m = vt.varlen.Attn(128, [2, 1]).cuda()
    _, cos, sin = vt.varlen.rope_freqs([(2, 4, 8)] * 2, [8, 8], device="cuda")         # 8 tokens + a [2, 4, 8] grid = 72 rows, twice
    x, w = torch.randn(144, 128), torch.randn(144, 128)
    return m, lambda xi: m(xi, (cos, sin), [0, 72, 144], None), x, w


def _ar_block():
    import video_tokenizer_amd as vt
    torch.manual_seed(22)
    m = vt.larp_ar.TransformerBlock(vt.larp_ar.ModelArgs(dim=384, n_head=6), 0.0).cuda().eval()     # eval: the dropouts are identities
    x, w = torch.randn(2, 72, 384), torch.randn(2, 72, 384)
    return m, m, x, w


LAYERS = {"varlen_attn": (_varlen_attn, ("to_qkv.weight", "out_proj.weight")),                       # VarlenAttentionLayer
          "ar_block": (_ar_block, ("attention.wqkv.weight", "attention.wo.weight",                   # _AttnBranch
                                   "feed_forward.w1.weight", "feed_forward.w3.weight", "feed_forward.w2.weight"))}   # _FfnBranch


def _step(m, run, x, w):
    xi = x.cuda().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = run(xi)
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xi.grad, {n: p.grad for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def all_trainable():
    """per layer: the module, its inputs and the outputs of one step with every parameter trainable, computed once"""
    cache = {}

    def get(layer):
        if layer not in cache:
            built = LAYERS[layer][0]()
            cache[layer] = (built, _step(*built))
        return cache[layer]
    return get


@pytest.mark.parametrize("layer,frozen", [(layer, n) for layer, (_, names) in LAYERS.items() for n in names])
def test_one_frozen_weight_leaves_the_other_gradients_their_bits(all_trainable, layer, frozen):
    (m, run, x, w), (y, dx, full) = all_trainable(layer)
    assert all(g is not None for g in full.values())
    m.get_parameter(frozen).requires_grad_(False)
    try:
        y2, dx2, part = _step(m, run, x, w)
    finally:
        m.get_parameter(frozen).requires_grad_(True)
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    for n in full:
        if n == frozen:
            assert part[n] is None, n
        else:
            assert torch.equal(part[n], full[n]), n
