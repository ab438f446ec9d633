"""SHA-256 of the outputs and of every gradient of one step of each model family that runs through the Python host layer (packed weights,
stack handles and workspaces, parameter tables), for a refactor of that layer that must not change a bit: run once per tree, diff the two
listings.  One line per tensor: `<leg> <name> <sha256>`.

Legs: a `tiny` gated FSQ autoencoder (8x32x32 clips, 32 tokens); a tiny `autoencoder_design`; LARP_AR `class_S2` and `class_S2_gqa` training
step; greedy generation of `class_S2` at the three VT_AR_FUSED_DECODE levels; a 2-block BlockStack, plain and rotary.  For the layer Functions'
weight-gradient queue (functional._WeightGrads): `varlen.Attn` on a ragged packed batch (M = 130); a tiny `autoencoder_stat` step; Bottleneck
and PatchEmbed3D on their own at M = 72; one design block with cross attention, all trainable, with cross_attn.to_gate frozen and with
self_attn.to_qkv frozen; the `class_S2` step with one w1 frozen.  For the patch ends (csrc/vt_patch.hip, vt_packed.hip and their Functions): a tiny
`autoencoder_dualpatch` step and a small packed `titok` step on two clips of different sizes.

  python tools/host_layer_bits.py > listing.txt
  python tools/host_layer_bits.py --flat-order > order.txt      (no GPU: engine._flat_order of configs `tiny` and `B`)
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import video_tokenizer_amd as vt  # noqa: E402
from oracle import ar_oracle as A  # noqa: E402
from oracle import inputs as gen  # noqa: E402
from oracle import titok_oracle as T  # noqa: E402
from tests.golden.make_golden import ar_cases, ar_inputs  # noqa: E402


# torch's own glue must repeat too: the gradient of the grouped-query row gather of wqkv is an index_add, summed with atomics by default
torch.use_deterministic_algorithms(True, warn_only=True)
torch.utils.deterministic.fill_uninitialized_memory = False


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def report(leg, out, model=None, extra=()):
    torch.cuda.synchronize()
    print(leg, "out", sha(out))
    for name, t in extra:
        print(leg, name, sha(t))
    if model is not None:
        for name, p in model.named_parameters():
            print(leg, "grad:" + name, "none" if p.grad is None else sha(p.grad))


def gated_autoencoder():
    cfg = T.make_cfg("tiny", frames=8, side=32, tokens=32)
    cls = type("AutoEncoderTiny", (vt.titok._AutoEncoderBase,), dict(MODEL_SIZE="tiny", LEVELS=list(cfg["levels"])))
    m = cls(bottleneck=None, prior_model=None, _geometry=dict(in_grid=[8, 32, 32], patch_size=cfg["patch"], tokens=32))
    m.load_state_dict(T.init_state_dict(cfg), strict=True)
    m = m.cuda()
    video = torch.from_numpy(gen.video_clips(2, 8, 32, 620)).cuda()
    up = torch.from_numpy(gen.normal((2, 3, 8, 32, 32), 621)).cuda()
    for leg in ("gated_ae", "gated_ae_second_step"):          # the second step runs on the pooled workspaces and the kept packs
        for p in m.parameters():
            p.grad = None
        out = m(video)["pred_frames"]
        (out * up).sum().backward()
        report(leg, out, m)


def design_autoencoder():
    torch.manual_seed(3)
    m = vt.make({"name": "autoencoder_design", "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        in_grid=[4, 32, 32], patch_size=[4, 8, 8], tokens=8, cond_tokens=4, model_size="tiny")}}).cuda()
    video = torch.from_numpy(gen.video_clips(2, 4, 32, 901).astype("float32")).cuda()
    up = torch.from_numpy(gen.normal((2, 3, 4, 32, 32), 902)).cuda()
    for leg in ("design_ae", "design_ae_second_step"):
        for p in m.parameters():
            p.grad = None
        out = m(video)["pred_frames"]
        (out * up).sum().backward()
        report(leg, out, m)


def ar_model(name):
    kw, B, seed = ar_cases()[name]
    cfg = A.make_cfg(**kw)
    m = vt.LARP_AR(vt.larp_ar.ModelArgs(dim=cfg["dim"], n_layer=cfg["n_layer"], n_head=cfg["n_head"], n_kv_head=cfg["n_kv_head"],
                                        vocab_size=cfg["vocab_size"], max_seq_len=cfg["max_seq_len"], num_classes=cfg["num_classes"],
                                        cls_token_num=cfg["cls_token_num"], frame_prediction=cfg["frame_prediction"], use_fixed_pe=cfg["use_fixed_pe"],
                                        token_dropout_p=0.0, resid_dropout_p=0.0, ffn_dropout_p=0.0, class_dropout_prob=0.1))
    m.load_state_dict(A.init_state_dict(cfg, seed), strict=True)
    tok, cond = ar_inputs(cfg, B, seed)
    return m.cuda(), cfg, tok.cuda(), cond.cuda()


def ar_training(name):
    m, cfg, tok, cond = ar_model(name)
    m.train()
    m.cls_embedding.dropout_prob = 0.0
    logits, loss = m(tok[:, :-1], cond, targets=tok)
    loss.backward()
    report("ar_train_" + name, logits, m, extra=[("loss", loss)])


def ar_generation():
    m, cfg, tok, cond = ar_model("class_S2")
    m.eval()
    for level in ("0", "swiglu", "norm"):
        os.environ["VT_AR_FUSED_DECODE"] = level
        with m.sampling():
            seq = vt.larp_ar.generate(m, cond, cfg["max_seq_len"], cfg_scale=3.0, cfg_interval=20, use_graph=False, temperature=1.0, top_k=0,
                                      top_p=1.0, sample_logits=False)
        m.reset_caches()
        report("ar_generate_fused_" + level, seq)
    del os.environ["VT_AR_FUSED_DECODE"]


def block_stacks():
    torch.manual_seed(11)
    blocks = torch.nn.ModuleList([vt.titok.SimpleBlock(128, 2) for _ in range(2)]).cuda()
    x = torch.from_numpy(gen.normal((2, 72, 128), 1801, 1.0)).cuda()           # 72 rows: 8 latents + the grid [2, 4, 8]
    up = torch.from_numpy(gen.normal((2, 72, 128), 1802, 1.0)).cuda()
    cos, sin = (t.cuda() for t in vt.titok.rope_tables(8, [2, 4, 8]))
    for leg, run in (("block_stack_plain", lambda xi: vt.functional.block_stack(xi, blocks, 2)),
                     ("block_stack_rotary", lambda xi: vt.functional.rotary_block_stack(xi, blocks, 2, cos, sin))):
        for p in blocks.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        out = run(xi)
        (out * up).sum().backward()
        report(leg, out, blocks, extra=[("dx", xi.grad)])


def step(leg, model, run, x, up, extra=()):
    """one forward + backward of run(*x) under the loss sum(out * up), from cleared gradients; the inputs' gradients are listed as dx0, dx1, ..."""
    for p in model.parameters():
        p.grad = None
    xs = [t.clone().requires_grad_(True) for t in x]
    out = run(*xs)
    (out * up).sum().backward()
    report(leg, out, model, extra=[(f"dx{i}", t.grad) for i, t in enumerate(xs)] + list(extra))


def normal(shape, seed):
    return torch.from_numpy(gen.normal(shape, seed, 1.0)).cuda()


def varlen_attn():
    """varlen.Attn on a ragged packed batch: sequences of 40 and 90 rows, M = 130, so both weight-gradient problems are row-padded"""
    torch.manual_seed(12)
    m = vt.varlen.Attn(128, [2, 1]).cuda()
    _, cos, sin = vt.varlen.rope_freqs([(2, 4, 4), (5, 4, 4)], [8, 10], device="cuda")
    step("varlen_attn_ragged", m, lambda x: m(x, (cos, sin), [0, 40, 130], None), [normal((130, 128), 1901)], normal((130, 128), 1902))


def stat_autoencoder():
    """a tiny `autoencoder_stat` training step ('adaptive' stage): StatGate, Linear and ConvTransposePatch"""
    from tests import stat_reference as S
    cfg = S.make_cfg("tiny")
    m = vt.make({"name": "autoencoder_stat", "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        in_grid=[cfg["frames"], cfg["side"], cfg["side"]], patch_size=cfg["patch"], tokens=cfg["tokens"], model_size=cfg["size"])}})
    m.load_state_dict(S.init_state_dict(cfg), strict=True)
    m = m.cuda().train()
    torch.manual_seed(13)
    video = torch.from_numpy(gen.video_clips(2, 8, 32, 1911)).cuda()
    up, a, c = normal((2, 3, 8, 32, 32), 1912), normal((2, 32), 1913), normal((2, 32), 1914)
    out = m(video, current_epoch=0)
    ((out["pred_frames"] * up).sum() + (out["probs"] * a).sum() + (out["mask"] * c).sum()).backward()
    report("stat_ae", out["pred_frames"], m, extra=[("probs", out["probs"]), ("mask", out["mask"])])


def ragged_projections():
    """Bottleneck (two functional.Linear around the quantizer) and PatchEmbed3D on their own with M = 2 x 36 = 72 rows: their row padding"""
    torch.manual_seed(14)
    b = vt.bottleneck.Bottleneck(16, 128, 128, 36, regularizer={"name": "vq", "args": dict(codebook_size=64, l2_normalized=True)}).cuda()
    up, wq = normal((2, 36, 128), 1922), normal((3,), 1923)

    def bottleneck(x):
        o = b(x)
        return o["output"] + (wq[0] * o["loss_q"] + wq[1] * o["loss_commit"] + wq[2] * o["loss_codebook"]) / up.sum()
    step("bottleneck_ragged", b, bottleneck, [normal((2, 36, 128), 1921)], up)
    pe = vt.embed.PatchEmbed3D(spatial_vid_size=48, temporal_vid_size=4, spatial_patch_size=8, temporal_patch_size=4, embed_dim=128).cuda()
    pos = normal((36, 128), 1933)
    step("patch_embed_ragged", pe, lambda v: pe(v, pos), [normal((2, 3, 4, 48, 48), 1931)], normal((2, 36, 128), 1932))
    step("patch_embed_ragged_no_pos", pe, pe, [normal((2, 3, 4, 48, 48), 1931)], normal((2, 36, 128), 1932))


def design_blocks_half_frozen():
    """one design block with cross attention, 2 x 72 rows: one half of a concatenated weight frozen, the other trainable -- one queued
    problem, one slice returned, one None"""
    cos, sin = (t.cuda() for t in vt.titok.rope_tables(8, [2, 4, 8]))
    x, ctx, up = normal((2, 72, 128), 1941), normal((2, 33, 128), 1942), normal((2, 72, 128), 1943)
    for leg, frozen in (("design_block", ()), ("design_block_cross_gate_frozen", ("cross_attn.to_gate.weight",)),
                        ("design_block_self_qkv_frozen", ("self_attn.to_qkv.weight",))):
        torch.manual_seed(15)
        blk = vt.design.TransformerBlock(128, 2, has_cross_attn=True).cuda()
        for n in frozen:
            blk.get_parameter(n).requires_grad_(False)
        step(leg, blk, lambda xi, ci: blk(xi, (cos, sin), context=ci), [x, ctx], up)


def ar_training_w1_frozen():
    """the class_S2 training step with the first block's w1 frozen beside a trainable w3 (the halves of _FfnBranch's concatenated weight)"""
    m, cfg, tok, cond = ar_model("class_S2")
    m.train()
    m.cls_embedding.dropout_prob = 0.0
    m.layers[0].feed_forward.w1.weight.requires_grad_(False)
    logits, loss = m(tok[:, :-1], cond, targets=tok)
    loss.backward()
    report("ar_train_class_S2_w1_frozen", logits, m, extra=[("loss", loss)])


def dualpatch_autoencoder():
    """a tiny `autoencoder_dualpatch` step (case A of tests/dualpatch_reference.py: 7 frames of 32 x 64, a one-frame first segment): DualPatchEmbed
    and DualConvTransposePatch, both weight gradients of each in one grouped launch"""
    from tests import dualpatch_reference as D
    c = D.CASES["A"]
    torch.manual_seed(16)
    m = vt.make({"name": "autoencoder_dualpatch", "args": {"bottleneck": None, "prior_model": None, "_geometry": dict(
        dims=c["dims"], tokens=c["tokens"], **D.geometry("A"))}}).cuda()
    step("dualpatch_ae", m, lambda v: m(v)["pred_frames"], [torch.from_numpy(D.video("A")).cuda()], normal(D.video_shape("A"), 1951))


def titok_packed():
    """a small packed `titok` step on two clips of different sizes through encode / decode: PatchRowsClips and UnpatchifyClips"""
    from tests import titok_reference as K
    torch.manual_seed(17)
    m = vt.TiTok(_geometry=dict(dims=K.CASES["A"]["dims"])).cuda()
    sizes, counts = [(4, 16, 16), (8, 16, 24)], [24, 40]
    ups = [normal((3,) + s, 1962 + i) for i, s in enumerate(sizes)]

    def run(*clips):
        x_q, _ = m.encode(list(clips), counts)
        return torch.cat([(p * u).reshape(-1) for p, u in zip(m.decode(x_q, counts, sizes), ups)])
    step("titok_packed", m, run, [torch.from_numpy(gen.uniform((3,) + s, 1960 + i)).cuda() for i, s in enumerate(sizes)], 1.0)


def flat_order():
    """--flat-order (no GPU needed): (stage, name) of engine._flat_order, the layout of the flat gradient buffer and of the all-reduce slices"""
    from video_tokenizer_amd.engine import _flat_order
    for name in ("tiny", "B"):
        m = vt.make(vt.config.model_spec(vt.config.geometry(name)))
        for n, _, stage in _flat_order(m):
            print("flat_order", name, stage, n)


if __name__ == "__main__":
    if "--flat-order" in sys.argv:
        flat_order()
        sys.exit(0)
    gated_autoencoder()
    design_autoencoder()
    ar_training("class_S2")
    ar_training("class_S2_gqa")
    ar_generation()
    block_stacks()
    varlen_attn()
    stat_autoencoder()
    ragged_projections()
    design_blocks_half_frozen()
    ar_training_w1_frozen()
    dualpatch_autoencoder()
    titok_packed()
