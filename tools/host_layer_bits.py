"""SHA-256 of the outputs and of every gradient of one step of each model family that runs through the Python host layer (packed weights,
stack handles and workspaces, parameter tables), for a refactor of that layer that must not change a bit: run once per tree, diff the two
listings.  One line per tensor: `<leg> <name> <sha256>`.

Legs: a `tiny` gated FSQ autoencoder (8x32x32 clips, 32 tokens); a tiny `autoencoder_design`; LARP_AR `class_S2` and `class_S2_gqa` training
step; greedy generation of `class_S2` at the three VT_AR_FUSED_DECODE levels; a 2-block BlockStack, plain and rotary.

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
