"""packs.py, the registry of packed weights, on the CPU: `vt.hip.pack_weight` is replaced by a counting torch stand-in, so every look-up the
model families make (one weight, weights concatenated along N, a padded contraction dim, the grouped-query row gather, the 8 + 8-row
w3 / w1 interleave of the decode GEMM) runs without a GPU.  What is pinned: when a pack is re-made, who owns it, and that it lives nowhere
but in the registry."""
import copy
import gc
import pickle

import pytest
import torch
from torch import nn

import video_tokenizer_amd as vt
from video_tokenizer_amd import larp_ar, packs


@pytest.fixture
def packed(monkeypatch):
    """the shapes hip.pack_weight was called with; the stand-in returns (bf16 [N, k_pad or K], its transpose)"""
    calls = []

    def pack_weight(w, k_pad=None):
        calls.append(tuple(w.shape))
        wb = torch.zeros(w.shape[0], k_pad or w.shape[1], dtype=torch.bfloat16)
        wb[:, :w.shape[1]] = w
        return wb, wb.t().contiguous()

    monkeypatch.setattr(vt.hip, "pack_weight", pack_weight)
    return calls


def ar_model():
    """one grouped-query block of LARP_AR: 2 query heads on 1 K / V head, width 128, hidden 512"""
    torch.manual_seed(0)
    m = vt.LARP_AR(larp_ar.ModelArgs(dim=128, n_layer=1, n_head=2, n_kv_head=1, vocab_size=32, max_seq_len=8, num_classes=3))
    return m, m.layers[0].attention, m.layers[0].feed_forward


def design_block():
    torch.manual_seed(0)
    return vt.design.TransformerBlock(128, 2)          # ffn inner width 352, padded to 384 for the contraction


def first(pack):
    """the [N, K] operand of a pack (the interleaved SwiGLU pack is that tensor alone)"""
    return pack if torch.is_tensor(pack) else pack[0]


def bf16(t):
    return t.detach().to(torch.bfloat16)


# kind -> (model, look-up as the product spells it, the source weight a test writes to, that weight's rows inside the [N, K] operand)
def kinds():
    m, at, ff = ar_model()
    blk = design_block()
    I = ff.w1.weight.shape[0]
    w1_rows = (torch.arange(I) // 8) * 16 + 8 + torch.arange(I) % 8        # w1 row i sits behind the 8 w3 rows of its slab
    return {"single": (m, lambda: larp_ar._pack(at, "wo"), at.wo.weight, slice(None)),
            "concatenated": (m, lambda: larp_ar._pack(ff, "w3", "w1"), ff.w1.weight, slice(I, 2 * I)),
            "k_pad": (blk, lambda: packs.get(blk, ("ffn.3",), k_pad=384), blk.ffn[3].weight, slice(None)),
            "gqa": (m, lambda: larp_ar._pack_qkv(at), at.wqkv.weight, at._gqa_rows),
            "swiglu": (m, lambda: larp_ar._pack_swiglu(ff), ff.w1.weight, w1_rows)}


def holds(pack, weight, rows):
    """the operand's rows `rows` are the bf16 values of `weight` (of its gathered rows, for the grouped-query pack)"""
    got = first(pack)
    if torch.is_tensor(rows) and rows.numel() != weight.shape[0]:          # gqa: operand = weight[rows]
        return torch.equal(got, bf16(weight)[rows])
    return torch.equal(got[rows][:, :weight.shape[1]], bf16(weight))


@pytest.mark.parametrize("kind", ["single", "concatenated", "k_pad", "gqa", "swiglu"])
def test_two_lookups_make_one_pack(packed, kind):
    model, look, w, rows = kinds()[kind]
    a, b = look(), look()
    assert a is b and holds(a, w, rows)
    assert len(packed) == (0 if kind == "swiglu" else 1)                    # the SwiGLU interleave is converted by torch
    if kind == "k_pad":
        assert a[0].shape == (128, 384) and a[1].shape == (384, 128) and float(a[0][:, 352:].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["single", "concatenated", "k_pad", "gqa", "swiglu"])
def test_version_bumps_remake_the_pack(packed, kind):
    model, look, w, rows = kinds()[kind]
    a = look()
    with torch.no_grad():
        w.mul_(2.0)                                                         # in place under no_grad: what an optimizer step does
    b = look()
    assert b is not a and holds(b, w, rows) and not torch.equal(first(a), first(b))
    sd = {k: v * 0.5 for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    c = look()
    assert c is not b and holds(c, w, rows) and not torch.equal(first(c), first(b))
    assert c is look()


@pytest.mark.parametrize("kind", ["single", "concatenated", "k_pad", "gqa", "swiglu"])
def test_data_write_needs_invalidate_weight_packs(packed, kind):
    """`p.data.copy_` bumps no version: the pack stays (stale) until vt.invalidate_weight_packs(model).  On the parent of the registry the
    grouped-query and SwiGLU copies stayed stale even then."""
    model, look, w, rows = kinds()[kind]
    a = look()
    version = w._version
    w.data.copy_(w.data * 1.5)
    assert w._version == version
    assert look() is a and not holds(a, w, rows)
    vt.invalidate_weight_packs(model)
    b = look()
    assert b is not a and holds(b, w, rows)
    assert look() is b


def test_deepcopy_starts_empty_under_a_new_uid(packed):
    m, at, ff = ar_model()
    a = larp_ar._pack(at, "wo")
    key = packs.pack_key(at, [at.wo.weight])
    m2 = copy.deepcopy(m)
    at2 = m2.layers[0].attention
    assert all(mod not in packs._OWNERS for mod in m2.modules())            # the copy has no entries
    at2.wo.weight.data.copy_(at2.wo.weight.data * 3.0)                      # (no version bump: a copied entry would still match)
    n = len(packed)
    b = larp_ar._pack(at2, "wo")
    assert len(packed) == n + 1 and b is not a and holds(b, at2.wo.weight, slice(None)) and not holds(b, at.wo.weight, slice(None))
    assert larp_ar._pack(at, "wo") is a                                     # the original keeps its own
    key2 = packs.pack_key(at2, [at2.wo.weight])
    assert key2[0] != key[0] and key2[1] == 0


def test_entries_die_with_their_owner_and_uids_are_never_reused(packed):
    gc.collect()
    assert len(packs._OWNERS) == 0, "an earlier test leaked an owner"
    m, at, ff = ar_model()
    larp_ar._pack(at, "wo"), larp_ar._pack_qkv(at), larp_ar._pack_swiglu(ff), larp_ar._pack(m, "output")
    seen = [packs.pack_key(mod, [])[0] for mod in (at, ff, m)]
    assert len(packs._OWNERS) == 3 and len(set(seen)) == 3
    del m, at, ff
    gc.collect()
    assert len(packs._OWNERS) == 0
    later = nn.Linear(4, 4)
    assert packs.pack_key(later, [later.weight])[0] > max(seen)


def test_no_pack_in_any_module_dict_or_pickle(packed):
    m, at, ff = ar_model()
    blk = design_block()
    dicts = {id(mod): set(mod.__dict__) for root in (m, blk) for mod in root.modules()}
    size = len(pickle.dumps(m)), len(pickle.dumps(blk))
    for look in (lambda: larp_ar._pack(at, "wo"), lambda: larp_ar._pack(ff, "w3", "w1"), lambda: larp_ar._pack_qkv(at), lambda: larp_ar._pack_swiglu(ff),
                 lambda: larp_ar._pack(m, "output"), lambda: packs.get(blk, ("ffn.1",)), lambda: packs.get(blk, ("ffn.3",), k_pad=384),
                 lambda: packs.get(blk.self_attn, ("to_qkv", "to_gate"))):
        assert look() is look()
    packs.pack_key(blk, [blk.ffn[1].weight])
    for root in (m, blk):
        for mod in root.modules():
            assert set(mod.__dict__) == dicts[id(mod)], type(mod).__name__
            assert not any("pack" in k for k in mod.__dict__)
    assert (len(pickle.dumps(m)), len(pickle.dumps(blk))) == size


def test_two_owners_of_the_same_parameters_get_different_keys(packed):
    lin = nn.Linear(8, 8, bias=False)
    one, two = nn.Sequential(lin), nn.Sequential(lin)
    k1, k2 = packs.pack_key(one, [lin.weight]), packs.pack_key(two, [lin.weight])
    assert k1 != k2 and k1[2:] == k2[2:] == ((lin.weight.data_ptr(), lin.weight._version),)
    assert packs.pack_key(one, [lin.weight]) == k1                          # stable while nothing changes
    packs.invalidate(one)
    assert packs.pack_key(one, [lin.weight]) == (k1[0], k1[1] + 1) + k1[2:] and packs.pack_key(two, [lin.weight]) == k2
