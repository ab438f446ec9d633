"""The one cache of packed weights: bf16 operand copies of a module's matrices, in the layouts the GEMM kernels read.

A pack belongs to the `nn.Module` that asks for it.  The registry is a WeakKeyDictionary on that module object, so nothing is stored in any
module's `__dict__`: copy.deepcopy(model) starts the copy empty under a new uid, torch.save(model) pickles no pack, and the entries die with
their owner.  An entry is valid for the (address, `_version`) of its source parameters and the owner's epoch.  Optimizer steps, in-place ops
under no_grad, load_state_dict and .to() change one of the first two; a write through `.data` (`p.data.copy_`, e.g. a hand-rolled EMA swap)
changes neither, which is what `invalidate` (vt.invalidate_weight_packs) is for.
"""
import itertools
import operator
import weakref

import torch

from . import hip

_UID = itertools.count(1)                    # process-wide, never reused
_OWNERS = weakref.WeakKeyDictionary()        # owning nn.Module -> _Owner


class _Owner:
    __slots__ = ("uid", "epoch", "entries")

    def __init__(self):
        self.uid, self.epoch, self.entries = next(_UID), 0, {}


def _owner(module):
    rec = _OWNERS.get(module)
    if rec is None:
        rec = _OWNERS[module] = _Owner()
    return rec


def _versions(ws):
    return tuple((w.data_ptr(), w._version) for w in ws)


def get(owner, names, k_pad=None, rows=None, interleave8=False):
    """Operand copies of the weights `names` of `owner` (attribute paths of its Linears: "wo", "ffn.1"), re-made when one of them changed.
    Several names: the weights concatenated along N (`to_q|to_gate`, `to_qkv|to_gate`, `w3|w1`).  Returns hip.pack_weight's pair
    (bf16 [N, K], bf16 [K, N]); `k_pad` zero-pads the contraction dim, `rows` (an index tensor) gathers rows first (the grouped-query
    expansion of wqkv).  interleave8: names = (w3, w1), returns ONE bf16 [2I, K] tensor with the two interleaved in slabs of 8 + 8 rows,
    the operand layout of vt_decode_norm_linear(mode 1), converted by torch."""
    rec = _owner(owner)
    ws = [operator.attrgetter(n)(owner).weight for n in names]
    key = (rec.epoch,) + _versions(ws)
    slot = (names, k_pad, rows is not None, interleave8)
    hit = rec.entries.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            ws = [w.detach() for w in ws]
            if interleave8:
                I, K = ws[1].shape
                pack = torch.cat([w.reshape(I // 8, 8, K) for w in ws], dim=1).reshape(2 * I, K).to(torch.bfloat16).contiguous()
            else:
                w = torch.cat(ws, dim=0) if len(ws) > 1 else ws[0]
                if rows is not None:
                    w = w.index_select(0, rows)
                pack = hip.pack_weight(w.float().contiguous(), k_pad=k_pad)
        hit = rec.entries[slot] = (key, pack)
    return hit[1]


def pack_key(owner, weights):
    """(uid, epoch, (address, version) ...): which weights of which module a workspace that holds packed copies was filled for
    (functional.GatedStack).  Addresses and `_version` counters alone do not identify a weight: the caching allocator hands a second model of
    the same geometry the addresses of a deleted first one, and freshly initialised parameters all carry the same version."""
    rec = _owner(owner)
    return (rec.uid, rec.epoch) + _versions(weights)


def invalidate(module):
    """Drop every pack owned by `module` or a submodule, and move their pack keys on."""
    for m in module.modules():
        rec = _OWNERS.get(m)
        if rec is not None:
            rec.epoch += 1
            rec.entries.clear()


def conv3d(owner, name, cout_abi, cin_abi, for_dgrad=False):
    """The operand image of the 3x3x3 convolution `name` of `owner` (an attribute path to an nn.Conv3d: "conv1", "downsample.conv") for
    vt_conv3d_fwd, or for vt_conv3d_dgrad (transposed, taps mirrored); channel counts zero-padded to the ABI's.  Cached like `get`."""
    rec = _owner(owner)
    w = operator.attrgetter(name)(owner).weight
    key = (rec.epoch,) + _versions([w])
    slot = ("conv3d", name, cout_abi, cin_abi, bool(for_dgrad))
    hit = rec.entries.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            pack = hip.conv3d_pack_weight(w.detach().float().contiguous(), cout_abi, cin_abi, for_dgrad)
        hit = rec.entries[slot] = (key, pack)
    return hit[1]
