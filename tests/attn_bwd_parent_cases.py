"""The non-causal attention backward against the bits of the commit before its dQ and dK/dV workgroups shared a launch.

Shared by tests/golden/make_golden_attn_bwd_parent.py (run once, on a GPU, under the PARENT commit's library) and
tests/test_attention_bwd_one_launch_gpu.py (the tree's library, every run).  Nothing in that change reorders a sum, so every output --
dqkv (or dq, dk, dv) and the delta workspace -- must keep every bit.

Inputs are integer hashes (oracle/inputs.hash_u64) mapped to k / 32, |k| <= 64: exact in bf16 and the same on every machine, so only
outputs are committed.  o and lse2 come from the library's own forward at run time (the forward kernel is not part of the change).
The entry points are called through the C ABI, because the op wrappers of video_tokenizer_amd.hip do not hand back the delta workspace.

A case's arrays are cut into row chunks and dealt to tests/golden/attn_bwd_parent_<case>_<i>.npz so that every file stays below 256 KB;
`load` puts them together again."""
import glob
import os

import numpy as np
import torch

from oracle import inputs as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILE_LIMIT = 256 << 10
CHUNK_BYTES = 64 << 10       # raw bytes of one row chunk
FILE_RAW_BYTES = 192 << 10   # raw bytes dealt to one file (compression only shrinks it)

# name -> (path, B, H, Lq, Lk, hd, q_begin); what each covers:
#   p130   6 workgroups per role (not a multiple of 8: the dQ role's chunks sit on a rotated set of XCDs); ragged 64-tile; a 2-row last block
#   p40    L < 64; a grid of 2
#   rows   n_dq = 4, n_dkv = 8; compact o / dO; zeroed dQ rows
#   hd32   the other head dimension
#   cross  n_dq = 4, n_dkv = 12; separate strides
CASES = {
    "p130": ("packed", 1, 3, 130, 130, 64, 0),
    "p40": ("packed", 1, 1, 40, 40, 64, 0),
    "rows": ("packed", 2, 2, 192, 192, 64, 64),
    "hd32": ("packed", 1, 5, 257, 257, 32, 0),
    "cross": ("cross", 2, 2, 70, 300, 64, 0),
}


def grid_values(rows, cols, seed):
    """bf16 [rows, cols] of k / 32, k = -64 .. 64 from the integer hash: no floating-point step on the way"""
    k = (gen.hash_u64(rows * cols, seed) % np.uint64(129)).astype(np.int64) - 64
    return torch.from_numpy((k.astype(np.float32) / 32.0).reshape(rows, cols)).to(torch.bfloat16)


def bits(t):
    """a device tensor's bits: bf16 -> uint16, fp32 stays fp32 (compared through its int32 view)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def run(hip, name):
    """-> {array name: bits} of one backward under the library that `hip` loaded"""
    path, B, H, Lq, Lk, hd, q_begin = CASES[name]
    D = H * hd
    seed = 7100 + 10 * list(CASES).index(name)
    L = hip.lib()
    if path == "packed":
        qkv = grid_values(B * Lq, 3 * D, seed).cuda()
        dO = grid_values(B * (Lq - q_begin), D, seed + 1).cuda()
        o, lse2 = hip.attention_fwd(qkv, B, Lq, H, hd, q_begin=q_begin)
        dqkv = torch.full_like(qkv, -7.0)
        delta = torch.zeros(B, H, Lq, device="cuda", dtype=torch.float32)
        hip.check(L.vt_attention_bwd_rows(hip.ptr(qkv), hip.ptr(o), hip.ptr(dO), hip.ptr(lse2), B, Lq, H, hd, q_begin, hip.ptr(dqkv), hip.ptr(delta),
                                          hip.stream()), "vt_attention_bwd_rows")
        torch.cuda.synchronize()
        return {"dqkv": bits(dqkv), "delta": bits(delta)}
    # cross: q = columns 0..D of a [B Lq, 2D] buffer, k and v = the two halves of one [B Lk, 2D] buffer; dq dense, dk / dv the halves of one buffer
    qbuf = grid_values(B * Lq, 2 * D, seed).cuda()
    kvbuf = grid_values(B * Lk, 2 * D, seed + 1).cuda()
    dO = grid_values(B * Lq, D, seed + 2).cuda()
    q, k, v = qbuf[:, :D], kvbuf[:, :D], kvbuf[:, D:]
    o, lse2 = hip.attention_cross_fwd(q, k, v, B, Lq, Lk, H, hd)
    dq = torch.full((B * Lq, D), -7.0, device="cuda", dtype=torch.bfloat16)
    dkv = torch.full((B * Lk, 2 * D), -7.0, device="cuda", dtype=torch.bfloat16)
    delta = torch.zeros(B, H, Lq, device="cuda", dtype=torch.float32)
    hip.check(L.vt_attention_cross_bwd(hip.ptr(q), q.stride(0), hip.ptr(k), k.stride(0), hip.ptr(v), v.stride(0), hip.ptr(o), hip.ptr(dO), hip.ptr(lse2),
                                       B, Lq, Lk, H, hd, hip.ptr(dq), dq.stride(0), hip.ptr(dkv[:, :D]), dkv.stride(0), hip.ptr(dkv[:, D:]), dkv.stride(0),
                                       hip.ptr(delta), hip.stream()), "vt_attention_cross_bwd")
    torch.cuda.synchronize()
    return {"dq": bits(dq), "dk": bits(dkv[:, :D]), "dv": bits(dkv[:, D:]), "delta": bits(delta)}


def files_of(name):
    return sorted(glob.glob(os.path.join(GOLDEN, f"attn_bwd_parent_{name}_*.npz")))


def save(name, arrays):
    """row chunks `<array>.<index>` dealt to attn_bwd_parent_<name>_<i>.npz in order"""
    for f in files_of(name):
        os.remove(f)
    chunks = []
    for key, a in arrays.items():
        a2 = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)
        step = max(1, CHUNK_BYTES // max(1, a2.shape[1] * a2.itemsize))
        chunks += [(f"{key}.{i:03d}", a2[r:r + step]) for i, r in enumerate(range(0, a2.shape[0], step))]
        chunks.append((f"{key}.shape", np.array(a.shape, dtype=np.int64)))
    files, size = [{}], 0
    for key, c in chunks:
        if size and size + c.nbytes > FILE_RAW_BYTES:
            files.append({})
            size = 0
        files[-1][key] = c
        size += c.nbytes
    for i, d in enumerate(files):
        fn = os.path.join(GOLDEN, f"attn_bwd_parent_{name}_{i}.npz")
        np.savez_compressed(fn, **d)
        assert os.path.getsize(fn) < FILE_LIMIT, (fn, os.path.getsize(fn))
    return len(files)


def load(name):
    fs = files_of(name)
    assert fs, f"no fixture for {name}: run tests/golden/make_golden_attn_bwd_parent.py under the parent commit's library"
    parts = {}
    for f in fs:
        assert os.path.getsize(f) < FILE_LIMIT
        with np.load(f) as z:
            parts.update({k: z[k] for k in z.files})
    out = {}
    for key in sorted(k[:-6] for k in parts if k.endswith(".shape")):
        rows = [parts[k] for k in sorted(parts) if k.startswith(key + ".") and not k.endswith(".shape")]
        out[key] = np.concatenate(rows, 0).reshape(tuple(parts[key + ".shape"]))
    return out
