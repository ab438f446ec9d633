"""SHA-256 of every output of a fixed list of calls into the row kernels (csrc/vt_layernorm.hip, vt_rows.hip, vt_pack.hip), for the library
named by VT_HIP_LIB (default: the tree's build).  The check of a refactor that must not change a bit: run it once per library, each in its
own process, and diff the two outputs.
usage: VT_HIP_LIB=video-tokenizer_amd/_ab/libvt_base.so python tools/row_output_hashes.py > parent.txt; python tools/row_output_hashes.py > tree.txt
The cases: LayerNorm forward and backward at all six widths, dense and through a row map, with and without dres, the bf16 copy of dx and
dxsum, at 508 and 509 rows (127 and 128 slabs: the 8-lane and the 32-lane reducer); vt_colsum of bf16 and fp32; vt_batch_sum, vt_cast_rows,
vt_zero_rows, vt_assemble_rows; vt_sum_slabs at 8 and at 32 lanes; vt_scale_rows; vt_pack_weight with aligned and ragged extents, a row
permutation, wb only and wt only; vt_pack_weights_grouped on the 40 jobs of tests/test_ops_gpu.py.  Every destination is zeroed first, so
a hash covers padding and unmapped rows too."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import video_tokenizer_amd.hip as hip  # noqa: E402

DIMS = (128, 256, 384, 512, 768, 1024)


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def show(name, **outs):
    torch.cuda.synchronize()
    print(name, " ".join(f"{k}={sha(v)}" for k, v in outs.items()), flush=True)


def layernorm(dim, rows, rmap):
    grp, stride, off = rmap or (rows, rows, 0)
    phys = (rows + grp - 1) // grp * stride
    xmap = hip.RowMap(grp, stride, off) if rmap else None
    x, gamma, beta = rand((phys, dim), dim + rows), rand((dim,), 2) + 1.0, rand((dim,), 3)
    y, mean, rstd = hip.layernorm_fwd(x, gamma, beta, 1e-5, rows=rows, xmap=xmap)
    name = f"layernorm dim={dim} rows={rows} map={rmap}"
    show(name + " fwd", y=y, mean=mean, rstd=rstd)
    dy, dres = rand((rows, dim), 4, torch.bfloat16), rand((phys, dim), 5)
    for use_dres, want_dxb, want_dxsum in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        dx = torch.zeros_like(x)
        dxb = torch.zeros(phys, dim, dtype=torch.bfloat16, device="cuda") if want_dxb else None
        dx, dxb, dg, db, ds = hip.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres if use_dres else None, xmap=xmap, dx=dx, dxb=dxb,
                                                want_dxsum=want_dxsum, want_dxb=want_dxb)
        show(name + f" bwd dres={int(use_dres)} dxb={int(want_dxb)} dxsum={int(want_dxsum)}", dx=dx, dxb=dxb, dgamma=dg, dbeta=db, dxsum=ds)


def rows_cases():
    for dtype in (torch.bfloat16, torch.float32):
        src = rand((1000, 776), 11, dtype)
        show(f"colsum {dtype} 1000x768 ld=776", out=hip.colsum(src[:, :768]))
        show(f"colsum {dtype} 5000x776", out=hip.colsum(src.repeat(5, 1)))
        show(f"colsum {dtype} row map", out=hip.colsum(src, rows=300, rmap=hip.RowMap(50, 160, 30)))
    src = rand((4 * 100, 256), 12)
    show("batch_sum 4x40x256 row map", out=hip.batch_sum(src, 4, 40, rmap=hip.RowMap(40, 100, 60)))
    show("batch_sum 4x100x256", out=hip.batch_sum(src, 4, 100))
    show("cast_rows dense", out=hip.cast_rows(src))
    show("cast_rows row map ldd=264", out=hip.cast_rows(src, rows=160, rmap=hip.RowMap(40, 100, 60), ldd=264))
    a, b = src.clone(), src.to(torch.bfloat16)
    hip.zero_rows(a, b, rows=160, rmap=hip.RowMap(40, 100, 60))
    show("zero_rows both, row map", a=a, b=b)
    a = src.clone()
    hip.zero_rows(a, None, rows=7)
    show("zero_rows fp32 only", a=a)
    dst = torch.zeros(3 * 100, 256, device="cuda")
    hip.assemble_rows(dst, 100, 60, 3, 40, src=rand((120, 256), 13), table=rand((40, 256), 14), vec=rand((256,), 15))
    hip.assemble_rows(dst, 100, 0, 3, 60, table=rand((60, 256), 16))
    hip.assemble_rows(dst, 100, 0, 3, 1, vec=rand((256,), 17))
    show("assemble_rows src+table+vec, table, vec", dst=dst)
    slabs = rand((300, 1000), 18)
    for nslab in (1, 127, 128, 300):        # 8 lanes below 128 slabs, 32 from there on
        show(f"sum_slabs nslab={nslab} width=777 stride=1000", out=hip.sum_slabs(slabs, nslab, 777, slab_stride=1000))
    f, h = torch.zeros(100, 72, device="cuda"), torch.zeros(100, 72, dtype=torch.bfloat16, device="cuda")
    hip.scale_rows(rand((100, 72), 19), 0.37, dst=f, dstb=h)
    show("scale_rows 100x72", dst=f, dstb=h)
    big = rand((4096, 384), 20)
    hip.scale_rows(big, -1.5, dst=big)
    show("scale_rows 4096x384 in place", dst=big)


def pack_single(N, K, perm=False, want_b=True, want_t=True, pad=8):
    w = rand((N, K), 100 * N + K)
    rp = torch.randperm(N, generator=torch.Generator().manual_seed(N)).to(torch.int32).cuda() if perm else None
    wb = torch.zeros(N, K + pad, dtype=torch.bfloat16, device="cuda") if want_b else None
    wt = torch.zeros(K, N + pad, dtype=torch.bfloat16, device="cuda") if want_t else None
    hip.check(hip.lib().vt_pack_weight(hip.ptr(w), N, K, hip.ptr(rp), hip.ptr(wb), K + pad, hip.ptr(wt), N + pad, hip.stream()), "vt_pack_weight")
    show(f"pack_weight {N}x{K} perm={int(perm)} pad={pad}", wb=wb, wt=wt)


def pack_grouped(ragged):
    """the job list of tests/test_ops_gpu.py::test_pack_weights_grouped_equals_single_packs"""
    shapes = [(768, 768), (2304, 768), (24, 768), (768, 24), (100, 36)] * 8
    if ragged:
        shapes[3], shapes[37] = (33, 50), (7, 129)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(0)).to(torch.int32).cuda()
    jobs, keep = (hip.PackJob * len(shapes))(), []
    for i, (N, K) in enumerate(shapes):
        w = rand((N, K), 400 + i)
        wb = torch.zeros(N, K + 8, dtype=torch.bfloat16, device="cuda")
        wt = torch.zeros(K, N + 8, dtype=torch.bfloat16, device="cuda") if i % 3 else None
        j = jobs[i]
        j.w, j.N, j.K, j.row_perm = w.data_ptr(), N, K, (perm.data_ptr() if N == 100 else None)
        j.wb, j.ldd, j.wt, j.lddT = wb.data_ptr(), K + 8, (wt.data_ptr() if wt is not None else None), N + 8
        keep.append((w, wb, wt))
    hip.check(hip.lib().vt_pack_weights_grouped(jobs, len(shapes), hip.stream()), "vt_pack_weights_grouped")
    for i, (_, wb, wt) in enumerate(keep):
        show(f"pack_weights_grouped ragged={int(ragged)} job {i} {shapes[i]}", wb=wb, wt=wt)


def main():
    print("# library:", os.path.basename(hip.LIB_PATH), file=sys.stderr)
    for dim in DIMS:
        for rows in (508, 509):
            layernorm(dim, rows, None)
            layernorm(dim, rows, (100, 130, 20))
    layernorm(768, 3000, (1000, 1024, 24))       # past the backward's 512 workgroups: the grid-stride loop
    rows_cases()
    for N, K in ((2304, 768), (768, 3072), (64, 64), (100, 72), (33, 50), (7, 129), (1, 1)):
        pack_single(N, K)
    pack_single(128, 256, pad=0)
    pack_single(100, 72, perm=True)
    pack_single(100, 71, perm=True)
    for N, K in ((768, 768), (33, 50)):
        pack_single(N, K, want_t=False)
        pack_single(N, K, want_b=False)
    pack_grouped(False)
    pack_grouped(True)


if __name__ == "__main__":
    main()
