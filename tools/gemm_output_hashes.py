"""SHA-256 of every output of a fixed list of vt_gemm_nt / vt_gemm_tn_grouped launches, for the library named by VT_HIP_LIB (default: the
tree's build).  The check of a refactor that must not change a bit: run it once per library, each in its own process, and diff the two outputs.
usage: VT_HIP_LIB=video-tokenizer_amd/_ab/libvt_base.so python tools/gemm_output_hashes.py > parent.txt; python tools/gemm_output_hashes.py > tree.txt
The cases are the smallest that reach each path of the NT kernels: all six epilogues (column sums with DGELU and MULAUX) on tiles 0, 1, 16, 2, 6
and 7 where valid and split K on tile 1; full tiles with the 16-byte read-back (384 x 384), ragged M with the 8-byte read-back (200 x 196),
N % 4 != 0 (200 x 198: nt_epilogue and its scalar tail), skinny (40 x 196), a persistent walk that takes a second tile (3264 x 3072 on tile 2:
272 tiles on 256 CUs), and the fp32 epilogue with every option under a row map of groups >= 192 rows (batched loop) and < 192 (rolled loop)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import video_tokenizer_amd.hip as hip  # noqa: E402

EPIS = {hip.EPI_BF16: "bf16", hip.EPI_BF16_GELU: "gelu", hip.EPI_F32: "f32", hip.EPI_BF16_DGELU: "dgelu", hip.EPI_BF16_GELU_GRAD: "gelu_grad",
        hip.EPI_BF16_MULAUX: "mulaux"}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def rand(shape, seed, std=1.0, dtype=torch.bfloat16):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).to(dtype).cuda()


def rows(M, N, dtype):
    """zeroed [M, N] with a row stride that is a multiple of 4 elements (the hash covers the padding too)"""
    return torch.zeros(M, (N + 3) // 4 * 4, dtype=dtype, device="cuda")


def nt_case(M, N, K, epi, tile, splitk=1, colsum=False):
    A, B, bias = rand((M, K), 1, 0.5), rand((N, K), 2, 0.5), rand((N,), 3, 1.0, torch.float32)
    f32 = epi == hip.EPI_F32
    out = rows(M, N, torch.float32 if f32 else torch.bfloat16)
    kw = dict(bias=bias, out=out[:, :N], tile=tile, splitk=splitk)
    outs = {"out": out}
    if epi in (hip.EPI_BF16_GELU, hip.EPI_BF16_GELU_GRAD):
        outs["out2"] = rows(M, N, torch.bfloat16)
        kw["out2"] = outs["out2"][:, :N]
    if epi in (hip.EPI_BF16_DGELU, hip.EPI_BF16_MULAUX):
        aux = rows(M, N, torch.bfloat16)
        aux[:, :N] = rand((M, N), 4)
        kw["aux"] = aux[:, :N]
        if colsum:
            outs["colsum"] = torch.zeros((M + 191) // 192, N, device="cuda")
            kw["colsum_partial"] = outs["colsum"]
    if f32:
        res = rows(M, N, torch.float32)
        res[:, :N] = rand((M, N), 5, 1.0, torch.float32)
        kw["residual"] = res[:, :N]
    hip.gemm_nt(A, B, epi, **kw)
    torch.cuda.synchronize()
    name = f"nt {EPIS[epi]:9s} tile={tile:<2d} splitk={splitk} colsum={int(colsum)} {M}x{N}x{K}"
    print(name, " ".join(f"{k}={sha(v)}" for k, v in outs.items()), flush=True)


def f32_full_case(tile, grp, stride, off):
    """every option of the fp32 epilogue at once, M = 400 rows scattered by the row map"""
    M, N, K, period = 400, 384, 128, 50
    out_rows = (M + grp - 1) // grp * stride
    A, B, bias = rand((M, K), 11, 0.5), rand((N, K), 12, 0.5), rand((N,), 13, 1.0, torch.float32)
    out, out2 = torch.zeros(out_rows, N, device="cuda"), torch.zeros(out_rows, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm_nt(A, B, hip.EPI_F32, bias=bias, out=out, out2=out2, residual=rand((out_rows, N), 14, 1.0, torch.float32),
                rowmod=rand((period, N), 15, 1.0, torch.float32), rowmod_period=period, omap=hip.RowMap(grp, stride, off), round_bf16=True,
                out_scale=0.5, tile=tile, splitk=1)
    torch.cuda.synchronize()
    print(f"nt f32 every option tile={tile:<2d} row map grp={grp} stride={stride} off={off}  out={sha(out)} out2={sha(out2)}", flush=True)


def tn_case(tile):
    M, P, Q = 256, 392, 200
    dY, X = rand((M, P), 21), rand((M, Q), 22)
    perm = torch.randperm(P - 8, generator=torch.Generator().manual_seed(23)).to(torch.int32).cuda()
    o1, o2 = torch.zeros(P, Q, device="cuda"), torch.zeros(P, Q, device="cuda")
    hip.gemm_tn_grouped([dict(A=dY, B=X, out=o1, tile=tile), dict(A=dY, B=X, out=o2, p_lim=P - 8, q_lim=Q - 8, row_perm=perm, tile=tile)])
    torch.cuda.synchronize()
    print(f"tn grouped tile={tile} {M}x{P}x{Q}  out={sha(o1)} limits+perm={sha(o2)}", flush=True)


def main():
    print("# library:", os.path.basename(hip.LIB_PATH), file=sys.stderr)
    for M, N, K in [(384, 384, 128), (200, 196, 128), (200, 198, 128), (40, 196, 128)]:
        for epi in EPIS:
            for tile in (0, 1, 16, 2, 6) + ((7,) if M <= 64 else ()):
                nt_case(M, N, K, epi, tile)
            nt_case(M, N, K, epi, 1, splitk=2)
            if epi in (hip.EPI_BF16_DGELU, hip.EPI_BF16_MULAUX) and N % 4 == 0:
                for tile in (0, 2, 6):
                    nt_case(M, N, K, epi, tile, colsum=True)
    for epi in EPIS:
        nt_case(3264, 3072, 64, epi, 2, colsum=epi in (hip.EPI_BF16_DGELU, hip.EPI_BF16_MULAUX))
    for tile in (1, 2, 6):
        f32_full_case(tile, 200, 260, 30)     # groups >= 192 rows: the 192-row kernel's batched loop
        f32_full_case(tile, 50, 80, 20)       # shorter groups: its rolled loop
    for tile in (1, 2, 7):
        tn_case(tile)


if __name__ == "__main__":
    main()
