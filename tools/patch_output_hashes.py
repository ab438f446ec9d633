"""SHA-256 of every output of a fixed list of calls into the six patch-end entry points (csrc/vt_patch.hip: vt_patchify, vt_unpatchify,
vt_patchify_dual, vt_unpatchify_dual; csrc/vt_packed.hip: vt_patchify_clips, vt_unpatchify_clips), for the library named by VT_HIP_LIB
(default: the tree's build).  The check of a refactor that must not change a bit: run it once per library, each in its own process, and
diff the two outputs.
usage: VT_HIP_LIB=video-tokenizer_amd/_ab/libvt_base.so python tools/patch_output_hashes.py > parent.txt; python tools/patch_output_hashes.py > tree.txt
The cases: the edge shapes of tests/test_patch_rows_gpu.py, tests/test_dualpatch_rows_gpu.py and tests/test_packed_rows_gpu.py, and the
benchmark's geometry (8 clips of 3 x 16 x 128 x 128, (4, 8, 8) patches; (1, 8, 8) + (3, 8, 8) for the two-segment pair).  Every destination is
zeroed first, so a hash would show an element left unwritten."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import video_tokenizer_amd.hip as hip  # noqa: E402

PLAIN = [(1, 3, 2, 8, 2, 8), (2, 3, 4, 24, 2, 8), (2, 2, 3, 32, 1, 16), (3, 1, 4, 16, 4, 8), (8, 3, 16, 128, 4, 8)]     # (B, C, T, S, pt, p)
DUAL = [(2, 3, 7, 16, 24, 1, 1, 3, 8, 8), (1, 1, 2, 8, 8, 1, 1, 1, 8, 8), (2, 3, 6, 32, 16, 2, 2, 2, 16, 8), (3, 2, 8, 16, 16, 4, 2, 4, 8, 16),
        (2, 3, 7, 16, 16, 1, 1, 3, 8, 8), (3, 2, 8, 16, 16, 4, 2, 4, 8, 8), (8, 3, 16, 128, 128, 1, 1, 3, 8, 8)]            # (B, C, T, H, W, T0, pt0, pt1, ph, pw)
CLIPS = [[(8, 16, 24)], [(4, 8, 8)] * 64, [(4, 8, 8), (8, 32, 40)], [(4, 8, 8), (8, 16, 16), (4, 32, 32)], [(16, 128, 128)] * 8]  # (T, H, W); C = 3, (4, 8)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def zeros(shape, dtype):
    return torch.zeros(shape, device="cuda", dtype=dtype)


def show(name, *outs):
    torch.cuda.synchronize()
    print(name, " ".join(sha(o) for o in outs), flush=True)


def main():
    print("# library:", os.path.basename(hip.LIB_PATH), file=sys.stderr)
    for s in PLAIN:
        B, C, T, S, pt, p = s
        n, kp = B * (T // pt) * (S // p) ** 2, C * pt * p * p
        show(f"patchify {s}", hip.patchify(rand((B, C, T, S, S), 1), pt, p, rows=zeros((n, kp), torch.bfloat16)))
        show(f"unpatchify {s}", hip.unpatchify(rand((n, kp), 2), B, C, T, S, pt, p, video=zeros((B, C, T, S, S), torch.float32)))
    for s in DUAL:
        B, C, T, H, W, T0, pt0, pt1, ph, pw = s
        n0, n1 = hip.dual_grids(T, H, W, T0, pt0, pt1, ph, pw)
        sh0, sh1 = (B * n0, C * pt0 * ph * pw), (B * n1, C * pt1 * ph * pw)
        show(f"patchify_dual {s}", *hip.patchify_dual(rand((B, C, T, H, W), 3), T0, pt0, pt1, ph, pw, rows0=zeros(sh0, torch.bfloat16),
                                                      rows1=zeros(sh1, torch.bfloat16)))
        show(f"unpatchify_dual {s}", hip.unpatchify_dual(rand(sh0, 4), rand(sh1, 5), *s, video=zeros((B, C, T, H, W), torch.float32)))
    for sizes in CLIPS:
        G = sum(t * h * w for t, h, w in hip.clip_grids(sizes, 4, 8))
        name = f"{len(sizes)} x {sizes[0]}" if len(set(sizes)) == 1 else str(sizes)
        show(f"patchify_clips {name}", hip.patchify_clips([rand((3, *size), 6 + i) for i, size in enumerate(sizes)], 4, 8, out=zeros((G, 768), torch.bfloat16)))
        show(f"unpatchify_clips {name}", *hip.unpatchify_clips(rand((G, 768), 7), sizes, 3, 4, 8, out=[zeros((3, *size), torch.float32) for size in sizes]))


if __name__ == "__main__":
    main()
