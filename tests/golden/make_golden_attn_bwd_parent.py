"""Record the attention backward of the commit BEFORE the one-launch backward as tests/golden/attn_bwd_parent_<case>_<i>.npz.

Run once, on a GPU, under the parent commit's library (it was run with the one-launch change still uncommitted, HEAD = the parent):
    bash tools/ab_build.sh                                   (builds git HEAD's library into video-tokenizer_amd/_ab/libvt_base.so)
    VT_HIP_LIB=$PWD/video-tokenizer_amd/_ab/libvt_base.so python tests/golden/make_golden_attn_bwd_parent.py [out_dir]
Cases, inputs and the file layout: tests/attn_bwd_parent_cases.py.  Each case runs twice and must repeat its bits before it is written.
With out_dir the files are also copied there."""
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import attn_bwd_parent_cases as P  # noqa: E402


def main():
    import video_tokenizer_amd.hip as hip
    assert os.environ.get("VT_HIP_LIB"), "select the parent commit's library with VT_HIP_LIB"
    print("library:", hip.LIB_PATH)
    for name in P.CASES:
        a, b = P.run(hip, name), P.run(hip, name)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k)
        n = P.save(name, a)
        back = P.load(name)
        assert all(np.array_equal(a[k].view(np.uint8), back[k].view(np.uint8)) for k in a) and set(a) == set(back)
        for f in P.files_of(name):
            print(f"{name:6s} {os.path.basename(f)} {os.path.getsize(f)} bytes")
            if len(sys.argv) > 1:
                os.makedirs(sys.argv[1], exist_ok=True)
                shutil.copy(f, sys.argv[1])
        print(f"{name:6s} {n} file(s): " + ", ".join(f"{k}{a[k].shape}" for k in a))


if __name__ == "__main__":
    main()
