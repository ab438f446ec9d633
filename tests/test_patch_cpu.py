"""The refusals of vt_patchify / vt_unpatchify (csrc/vt_patch.hip, no GPU): the one-segment entry points validate every argument on the host
before any launch, through the same make_geom as vt_patchify_dual / vt_unpatchify_dual (tests/test_dualpatch_cpu.py).

Every library call below is INVALID in exactly one way and must come back with VT_ERR_INVALID and a message that names the entry point:
the pointers are made-up addresses, so a call that got past the validation would launch on them."""
import ctypes

import pytest
import torch

import video_tokenizer_amd as vt

VT_ERR_INVALID = -1
P = 0x7F0000001000            # a 16-byte aligned made-up address; never dereferenced
GOOD = dict(B=2, C=3, T=4, S=24, pt=2, p=8)


def last_error():
    buf = ctypes.create_string_buffer(512)
    vt.hip.lib().vt_last_error(buf, 512)
    return buf.value.decode()


def call(unpatchify=False, video=P, rows=P + (1 << 40), **change):
    g = dict(GOOD, **change)
    sizes = [g[k] for k in ("B", "C", "T", "S", "pt", "p")]
    lib = vt.hip.lib()
    return lib.vt_unpatchify(rows, *sizes, video, None) if unpatchify else lib.vt_patchify(video, *sizes, rows, None)


REFUSED = {
    "a null video": (dict(video=None), "null"),
    "null rows": (dict(rows=None), "null"),
    "a misaligned video": (dict(video=P + 4), "video"),
    "misaligned rows": (dict(rows=P + 8), "rows"),
    "T % pt != 0": (dict(T=5), "T=5"),
    "S % p != 0": (dict(S=28), "=28"),
    "p % 8 != 0": (dict(S=24, p=12), "=12"),
    "B = 0": (dict(B=0), "B=0"),
    "C < 0": (dict(C=-3), "C=-3"),
    "T = 0": (dict(T=0), "T=0"),
    "S = 0": (dict(S=0), "=0"),
    "pt = 0": (dict(pt=0), "=0"),
    "p = 0": (dict(p=0), "=0"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_both_entry_points_refuse_and_name_the_value(what):
    change, value = REFUSED[what]
    assert call(**change) == VT_ERR_INVALID, what
    assert last_error().startswith("vt_patchify:") and value in last_error(), last_error()
    assert call(unpatchify=True, **change) == VT_ERR_INVALID, what
    assert last_error().startswith("vt_unpatchify:") and value in last_error(), last_error()


def test_wrappers_refuse_cpu_tensors_and_wrong_buffers():
    v, rows = torch.zeros(1, 1, 2, 8, 8), torch.zeros(1, 128, dtype=torch.bfloat16)
    with pytest.raises(vt.hip.HipError):
        vt.hip.patchify(v, 2, 8, rows=rows)
    with pytest.raises(vt.hip.HipError):
        vt.hip.unpatchify(rows.float(), 1, 1, 2, 8, 2, 8, video=v)
    with pytest.raises(AssertionError):                                          # the dtype, contiguity and size assertions of the dual wrappers
        vt.hip.patchify(v.double(), 2, 8, rows=rows)
    with pytest.raises(AssertionError):
        vt.hip.patchify(v.transpose(3, 4), 2, 8, rows=rows)
    with pytest.raises(AssertionError):
        vt.hip.patchify(v, 2, 8, rows=rows[:, :64])
    with pytest.raises(AssertionError):
        vt.hip.unpatchify(rows, 1, 1, 2, 8, 2, 8, video=v)                       # bf16 rows
