"""Host-side surface of the packed variable-length attention (no GPU): the refusals of vt_attention_varlen_* and vt_qknorm_rope_gqa_*,
which validate every argument before any launch; the fp32 restatement of tests/varlen_reference.py against the fixture the reference's own
code wrote (tests/golden/make_golden_varlen.py); varlen.rope_freqs against the reference's tables; get_model_dims.

Every call below is INVALID in exactly one way and must come back with VT_ERR_INVALID and a message that names the entry point: the
pointers are made-up addresses, so a call that got past the validation would launch on them."""
import ctypes

import pytest
import torch

import video_tokenizer_amd as vt
from tests import varlen_reference as R

VT_ERR_INVALID = -1
P = 0x7F0000001000            # a 16-byte aligned made-up address; never dereferenced
c_i32 = ctypes.c_int32


def last_error():
    buf = ctypes.create_string_buffer(512)
    vt.hip.lib().vt_last_error(buf, 512)
    return buf.value.decode()


def fwd(cu, M=8, Hq=4, Hkv=2, hd=64, q=P, q_rs=None, k_rs=None, v_rs=None, n=None):
    W = 64 * (Hq + 2 * Hkv)
    arr = (c_i32 * len(cu))(*cu) if cu is not None else None
    n = len(cu) - 1 if n is None else n
    return vt.hip.lib().vt_attention_varlen_fwd(q, W if q_rs is None else q_rs, P + 128 * Hq, W if k_rs is None else k_rs, P + 128 * (Hq + Hkv),
                                                W if v_rs is None else v_rs, arr, n, M, Hq, Hkv, hd, P + (1 << 20), P + (2 << 20), None)


def bwd(cu, M=8, Hq=4, Hkv=2, dk_rs=None, dv=P + (5 << 20)):
    W = 64 * (Hq + 2 * Hkv)
    arr = (c_i32 * len(cu))(*cu)
    return vt.hip.lib().vt_attention_varlen_bwd(P, W, P + 128 * Hq, W, P + 128 * (Hq + Hkv), W, P + (1 << 20), P + (2 << 20), P + (3 << 20), arr,
                                                len(cu) - 1, M, Hq, Hkv, 64, P + (4 << 20), W, P + (4 << 20) + 128 * Hq, W if dk_rs is None else dk_rs,
                                                dv, W, P + (6 << 20), None)


REFUSED_FWD = {
    "non-monotone cu": dict(cu=[0, 5, 3, 8]),
    "an empty sequence": dict(cu=[0, 5, 5, 8]),
    "cu[0] != 0": dict(cu=[1, 5, 8]),
    "cu[n] != M": dict(cu=[0, 5, 9]),
    "more than 64 sequences": dict(cu=list(range(66)), M=65),
    "no sequence": dict(cu=[0], M=8, n=0),
    "null cu": dict(cu=None, n=1),
    "Hq % Hkv != 0": dict(cu=[0, 8], Hq=3, Hkv=2),
    "head_dim 32": dict(cu=[0, 8], hd=32),
    "a q stride below 64 Hq": dict(cu=[0, 8], q_rs=64 * 4 - 8),
    "a k stride that is no multiple of 8": dict(cu=[0, 8], k_rs=64 * 8 + 4),
    "a v stride of 2^24": dict(cu=[0, 8], v_rs=1 << 24),
    "a misaligned q": dict(cu=[0, 8], q=P + 8),
}


@pytest.mark.parametrize("what", sorted(REFUSED_FWD))
def test_varlen_forward_refuses(what):
    assert fwd(**REFUSED_FWD[what]) == VT_ERR_INVALID, what
    assert "vt_attention_varlen_fwd" in last_error()


def test_varlen_backward_refuses():
    for kw in (dict(cu=[0, 5, 3, 8]), dict(cu=[2, 8]), dict(cu=[0, 7]), dict(cu=list(range(66)), M=65), dict(cu=[0, 8], Hq=4, Hkv=3),
               dict(cu=[0, 8], dk_rs=64), dict(cu=[0, 8], dv=P + (5 << 20) + 2)):
        assert bwd(**kw) == VT_ERR_INVALID, kw
        assert "vt_attention_varlen_bwd" in last_error()


def test_row_pass_refuses():
    lib = vt.hip.lib()

    def f(M=8, Hq=4, Hkv=2, in_rs=512, out_rs=512, src=P):
        return lib.vt_qknorm_rope_gqa_fwd(src, in_rs, M, Hq, Hkv, P, P, P, P, 1e-5, P, P, P + (1 << 20), out_rs, None)

    for kw in (dict(Hq=3), dict(in_rs=504), dict(out_rs=516), dict(src=P + 4), dict(M=0)):
        assert f(**kw) == VT_ERR_INVALID, kw
        assert "vt_qknorm_rope_gqa_fwd" in last_error()
    assert lib.vt_qknorm_rope_gqa_bwd(P, 512, P, 512, 8, 4, 3, P, P, 1e-5, P, P, P, 512, None, None, None, None, P, None) == VT_ERR_INVALID
    assert "vt_qknorm_rope_gqa_bwd" in last_error()
    assert lib.vt_qknorm_rope_gqa_bwd_workspace_bytes() == lib.vt_qknorm_rope_bwd_workspace_bytes() > 0


def test_wrappers_refuse_cpu_tensors_and_bad_boundaries():
    q = torch.zeros(8, 256, dtype=torch.bfloat16)
    kv = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(vt.hip.HipError):
        vt.hip.attention_varlen_fwd(q, kv, kv, [0, 8], 4, 2)
    with pytest.raises(vt.hip.HipError):
        vt.hip.cu_seqlens_host([0])
    with pytest.raises(vt.hip.HipError):
        vt.hip.cu_seqlens_host(torch.zeros(3))                       # a float tensor
    with pytest.raises(vt.hip.HipError):
        vt.hip.cu_seqlens_list([0, 3.5, 8])                          # a float in a list is not truncated
    with pytest.raises(vt.hip.HipError, match="cu_seqlens"):         # nor a float tensor handed to the layer or the Function
        vt.varlen.Attn(128, [2, 2])(torch.zeros(8, 128), (torch.zeros(8, 32), torch.zeros(8, 32)), torch.tensor([0.0, 8.0]), 8)
    with pytest.raises(vt.hip.HipError, match="cu_seqlens"):
        vt.functional.VarlenAttend.apply(q, kv, kv, torch.tensor([0.0, 8.0]), 4, 2)
    assert vt.hip.cu_seqlens_list((0, 3, 8)) == [0, 3, 8] == vt.hip.cu_seqlens_list(torch.tensor([0, 3, 8], dtype=torch.int32))
    arr, n, M = vt.hip.cu_seqlens_host(torch.tensor([0, 3, 8]))
    assert (list(arr), n, M) == ([0, 3, 8], 2, 8)
    assert vt.hip.VARLEN_MAX_SEQ == 64


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_reference_fixture(golden, case):
    freqs = torch.complex(torch.from_numpy(golden[f"{case}/freqs_re"]), torch.from_numpy(golden[f"{case}/freqs_im"]))
    out = R.run_case(case, freqs)
    for t in R.TENSORS:
        want = torch.from_numpy(golden[f"{case}/{t}"])
        assert out[t].shape == want.shape
        assert R.rel_l2(out[t], want) <= 1e-5, t


@pytest.mark.parametrize("case", list(R.CASES))
def test_rope_freqs_equal_the_reference_tables(golden, case):
    c = R.CASES[case]
    freqs, cos, sin = vt.varlen.rope_freqs(c["grids"], c["tokens"])
    want = torch.complex(torch.from_numpy(golden[f"{case}/freqs_re"]), torch.from_numpy(golden[f"{case}/freqs_im"]))
    assert freqs.dtype == torch.complex128 and tuple(freqs.shape) == (sum(R.lengths(case)), 32)
    assert float((freqs - want).abs().max()) <= 1e-12                # float64 on both sides; the angles reach a few thousand radians
    assert cos.dtype == torch.float32 == sin.dtype and float((cos - want.real.float()).abs().max()) <= 2.0 ** -23
    assert float((sin - want.imag.float()).abs().max()) <= 2.0 ** -23
    ids = vt.varlen.position_ids((2, 4, 4), 65)
    assert ids[:65].tolist() == [[t, t, t] for t in range(65)] and ids[65].tolist() == [65, 65, 65] and ids[-1].tolist() == [66, 68, 68]


def test_module_surface(golden):
    assert vt.varlen.get_model_dims("base") == (768, 12, [12, 4], 4.0) and vt.varlen.get_model_dims("large") == (1024, 24, [16, 4], 4.0)
    assert vt.varlen.get_model_dims("small_thin") == (768, 5, [12, 4], 2.0)
    m = vt.varlen.Attn(384, [6, 2])
    assert tuple(m.state_dict()) == tuple(str(golden["state_dict_keys"]).split("\n")) == R.PARAM_NAMES
    assert [",".join(str(d) for d in v.shape) for v in m.state_dict().values()] == str(golden["h6_2/state_dict_shapes"]).split("\n")
    with pytest.raises(ValueError):
        vt.varlen.Attn(384, [6, 4])
    with pytest.raises(vt.hip.HipError):
        m(torch.zeros(8, 384), (torch.zeros(8, 32), torch.zeros(8, 32)), [0, 8], 8)
