"""Host-side surface of the packed `titok` model (no GPU): the registry entry and the reference's state-dict keys and shapes; the fp32
restatement of tests/titok_reference.py against the fixture the reference's own code wrote (tests/golden/make_golden_titok.py); the refusals
of the five vt_packed.hip entry points, which validate every argument and every table on the host before any launch; the refusal of
unequal clips by TiTok.forward; the rotary-table cache.

Every library call below is INVALID in exactly one way and must come back with VT_ERR_INVALID and a message that names the entry point:
the pointers are made-up addresses, so a call that got past the validation would launch on them."""
import ctypes

import pytest
import torch

import video_tokenizer_amd as vt
from tests import titok_reference as R

VT_ERR_INVALID = -1
P = 0x7F0000001000            # a 16-byte aligned made-up address; never dereferenced
c_i32 = ctypes.c_int32
DIMS_A = R.CASES["A"]["dims"]


def last_error():
    buf = ctypes.create_string_buffer(512)
    vt.hip.lib().vt_last_error(buf, 512)
    return buf.value.decode()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _keys_and_shapes(sd):
    return list(sd), [",".join(str(d) for d in v.shape) for v in sd.values()]


def test_titok_is_registered_with_the_reference_state_dict(golden):
    assert vt.models["titok"] is vt.TiTok is vt.titok_model.TiTok
    with torch.device("meta"):
        m = vt.make({"name": "titok", "args": dict(bottleneck=None, prior_model=None, encoder_hidden_size=3, num_latent_tokens=7, junk="x")})
    keys, shapes = _keys_and_shapes(m.state_dict())
    assert keys == str(golden["titok/state_dict_keys"]).split("\n") and shapes == str(golden["titok/state_dict_shapes"]).split("\n")
    assert (m.encoder.width, m.encoder.num_layers, m.encoder.heads, m.decoder.num_layers) == (768, 12, [12, 4], 12)
    assert m.prior_model is None and m.quantize.levels == (8, 8, 8, 5, 5, 5) and m.encoder.patch_size == (4, 8, 8)


@pytest.mark.parametrize("case", list(R.CASES))
def test_encoder_and_decoder_have_the_reference_state_dict(golden, case):
    dims = R.CASES[case]["dims"]
    for stage, m in (("enc", vt.varlen.TiTokEncoder(out_channels=6, _dims=dims)), ("dec", vt.varlen.TiTokDecoder(in_channels=6, _dims=dims))):
        keys, shapes = _keys_and_shapes(m.state_dict())
        assert keys == str(golden[f"{case}/{stage}/state_dict_keys"]).split("\n") == list(R.param_shapes(case, stage)), stage
        assert shapes == str(golden[f"{case}/{stage}/state_dict_shapes"]).split("\n"), stage
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.params(case, stage).items()}, strict=True)
    f = vt.varlen.ffd(128, 4.0)
    assert [type(l).__name__ for l in f] == ["LayerNorm", "Linear", "GEGLU", "Dropout", "Linear"] and f[4].in_features == 352
    assert vt.varlen.ffd(512, 4.0)[4].in_features == 1376 == vt.varlen.ffd(1024, 2.0)[4].in_features
    with pytest.raises(ValueError):
        vt.varlen.TiTokEncoder(_dims=(96, 1, [3, 1], 4.0))              # head dimension 32
    with pytest.raises(ValueError):
        vt.varlen.TiTokEncoder(_dims=(192, 1, [3, 1], 4.0))             # no LayerNorm width


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_reference_fixture(golden, case):
    """the bar of tests/test_varlen_cpu.py for the layer's restatement: 1e-5 relative L2, fp32 against fp32"""
    for stage in R.STAGES:
        out = R.run_stage(case, stage, codes=golden[f"{case}/codes"])
        for t in R.tensors(case, stage):
            want = torch.from_numpy(golden[f"{case}/{stage}/{t}"])
            assert out[t].shape == want.shape, (stage, t)
            assert R.rel_l2(out[t], want) <= 1e-5, (stage, t, R.rel_l2(out[t], want))


def test_case_geometry():
    assert R.grid_sizes() == [1, 12, 8, 20] and R.lengths() == [2, 77, 15, 148] and R.cu_seqlens()[-1] == 242
    assert sum(R.TOKENS) == 201 and sum(R.grid_sizes()) == 41
    enc = vt.varlen.TiTokEncoder(out_channels=6, _dims=DIMS_A)
    grids, gs, lens, cu = enc.geometry(R.CLIP_SIZES, R.TOKENS)
    assert (grids, gs, lens, cu) == (R.grids(), R.grid_sizes(), R.lengths(), R.cu_seqlens())
    for sizes, counts in (([(4, 8, 8)] * 65, [1] * 65), ([(4, 8, 12)], [1]), ([(6, 8, 8)], [1]), ([(4, 8, 8)], [0]), ([(4, 8, 8)], [1, 2]), ([], [])):
        with pytest.raises(ValueError):
            enc.geometry(sizes, counts)


# ---- the five entry points refuse, on the host -----------------------------------------------------------------------------------------
def _clips(sizes, data=None):
    arr = (vt.hip.Clip * max(len(sizes), 1))()
    for i, (a, s) in enumerate(zip(arr, sizes)):
        a.data, a.T, a.H, a.W = (P + (i << 24)) if data is None else data[i], *s
    return arr


def patchify(sizes, n=None, C=3, pt=4, p=8, rows=None, out=P + (1 << 40), data=None, unpatchify=False, null_table=False):
    G = sum((T // pt) * (H // p) * (W // p) for T, H, W in sizes) if pt > 0 and p > 0 else 0
    rows = G if rows is None else rows
    n = len(sizes) if n is None else n
    tab = None if null_table else _clips(sizes, data)
    lib = vt.hip.lib()
    return lib.vt_unpatchify_clips(out, rows, tab, n, C, pt, p, None) if unpatchify else lib.vt_patchify_clips(tab, n, C, pt, p, out, rows, None)


REFUSED_CLIPS = {
    "65 clips": dict(sizes=[(4, 8, 8)] * 65),
    "no clip": dict(sizes=[], n=0),
    "W % p != 0": dict(sizes=[(4, 8, 8), (4, 8, 12)]),
    "H % p != 0": dict(sizes=[(4, 12, 8)]),
    "T % pt != 0": dict(sizes=[(6, 8, 8)]),
    "p % 8 != 0": dict(sizes=[(4, 8, 8)], p=4),
    "a misaligned clip": dict(sizes=[(4, 8, 8), (4, 8, 8)], data=[P, P + (1 << 24) + 4]),
    "a null clip": dict(sizes=[(4, 8, 8)], data=[None]),
    "a null table": dict(sizes=[(4, 8, 8)], null_table=True),
    "null rows": dict(sizes=[(4, 8, 8)], out=None),
    "a row count that is not the clips'": dict(sizes=[(4, 8, 8), (8, 16, 24)], rows=12),
    "an empty clip": dict(sizes=[(4, 0, 8)]),
}


@pytest.mark.parametrize("what", sorted(REFUSED_CLIPS))
def test_patchify_clips_refuses(what):
    assert patchify(**REFUSED_CLIPS[what]) == VT_ERR_INVALID, what
    assert "vt_patchify_clips" in last_error()
    assert patchify(unpatchify=True, **REFUSED_CLIPS[what]) == VT_ERR_INVALID, what
    assert "vt_unpatchify_clips" in last_error()


def test_refusals_name_the_offending_value():
    assert patchify(sizes=[(4, 8, 8), (4, 8, 12)]) == VT_ERR_INVALID and "clip 1" in last_error() and "W=12" in last_error()
    assert patchify(sizes=[(4, 8, 8)], p=4) == VT_ERR_INVALID and "p=4" in last_error()
    assert patchify(sizes=[(4, 8, 8)] * 65) == VT_ERR_INVALID and "n=65" in last_error()
    assert packed("scatter", cu=[0, 2, 10], lead=[2, 3]) == VT_ERR_INVALID and "lead[0]=2" in last_error()
    assert packed("gather", cu=[0, 2, 10], lead=[0, 3]) == VT_ERR_INVALID and "lead[0]=0" in last_error()
    assert packed("colsum", cu=[0, 5, 9], lead=[1, 1], M=10) == VT_ERR_INVALID and "cu_seqlens[2]=9" in last_error() and "M=10" in last_error()


def packed(op, cu, lead, M=None, D=128, which=0, n=None, src=P, dst=P + (1 << 30), vec=P + (1 << 29), ws=P + (1 << 31)):
    M = (cu[-1] if cu else 0) if M is None else M
    n = len(cu) - 1 if n is None else n
    cu_a = (c_i32 * len(cu))(*cu) if cu is not None else None
    lead_a = (c_i32 * max(len(lead), 1))(*lead) if lead is not None else None
    lib = vt.hip.lib()
    if op == "scatter":
        return lib.vt_packed_scatter(src, vec, cu_a, lead_a, n, M, D, which, dst, None)
    if op == "gather":
        return lib.vt_packed_gather(src, cu_a, lead_a, n, M, D, which, dst, None)
    return lib.vt_packed_segment_colsum(src, cu_a, lead_a, n, M, D, which, dst, ws, None)


REFUSED_PACKED = {
    "lead[b] == L_b": dict(cu=[0, 2, 10], lead=[2, 3]),
    "lead[b] == 0": dict(cu=[0, 2, 10], lead=[1, 0]),
    "a lead count past its sequence": dict(cu=[0, 2, 10], lead=[1, 9]),
    "non-increasing cu": dict(cu=[0, 5, 5, 8], lead=[1, 1, 1]),
    "decreasing cu": dict(cu=[0, 5, 3, 8], lead=[1, 1, 1]),
    "cu[0] != 0": dict(cu=[1, 5, 8], lead=[1, 1]),
    "cu[n] != M": dict(cu=[0, 5, 9], lead=[1, 1], M=10),
    "65 sequences": dict(cu=list(range(0, 132, 2)), lead=[1] * 65),
    "no sequence": dict(cu=[0], lead=[], n=0, M=8),
    "D % 4 != 0": dict(cu=[0, 8], lead=[3], D=126),
    "a null source": dict(cu=[0, 8], lead=[3], src=None),
    "a null destination": dict(cu=[0, 8], lead=[3], dst=None),
    "a misaligned source": dict(cu=[0, 8], lead=[3], src=P + 4),
    "null cu": dict(cu=None, lead=[3], n=1, M=8),
    "null lead": dict(cu=[0, 8], lead=None),
    "a segment that is neither": dict(cu=[0, 8], lead=[3], which=2),
}


@pytest.mark.parametrize("op", ["scatter", "gather", "colsum"])
@pytest.mark.parametrize("what", sorted(REFUSED_PACKED))
def test_packed_rows_refuse(op, what):
    assert packed(op, **REFUSED_PACKED[what]) == VT_ERR_INVALID, what
    assert {"scatter": "vt_packed_scatter", "gather": "vt_packed_gather", "colsum": "vt_packed_segment_colsum"}[op] in last_error()


def test_scatter_takes_a_null_vec_and_colsum_needs_its_workspace():
    assert packed("colsum", cu=[0, 8], lead=[3], ws=None) == VT_ERR_INVALID and "vt_packed_segment_colsum" in last_error()
    assert packed("scatter", cu=[0, 8], lead=[3], vec=P + 8) == VT_ERR_INVALID and "vt_packed_scatter" in last_error()
    assert vt.hip.lib().vt_packed_segment_colsum_workspace_bytes(768) >= 768 * 4


def test_wrappers_refuse_cpu_tensors_and_float_counts():
    x = torch.zeros(8, 128)
    with pytest.raises(vt.hip.HipError):
        vt.hip.packed_gather(x, [0, 8], [3], vt.hip.PACKED_LEAD)
    with pytest.raises(vt.hip.HipError):
        vt.hip.patchify_clips([torch.zeros(3, 4, 8, 8)], 4, 8)
    with pytest.raises(vt.hip.HipError, match="integers"):
        vt.hip._packed_tables([0, 8], [2.5])
    with pytest.raises(vt.hip.HipError, match="lead counts"):
        vt.hip._packed_tables([0, 8], [2, 3])
    assert vt.hip.clip_grids(R.CLIP_SIZES, 4, 8) == R.grids()


# ---- the model's host side --------------------------------------------------------------------------------------------------------------
def test_forward_refuses_clips_of_unequal_size():
    m = vt.TiTok(_geometry=dict(dims=DIMS_A))
    with pytest.raises(ValueError, match="encode"):
        m([torch.zeros(3, 4, 8, 8), torch.zeros(3, 4, 8, 16)])
    with pytest.raises(vt.hip.HipError):
        m([torch.zeros(3, 4, 8, 8), torch.zeros(3, 4, 8, 8)])              # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        vt.varlen.TiTokDecoder(in_channels=6, _dims=DIMS_A).geometry([(4, 8, 8)] * 65, [1] * 65)


def test_rotary_tables_are_cached_by_grids_and_token_counts():
    enc = vt.varlen.TiTokEncoder(out_channels=6, _dims=DIMS_A)
    a = enc.rope_tables(R.grids(), R.TOKENS, "cpu")
    b = enc.rope_tables([list(g) for g in R.grids()], list(R.TOKENS), "cpu")
    assert a[0] is b[0] and a[1] is b[1]                                    # the same tensors for the same key
    c = enc.rope_tables(R.grids(), (1, 65, 7, 127), "cpu")
    assert c[0] is not a[0] and c[0].shape == (241, 32) and a[0].shape == (242, 32)
    want = vt.varlen.rope_freqs(R.grids(), R.TOKENS)
    assert torch.equal(a[0], want[1]) and torch.equal(a[1], want[2])
    for n in range(2, 2 + 2 * vt.varlen._TABLE_CACHE_ENTRIES):             # the cache is small and bounded
        enc.rope_tables([(1, 1, 1)], [n], "cpu")
    assert len(enc._tables) <= vt.varlen._TABLE_CACHE_ENTRIES
    assert enc.rope_tables(R.grids(), R.TOKENS, "cpu")[0] is not a[0]       # evicted and rebuilt
