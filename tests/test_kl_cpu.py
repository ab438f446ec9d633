"""The KL ('skl') bottleneck without a GPU: the CPU restatement against fixtures made by the reference's own bottleneck.py, the
module surface (state-dict layout, yaml + --opts, rejected names), host-side argument checks of the new entry points, workspace
planning, and the stream-order ledger of a KL handle's whole step (tests/c/engine_ledger_kl.hip)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import video_tokenizer_amd as vt
from oracle import larp_oracle as O
from tests import kl_reference as K
from tests import ledger as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _pieces():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "kl_pieces.npz")).items()}


def test_restatement_matches_reference_fixtures():
    P = _pieces()
    z = P["z"].clone().requires_grad_(True)
    out = K.kl_bottleneck(z, P["noise"])
    torch.testing.assert_close(out["regularized_z"], P["sample"], rtol=1e-6, atol=0)
    torch.testing.assert_close(out["mean"], P["mean"], rtol=0, atol=0)
    torch.testing.assert_close(out["kl"], P["kl"], rtol=1e-6, atol=0)
    torch.testing.assert_close(out["loss_kl"].reshape(1), P["loss_kl"], rtol=1e-6, atol=0)
    K.weighted_loss(out, P["w"]).backward()
    torch.testing.assert_close(z.grad, P["dz"], rtol=1e-6, atol=1e-6)
    # the clamp cases: outside the bounds no logvar gradient, at the bounds (inclusive) a gradient
    lv = P["z"][..., 1::2]
    dlv = P["dz"][..., 1::2]
    assert (dlv[(lv < -30) | (lv > 20)] == 0).all()
    assert (dlv[(lv == -30) | (lv == 20)] != 0).all() and ((lv == -30) | (lv == 20)).sum() == 4


def test_bottleneck_state_dict_layout_matches_reference():
    from video_tokenizer_amd.bottleneck import Bottleneck, SummedKLDivergenceRegularizer
    lay = np.load(os.path.join(GOLD, "kl_layout.npz"))
    args = json.loads(str(lay["args"]))
    b = Bottleneck(regularizer={"name": "skl", "args": {}}, norm="none", **args)
    sd = b.state_dict()
    assert list(sd) == json.loads(str(lay["names"]))
    assert [list(v.shape) for v in sd.values()] == json.loads(str(lay["shapes"]))
    assert b.project_dim == 2 * args["bottleneck_dim"] and isinstance(b.regularizer, SummedKLDivergenceRegularizer)
    assert b.regularizer.decode is not None and torch.equal(b.regularizer.decode(torch.ones(2)), torch.ones(2))


def test_distribution_glue_matches_restatement():
    from video_tokenizer_amd.bottleneck import DiagonalGaussianDistribution
    P = _pieces()
    dist = DiagonalGaussianDistribution(P["z"], deterministic=False)
    torch.testing.assert_close(dist.kl(), P["kl"], rtol=1e-6, atol=0)
    assert torch.equal(dist.mode(), P["mean"]) and torch.equal(dist.mean, P["mean"])
    assert dist.logvar.min() >= -30 and dist.logvar.max() <= 20
    torch.testing.assert_close(dist.var, torch.exp(dist.logvar))
    torch.testing.assert_close(dist.std, torch.exp(0.5 * dist.logvar))
    assert dist.nll(P["sample"], dims=[1, 2]).shape == (P["z"].shape[0],)
    assert torch.equal(DiagonalGaussianDistribution(P["z"], deterministic=True).sample(), P["mean"])


def test_yaml_opts_surface_builds_the_kl_model():
    from tests.test_host_cpu import YAML     # the shipped yaml's surface, as test_yaml_surface_vars_and_opts reads it
    from video_tokenizer_amd.config import load_cfg
    args = {"csv_file": "null128", "frame_num": 4, "input_size": 32}
    cfg = load_cfg(YAML, args, ["model.name", "larp_tokenizer", "model.args.bottleneck_type", "vq",
                                "model.args.bottleneck.args.regularizer.name", "skl", "model.args.input_size", "32",
                                "model.args.encoder_depth", "2", "model.args.decoder_depth", "2"])
    m = vt.make(cfg.model)
    d = cfg.model.args.bottleneck.args.bottleneck_dim
    assert m._kl and m._engine is not None
    assert tuple(m.bottleneck.in_linear.weight.shape) == (2 * d, m.encoder_hidden_size)
    assert tuple(m.bottleneck.out_linear.weight.shape) == (m.decoder_hidden_size, d)
    assert not any("regularizer" in k for k in m.state_dict())
    assert m.codebook_size == cfg.model.args.bottleneck.args.regularizer.args.codebook_size


@pytest.mark.parametrize("name", ["vqkl", "kl", "fsq", "none"])
def test_unsupported_regularizers_still_raise(name):
    from video_tokenizer_amd.bottleneck import Bottleneck
    with pytest.raises(NotImplementedError):
        Bottleneck(8, 64, 48, 16, regularizer={"name": name, "args": {}})


def _err():
    buf = ctypes.create_string_buffer(512)
    vt.hip.lib().vt_last_error(buf, 512)
    return buf.value.decode()


def _cfg(name="tiny", B=2):
    c = O.make_cfg(name)
    t = vt.hip.TokenizerConfig()
    t.B, t.C, t.T, t.S, t.pt, t.p = B, 3, c["frame_num"], c["input_size"], c["temporal_patch_size"], c["patch_size"]
    t.D, t.H, t.depth_enc, t.depth_dec = 768, 12, c["encoder_depth"], c["decoder_depth"]
    t.Nq, t.d, t.K = c["bottleneck_token_num"], c["bottleneck_dim"], c["codebook_size"]
    t.vq_mode, t.l2_normalized, t.inv_tau, t.beta, t.codebook_w = 0, 1, 1.0, 0.25, 1.0
    return t


def test_host_argument_errors():
    L = vt.hip.lib()
    p16 = ctypes.c_void_p(1 << 20)          # any aligned non-null address: the checks return before anything is launched or read
    # vt_kl_forward: missing outputs, bad d, misaligned z, row count not a multiple of the batch, short bf16 stride
    assert L.vt_kl_forward(p16, 16, 64, 8, 2, 0, None, None, None, None, 0, None, None, p16, None) == -1 and "vt_kl_forward" in _err()
    assert L.vt_kl_forward(p16, 16, 64, 6, 2, 0, None, None, None, None, 0, None, p16, p16, None) == -1 and "d=6" in _err()
    assert L.vt_kl_forward(ctypes.c_void_p((1 << 20) + 4), 16, 64, 8, 2, 0, None, None, None, None, 0, None, p16, p16, None) == -1
    assert L.vt_kl_forward(p16, 16, 63, 8, 2, 0, None, None, None, None, 0, None, p16, p16, None) == -1 and "batch" in _err()
    assert L.vt_kl_forward(p16, 16, 64, 8, 2, 0, None, None, None, p16, 4, None, p16, p16, None) == -1 and "ldp" in _err()
    assert L.vt_kl_forward(p16, 8, 64, 8, 2, 0, None, None, None, None, 0, None, p16, p16, None) == -1 and "ldz" in _err()
    # vt_kl_backward: no output, bad ldp, misaligned dz
    assert L.vt_kl_backward(p16, 8, None, None, p16, 16, p16, 64, 8, 2, None, None, 0, None) == -1 and "vt_kl_backward" in _err()
    assert L.vt_kl_backward(p16, 8, None, None, p16, 16, p16, 64, 8, 2, None, p16, 8, None) == -1 and "ldp" in _err()
    assert L.vt_kl_backward(p16, 8, None, None, p16, 16, p16, 64, 8, 2, ctypes.c_void_p((1 << 20) + 8), None, 0, None) == -1
    # engine: create_kl validates like create (but ignores K); a KL handle refuses the VQ entry points and vice versa
    bad = _cfg()
    bad.d = 12
    h = ctypes.c_void_p()
    assert L.vt_tokenizer_create_kl(ctypes.byref(bad), ctypes.byref(h)) == -1 and "vt_tokenizer_create_kl" in _err()
    c = _cfg()
    c.K = 0
    hk, hv = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vt_tokenizer_create_kl(ctypes.byref(c), ctypes.byref(hk)) == 0
    assert L.vt_tokenizer_create(ctypes.byref(c), ctypes.byref(hv)) == -1      # K = 0 is only ignored by a KL handle
    c.K = 512
    assert L.vt_tokenizer_create(ctypes.byref(c), ctypes.byref(hv)) == 0
    try:
        P = vt.hip.TokenizerTensors()
        ok, okv = vt.hip.TokenizerKLOutputs(), vt.hip.TokenizerOutputs()
        assert L.vt_tokenizer_encode_kl(hv, ctypes.byref(P), p16, p16, ctypes.byref(ok), 0, None) == -1 and "VQ" in _err()
        assert L.vt_tokenizer_encode(hk, ctypes.byref(P), p16, p16, ctypes.byref(okv), 0, None) == -1 and "KL" in _err()
        assert L.vt_tokenizer_codes_to_encoded(hk, ctypes.byref(P), p16, p16, p16, None) == -1 and "KL" in _err()
        assert L.vt_tokenizer_encode_kl(hk, ctypes.byref(P), p16, p16, ctypes.byref(ok), 0, None) == -1 and "loss_kl" in _err()
    finally:
        L.vt_tokenizer_destroy(hk)
        L.vt_tokenizer_destroy(hv)


def test_create_kl_plans_config_b():
    """pure host planning at config B, 8 clips: the KL handle drops the quantizer's buffers (K x d codebook copies, its workspace)
    and plans the noise; stage count as for VQ"""
    L = vt.hip.lib()
    c = _cfg("B", 8)
    hk, hv = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vt_tokenizer_create_kl(ctypes.byref(c), ctypes.byref(hk)) == 0
    assert L.vt_tokenizer_create(ctypes.byref(c), ctypes.byref(hv)) == 0
    try:
        wk, wv = L.vt_tokenizer_workspace_bytes(hk), L.vt_tokenizer_workspace_bytes(hv)
        assert 0 < wk < wv < (64 << 30), (wk, wv)
        assert L.vt_tokenizer_num_backward_stages(hk) == L.vt_tokenizer_num_backward_stages(hv) == 27
    finally:
        L.vt_tokenizer_destroy(hk)
        L.vt_tokenizer_destroy(hv)


# ---- the stream-order ledger of a KL handle --------------------------------------------------------------------------------------
KL_SRC = os.path.join(ROOT, "tests", "c", "engine_ledger_kl.hip")
KL_LIB = os.path.join(LG.BUILD, "libvt_engine_ledger_kl.so")


def build_kl_ledger():
    LG.build()                                   # the product objects and the plain stand-in (cached)
    objs = [os.path.join(LG.PKG, "_obj", "vt_engine.o"), os.path.join(LG.PKG, "_obj", "vt_api.o")]
    stub = os.path.join(LG.BUILD, "engine_ledger_kl.o")
    deps = [KL_SRC, LG.SRC, os.path.join(LG.PKG, "csrc", "vt_common.h"), os.path.join(ROOT, "include", "vt_hip.h")]
    if not os.path.exists(stub) or any(os.path.getmtime(d) > os.path.getmtime(stub) for d in deps):
        subprocess.check_call([LG.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-c", KL_SRC, "-o", stub])
    if not os.path.exists(KL_LIB) or any(os.path.getmtime(o) > os.path.getmtime(KL_LIB) for o in objs + [stub]):
        subprocess.check_call([LG.HIPCC, "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", KL_LIB] + objs + [stub])
    return KL_LIB


class KLLedger(LG.Ledger):
    """tests/ledger.Ledger over the stand-in that also records vt_kl_forward / vt_kl_backward"""

    def __init__(self):
        self.lib = ctypes.CDLL(build_kl_ledger())
        L = self.lib
        L.vt_ledger_size.restype = ctypes.c_int64
        L.vt_ledger_get.restype = ctypes.c_int64
        L.vt_ledger_get.argtypes = [ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64]
        L.vt_ledger_note_access.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
        L.vt_ledger_note_record.restype = ctypes.c_uint64
        L.vt_ledger_note_record.argtypes = [ctypes.c_uint64]
        L.vt_ledger_note_wait.argtypes = [ctypes.c_uint64, ctypes.c_uint64]


needs_hipcc = pytest.mark.skipif(shutil.which(LG.HIPCC) is None and not os.path.exists(LG.HIPCC), reason="needs hipcc to link the recording engine")


@pytest.fixture(scope="module")
def klg():
    return KLLedger()


def _bind(klg, monkeypatch):
    """tests/test_engine_ledger_cpu.host_on_ledger over the KL stand-in"""
    from video_tokenizer_amd import engine as E
    from video_tokenizer_amd import hip
    L = klg.lib
    for name, (res, args) in hip.ENGINE_SIGNATURES.items():
        if name.startswith("vt_tokenizer_"):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    L.vt_last_error.restype, L.vt_last_error.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]
    monkeypatch.setattr(hip, "_lib", L)
    monkeypatch.setattr(hip, "ptr", lambda t: None if t is None else ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(LG.MAIN))
    monkeypatch.setattr(E, "_check_video", lambda m, x: x.contiguous().float())

    def param_struct(self):
        named = self._named()
        return E._Tensors(self.model, lambda n: named[n].data_ptr() if named.get(n) is not None else None)
    monkeypatch.setattr(E.TokenizerEngine, "param_struct", param_struct)
    return vt, E


def _kl_model(name="tiny", **over):
    cfg = O.make_cfg(name, **over)
    return vt.make(K.kl_spec(cfg)), cfg


@needs_hipcc
@pytest.mark.parametrize("reducer,side,tail", [(False, False, 0), (True, True, 3), (True, False, 3)],
                         ids=["single-stream", "dp-side-stream-tail3", "dp-until-flush-tail3"])
def test_kl_schedule_has_no_race(klg, monkeypatch, reducer, side, tail):
    from tests import test_engine_ledger_cpu as T
    _, E = _bind(klg, monkeypatch)
    model, cfg = _kl_model()
    red = T.fake_reducer(klg, 1024) if reducer else None
    ops = T.run_steps(klg, E, model, cfg, 2, steps=2, reducer=red, side=side, tail=tail)
    names = [o.name for o in ops]
    assert names.count("kl_forward") == 2 and names.count("kl_backward") == 2
    assert not any(n.startswith("UNMODELLED") or n.startswith("vq_") for n in names)
    if not reducer:
        assert {o.stream for o in ops} == {LG.MAIN}
    else:
        assert LG.COMM in {o.stream for o in ops} and (LG.SIDE in {o.stream for o in ops}) == side
        total = sum(p.numel() for p in model.parameters())
        assert red.launched[-1][1] == total
    bad, n = LG.races(ops)
    assert not bad, (n, bad)
