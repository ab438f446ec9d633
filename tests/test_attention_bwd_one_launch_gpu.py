"""The non-causal attention backward (attn_delta_kernel, then dK/dV and dQ workgroups in one launch of attn_bwd_kernel) returns the bits
that the two separate launches of the parent commit returned: dqkv (cross: dq, dk, dv) and the delta workspace, torch.equal on the raw
bits against tests/golden/attn_bwd_parent_*.npz (recorded by tests/golden/make_golden_attn_bwd_parent.py under the parent's library).
Shapes and what each covers: tests/attn_bwd_parent_cases.py.  Accuracy against the oracle stays with tests/test_attention_edges_gpu.py,
tests/test_cross_attention_gpu.py and the model parity tests."""
import numpy as np
import pytest
import torch

from tests import attn_bwd_parent_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import video_tokenizer_amd.hip as h
    h.lib()
    return h


def as_ints(a):
    """raw bits as an integer tensor (a NaN would still compare equal to itself)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int32))


@pytest.mark.parametrize("name", list(P.CASES))
def test_bits_of_the_parent_commit(hip, name):
    want, got = P.load(name), P.run(hip, name)
    assert set(want) == set(got)
    for k in sorted(want):
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        w, g = as_ints(want[k]), as_ints(got[k])
        print(f"{name} {k} {tuple(g.shape)} differing elements {int((w != g).sum())}")
        assert torch.equal(w, g), (name, k)


def test_second_call_repeats_every_bit(hip):
    a, b = P.run(hip, "p130"), P.run(hip, "p130")
    for k in a:
        assert torch.equal(as_ints(a[k]), as_ints(b[k])), k
