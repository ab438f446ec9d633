"""varlen.Attn on the GPU against the fixture the reference's own code wrote (tests/golden/make_golden_varlen.py).

Tolerance, from the reference alone (the rule of tests/test_design_gpu.py): for y, dx and every parameter gradient the relative L2 distance to
the reference's fp32 result is at most 2 x the distance of the reference's OWN autocast-bf16 CPU run from it (`<tensor>_bf16_dist` in the
fixture).  The HIP path rounds where autocast does, differs in summation order and reads fp32 rotary tables where the reference multiplies
in complex128; the factor 2 is the headroom for that.  Each case prints `RATIO <case> <tensor> <distance> <bf16_dist> <ratio>` first.

Measured ratios on an MI355X (distance / bf16_dist, bar 2):
  h6_2: y 1.016, dx 1.006, pre_ln.weight 1.016, pre_ln.bias 1.018, to_qkv 0.983, q_norm.weight 0.451, q_norm.bias 0.398,
        k_norm.weight 0.622, k_norm.bias 0.538, out_proj 0.975
  h4_2: y 1.016, dx 1.007, pre_ln.weight 1.013, pre_ln.bias 1.010, to_qkv 0.981, q_norm.weight 0.707, q_norm.bias 0.422,
        k_norm.weight 0.836, k_norm.bias 0.731, out_proj 0.981
  h2_2: y 1.021, dx 1.026, pre_ln.weight 1.022, pre_ln.bias 1.024, to_qkv 1.000, q_norm.weight 0.909, q_norm.bias 0.804,
        k_norm.weight 0.988, k_norm.bias 0.717, out_proj 0.982
"""
import pytest
import torch

from tests import varlen_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _layer(case):
    import video_tokenizer_amd as vt
    c = R.CASES[case]
    I = {k: torch.from_numpy(v) for k, v in R.case_inputs(case).items()}
    m = vt.varlen.Attn(c["dim"], list(c["heads"]))
    m.load_state_dict({n: I[n] for n in R.PARAM_NAMES}, strict=True)     # the reference's keys
    _, cos, sin = vt.varlen.rope_freqs(c["grids"], c["tokens"], device="cuda")
    return m.cuda(), I, (cos, sin)


def _step(m, I, freqs, cu, rows=slice(None)):
    x = I["x"][rows].cuda().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(x, freqs, cu, None)
    (y * I["w"][rows].cuda()).sum().backward()
    torch.cuda.synchronize()
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"d_" + n: p.grad for n, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("case", list(R.CASES))
def test_layer_matches_the_reference_within_its_own_bf16_distance(golden, case):
    m, I, freqs = _layer(case)
    assert tuple(m.state_dict()) == tuple(str(golden["state_dict_keys"]).split("\n")) == R.PARAM_NAMES
    assert [",".join(str(d) for d in v.shape) for v in m.state_dict().values()] == str(golden[f"{case}/state_dict_shapes"]).split("\n")
    cu = R.cu_seqlens(case)
    out = _step(m, I, freqs, cu)
    assert out["y"].dtype == torch.float32 and out["dx"].dtype == torch.float32
    failures = []
    for t in R.TENSORS:
        want = torch.from_numpy(golden[f"{case}/{t}"])
        assert out[t] is not None and tuple(out[t].shape) == tuple(want.shape), t
        d, bar = R.rel_l2(out[t].cpu(), want), float(golden[f"{case}/{t}_bf16_dist"])
        print(f"RATIO {case} {t} {d:.3e} {bar:.3e} {d / bar:.3f}")
        if not d <= 2 * bar:
            failures.append((t, d, bar))
    assert not failures, failures
    again = _step(m, I, freqs, torch.tensor(cu, device="cuda"))        # a device tensor of boundaries; a second step reproduces every bit
    for t in R.TENSORS:
        assert torch.equal(out[t], again[t]), t


def test_packed_forward_equals_per_sequence_forward(monkeypatch):
    """bit for bit: LayerNorm, the row pass and the GEMMs work row by row, the attention is bit-exact per sequence
    (tests/test_varlen_attention_gpu.py).  The automatic GEMM dispatch takes another kernel, with another summation order, for launches of
    at most 64 rows (the 7-row sequence here): both forwards are pinned to the 128x128 tile kernel so that a row's sum has one order."""
    import video_tokenizer_amd as vt
    monkeypatch.setattr(vt.hip, "GEMM_TILE", 1)
    case = "h6_2"
    m, I, (cos, sin) = _layer(case)
    cu = R.cu_seqlens(case)
    with torch.no_grad():
        y = m(I["x"].cuda(), (cos, sin), cu, None)
        for a, b in zip(cu[:-1], cu[1:]):
            one = m(I["x"][a:b].cuda(), (cos[a:b].contiguous(), sin[a:b].contiguous()), [0, b - a], None)
            assert torch.equal(y[a:b], one), (a, b)


def test_complex_table_and_cpu_refusal(golden):
    import video_tokenizer_amd as vt
    case = "h2_2"
    m, I, (cos, sin) = _layer(case)
    cu = R.cu_seqlens(case)
    freqs = torch.complex(torch.from_numpy(golden[f"{case}/freqs_re"]), torch.from_numpy(golden[f"{case}/freqs_im"]))
    with torch.no_grad():
        assert torch.equal(m(I["x"].cuda(), freqs, cu, None), m(I["x"].cuda(), (cos, sin), cu, None))
    with pytest.raises(vt.hip.HipError):
        m(I["x"], (cos, sin), cu, None)                                # a CPU tensor
