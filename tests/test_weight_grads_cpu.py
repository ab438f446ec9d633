"""functional._WeightGrads (the queue of transposed GEMMs of one backward) and functional._needs / _grads (gradients by the name of the
forward's argument) on the CPU: `vt.hip.gemm_tn_grouped` is replaced by a recording stand-in, the way tests/test_packs_cpu.py replaces
pack_weight, so what reaches the grouped launch -- which problems, in which order, padded how -- is pinned without a GPU."""
import ast
import inspect
import textwrap
import types

import pytest
import torch

import video_tokenizer_amd as vt
from video_tokenizer_amd import functional as F_


@pytest.fixture
def launches(monkeypatch):
    """one entry per hip.gemm_tn_grouped call: the list of problems it was handed"""
    calls = []
    monkeypatch.setattr(vt.hip, "gemm_tn_grouped", lambda problems: calls.append(list(problems)))
    return calls


def operands(M, P, Q, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (M, P), generator=g).to(torch.bfloat16), torch.randint(-3, 4, (M, Q), generator=g).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------ _WeightGrads
def test_problems_arrive_in_the_order_they_were_added(launches):
    wg = F_._WeightGrads()
    pairs = [operands(64, 8 * (i + 1), 16 * (i + 1), i) for i in range(3)]
    outs = [wg.add(dY, X) for dY, X in pairs]
    assert not launches                                                # add() only queues
    wg.run()
    assert len(launches) == 1 and len(launches[0]) == 3
    for job, out, (dY, X) in zip(launches[0], outs, pairs):
        assert job["A"] is dY and job["B"] is X and job["out"] is out  # M % 64 == 0: the operands themselves, no copy
        assert out.shape == (dY.shape[1], X.shape[1]) and out.dtype == torch.float32


def test_an_unwanted_problem_is_neither_queued_nor_allocated(launches, monkeypatch):
    wg = F_._WeightGrads()
    dY, X = operands(130, 8, 16, 0)
    first = wg.add(dY, X)
    dY2, X2 = operands(130, 24, 8, 1)

    def refuse(*a, **kw):
        raise AssertionError("an unwanted problem allocated a tensor")

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", refuse)
        m.setattr(torch, "zeros", refuse)
        assert wg.add(dY2, X2, want=False) is None
    wg.run()
    assert len(launches) == 1 and [job["out"] for job in launches[0]] == [first]


def test_ragged_rows_are_zero_padded_to_the_next_multiple_of_64(launches):
    wg = F_._WeightGrads()
    dY, X = operands(130, 136, 72, 2)
    out = wg.add(dY, X)
    wg.run()
    assert len(launches) == 1 and len(launches[0]) == 1
    job = launches[0][0]
    for padded, t in ((job["A"], dY), (job["B"], X)):
        assert padded.shape == (192, t.shape[1]) and padded.dtype == t.dtype
        assert torch.equal(padded[:130], t) and not padded[130:].any()
    assert out.shape == (136, 72)


def test_a_tensor_two_problems_read_is_padded_once(launches):
    wg = F_._WeightGrads()
    dY, X = operands(130, 8, 16, 3)
    dY2, _ = operands(130, 24, 8, 4)
    wg.add(dY, X)
    wg.add(dY2, X)
    wg.add(dY, dY2)
    wg.run()
    assert len(launches) == 1
    a, b, c = launches[0]
    assert a["B"] is b["B"] and a["A"] is c["A"] and b["A"] is c["B"]
    assert a["A"] is not a["B"] and a["B"] is not X


def test_seventeen_problems_go_out_as_sixteen_and_one(launches):
    assert vt.hip.TN_MAX_GROUP == 16
    wg = F_._WeightGrads()
    outs = [wg.add(*operands(64, 8, 8, i)) for i in range(17)]
    wg.run()
    assert [len(c) for c in launches] == [16, 1]
    assert all(job["out"] is out for job, out in zip(launches[0] + launches[1], outs))


def test_an_empty_queue_makes_no_call(launches):
    wg = F_._WeightGrads()
    assert wg.add(*operands(64, 8, 8, 0), want=False) is None
    wg.run()
    assert not launches


# ------------------------------------------------------------------------------------------------------------------ _needs / _grads
class _Probe(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, weight, bias, eps):
        return x


def _ctx(*need):
    return types.SimpleNamespace(needs_input_grad=tuple(need))


def test_grads_have_the_arity_and_order_of_the_forward():
    ctx = _ctx(True, False, True, True, False)
    assert F_._needs(ctx, _Probe) == dict(x=True, cos=False, weight=True, bias=True, eps=False)
    assert F_._grads(ctx, _Probe, bias="db", x="dx", weight="dw") == ("dx", None, "dw", "db", None)
    assert F_._grads(ctx, _Probe, x="dx") == ("dx", None, None, None, None)


def test_an_unneeded_argument_is_none_even_when_a_value_was_passed():
    assert F_._grads(_ctx(True, False, False, True, False), _Probe, x="dx", cos="dcos", weight="dw", bias="db") == ("dx", None, None, "db", None)


def test_a_name_the_forward_does_not_have_raises():
    with pytest.raises(KeyError, match="wieght"):
        F_._grads(_ctx(True, True, True, True, True), _Probe, x="dx", wieght="dw")


def _function_classes():
    seen = {}
    for mod in vars(vt).values():
        if isinstance(mod, types.ModuleType) and mod.__name__.startswith(vt.__name__ + "."):
            for cls in vars(mod).values():
                if isinstance(cls, type) and issubclass(cls, torch.autograd.Function) and cls.__module__ == mod.__name__:
                    seen[cls.__qualname__] = cls
    return seen


def _named_calls(cls, helper):
    """the `helper(ctx, Cls, name=..., ...)` calls in cls.backward: [(the class named, the keyword names)]"""
    tree = ast.parse(textwrap.dedent(inspect.getsource(cls.backward)))
    return [(c.args[1].id, [k.arg for k in c.keywords]) for c in ast.walk(tree)
            if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == helper]


def test_every_function_names_only_arguments_its_forward_has():
    """walks the package's autograd Functions: a misspelt name in a `_grads(...)` call or a `need["..."]` look-up fails here, not in a backward
    on the GPU"""
    users = []
    for name, cls in _function_classes().items():
        args = set(F_._forward_args(cls))
        calls = _named_calls(cls, "_grads") + _named_calls(cls, "_needs")
        for named, keywords in calls:
            assert named == name, f"{name}.backward names {named}"
            assert None not in keywords and set(keywords) <= args, (name, sorted(set(keywords) - args))
        if calls:
            users.append(name)
            src = ast.parse(textwrap.dedent(inspect.getsource(cls.backward)))
            looked_up = {n.slice.value for n in ast.walk(src) if isinstance(n, ast.Subscript) and isinstance(n.value, ast.Name)
                         and n.value.id == "need" and isinstance(n.slice, ast.Constant)}
            assert looked_up <= args, (name, sorted(looked_up - args))
    assert {"Linear", "PatchEmbed", "CrossAttentionLayer", "SelfAttentionLayer", "FeedForwardLayer", "VarlenAttentionLayer", "_AttnBranch",
            "_FfnBranch", "StatGate", "ConvTransposePatch", "ResidualScale", "RMSNormRows", "RMSNormF32", "LayerNormRows"} <= set(users)
