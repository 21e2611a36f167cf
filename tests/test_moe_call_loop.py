"""The Python call loops of the MXFP4 expert projections (functional.matmul_mxfp4_experts / _glu / _sum and their _grouped forms; DESIGN.md
§33), without a GPU: a recording object stands in for each binding's lib(), the device gate is opened for CPU tensors, and what is
asserted is what reaches the C ABI: how many native calls, the cut over the tokens of each, the argument count against the binding's
signature, the plan that trails the arguments on the grouped route only, and the one workspace of the sum form."""
from ctypes import c_void_p

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _moegemm_native as gn, _moemlp_native as mlpn
from mps_bitsandbytes_amd import functional as F

T, A, E, N, K = 5, 3, 4, 8, 64
CUT = 2                                                      # tokens per native call once the pairs of a call are patched to CUT * A
CUTS = [(0, 2), (2, 4), (4, 5)]                              # three calls, the last one short
BYTES = 256                                                  # what the recorder answers for plan_bytes and workspace_bytes


class Recorder:
    """lib() of a binding: every entry point records (name, args) in the one log of a test and succeeds"""
    def __init__(self, log):
        self.log = log

    def __getattr__(self, entry):
        def call(*args):
            self.log.append((entry, args))
            return BYTES if entry.endswith("_bytes") else 0
        return call


@pytest.fixture
def log(monkeypatch):
    calls = []
    for native in (moen, mlpn, gn):
        monkeypatch.setattr(native, "lib", lambda calls=calls: Recorder(calls))
    monkeypatch.setattr(moen, "MAX_PAIRS", CUT * A)
    monkeypatch.setattr(mlpn, "MAX_PAIRS", CUT * A)
    monkeypatch.setattr(F, "MOE_GROUPED_MAX_PAIRS", CUT * A)
    monkeypatch.setattr(F, "_check_device", lambda tensor, operation="operation": None)
    monkeypatch.setattr(F, "stream_ptr", lambda device: c_void_p(0))
    return calls


def _operands(dtype=torch.bfloat16):
    return dict(x=torch.zeros(T, K, dtype=dtype), h=torch.zeros(T, A, K, dtype=dtype), w=torch.zeros(E, N, K // 2, dtype=torch.uint8),
                s=torch.zeros(E, N, K // 32, dtype=torch.uint8), ids=torch.zeros(T, A, dtype=torch.int32), rw=torch.zeros(T, A),
                bias=torch.zeros(E, N))


def _value(p):
    return (p.value or 0) if isinstance(p, c_void_p) else p


def _launches(log, entry):
    return [args for name, args in log if name == entry]


def _check_calls(log, native, entry, ids, ids_at, plans=None):
    """the calls of `entry`: one per cut, the signature's argument count, the ids of the cut, the plan at the end or no plan at all"""
    calls = _launches(log, entry)
    assert len(calls) == len(CUTS), entry
    for args, (t0, t1), q in zip(calls, CUTS, plans or [None] * len(CUTS)):
        assert len(args) == len(native._SIGNATURES[entry][1]), entry
        assert args[1] == t1 - t0 and args[2] == A, (entry, args[1:3])
        assert _value(args[ids_at]) == ids.data_ptr() + t0 * A * 4, (entry, t0)
        assert _value(args[-1]) == 0                         # the stream
        if native is gn:
            assert args[-2] == q.numel() == BYTES and _value(args[-3]) == q.data_ptr(), entry
    return calls


FORMS = {    # form -> (decode binding, its entry point, the grouped one, where the ids stand among the arguments)
    "plain": (moen, "mbnb_moe_mxfp4_experts", "mbnb_moegemm_experts", 10),
    "glu": (mlpn, "mbnb_moemlp_gate_up_glu", "mbnb_moegemm_gate_up_glu", 9),
    "sum": (mlpn, "mbnb_moemlp_down_sum", "mbnb_moegemm_down_sum", 9),
}


def _run(form, o, grouped_api, **kw):
    if form == "plain":
        f = bnb.matmul_mxfp4_experts_grouped if grouped_api else bnb.matmul_mxfp4_experts
        return f(o["x"], o["w"], o["s"], o["ids"], o["bias"], **kw)
    if form == "glu":
        f = bnb.matmul_mxfp4_experts_grouped_glu if grouped_api else bnb.matmul_mxfp4_experts_glu
        return f(o["x"], o["w"], o["s"], o["ids"], o["bias"], **kw)
    f = bnb.matmul_mxfp4_experts_grouped_sum if grouped_api else bnb.matmul_mxfp4_experts_sum
    return f(o["h"], o["w"], o["s"], o["ids"], o["rw"], o["bias"], **kw)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_decode_route_cuts_over_the_tokens_and_passes_no_plan(form, log, monkeypatch):
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
    native, entry, grouped_entry, ids_at = FORMS[form]
    o = _operands()
    out = _run(form, o, False)
    assert tuple(out.shape) == {"plain": (T, A, N), "glu": (T, A, N // 2), "sum": (T, N)}[form] and out.dtype == torch.bfloat16
    calls = _check_calls(log, native, entry, o["ids"], ids_at)
    assert {name for name, _ in log} == {entry} | ({"mbnb_moemlp_workspace_bytes"} if form == "sum" else set())
    assert len(gn._SIGNATURES[grouped_entry][1]) == len(native._SIGNATURES[entry][1]) + 2          # the plan and its bytes, nothing else
    if form == "sum":                                        # one workspace, sized for the first (largest) cut and reused
        assert _launches(log, "mbnb_moemlp_workspace_bytes") == [(CUT, A, N)]
        assert len({_value(args[16]) for args in calls}) == 1 and all(args[17] == BYTES for args in calls) and _value(calls[0][16]) != 0


@pytest.mark.parametrize("automatic", [False, True])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_grouped_route_cuts_the_same_way_and_the_plan_trails_the_arguments(form, automatic, log, monkeypatch):
    """through the _grouped function, and through the automatic one from MOE_GROUPED_MIN_PAIRS pairs up"""
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", 1 if automatic else None)
    native, entry, grouped_entry, ids_at = FORMS[form]
    o = _operands(torch.float16)
    plans = None if automatic else [torch.zeros(BYTES, dtype=torch.uint8) for _ in CUTS]
    _run(form, o, not automatic, **({} if automatic else {"plan": plans}))
    if automatic:                                            # the plans are built here: one mbnb_moegemm_plan per cut, its buffer the one passed on
        built = _launches(log, "mbnb_moegemm_plan")
        assert [(args[1], args[2], args[4]) for args in built] == [((t1 - t0) * A, E, BYTES) for t0, t1 in CUTS]
        calls = _launches(log, grouped_entry)
        assert [_value(args[-3]) for args in calls] == [_value(args[3]) for args in built]
        assert [args[-2] for args in calls] == [BYTES] * len(CUTS) and len(calls) == len(CUTS)
        assert all(len(args) == len(gn._SIGNATURES[grouped_entry][1]) and args[1] == t1 - t0 for args, (t0, t1) in zip(calls, CUTS))
    else:
        calls = _check_calls(log, gn, grouped_entry, o["ids"], ids_at, plans)
        assert not _launches(log, "mbnb_moegemm_plan")
    assert not _launches(log, entry)                         # nothing went to the decode library
    if form == "sum":
        assert _launches(log, "mbnb_moegemm_workspace_bytes") == [(CUT * A, N)] and not _launches(log, "mbnb_moemlp_workspace_bytes")
        assert len({_value(args[16]) for args in calls}) == 1 and all(args[17] == BYTES for args in calls)
    else:
        assert not [name for name, _ in log if "workspace" in name]


def test_the_limits_of_an_automatic_function_are_its_decode_binding_s(log, monkeypatch):
    """A beyond the decode launch's pairs is refused even where the grouped route would take the call; matmul_mxfp4_experts has no
    limit on E on the decode route, so more experts than the grouped library takes stay there"""
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", 1)
    o = _operands()
    monkeypatch.setattr(mlpn, "MAX_PAIRS", A - 1)
    with pytest.raises(ValueError, match="slots per token exceed"):
        _run("glu", o, False)
    _run("glu", o, True)                                     # the grouped function's own limit is the grouped library's
    assert _launches(log, "mbnb_moegemm_gate_up_glu")
    del log[:]
    monkeypatch.setattr(gn, "MAX_EXPERTS", E - 1)
    _run("plain", o, False)
    assert len(_launches(log, "mbnb_moe_mxfp4_experts")) == len(CUTS) and not _launches(log, "mbnb_moegemm_experts")


def test_an_empty_call_makes_no_native_call(log, monkeypatch):
    for threshold in (None, 1):
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", threshold)
        o = {k: (v[:0] if k in ("x", "h", "ids", "rw") else v) for k, v in _operands().items()}
        for form in FORMS:
            for grouped_api in (False, True):
                out = _run(form, o, grouped_api)
                assert out.shape[0] == 0
        out = bnb.matmul_mxfp4_experts_sum(torch.zeros(2, 0, K, dtype=torch.bfloat16), o["w"], o["s"], torch.zeros(2, 0, dtype=torch.int32),
                                           torch.zeros(2, 0))
        assert tuple(out.shape) == (2, N) and (out == 0).all()  # tokens without a slot: zeros, before any route is chosen
    assert log == []


def test_a_caller_s_plan_is_held_against_the_cuts(log, monkeypatch):
    o = _operands()
    good = [torch.zeros(BYTES, dtype=torch.uint8) for _ in CUTS]
    for bad in (good[:2], good + good[:1], [q[:-1] for q in good], [q.to(torch.int8) for q in good], good[0], [q.repeat(2)[::2] for q in good]):
        with pytest.raises(ValueError, match="plan must be what moe_grouped_plan returned"):
            _run("glu", o, True, plan=bad)
    assert not _launches(log, "mbnb_moegemm_gate_up_glu")


def test_moe_mlp_mxfp4_builds_one_plan_per_cut_and_both_projections_share_it(log, monkeypatch):
    """(Before the call loops were shared this one could not run without a GPU: moe_mlp_mxfp4 asked for cuda ids before it planned.
    Every other test of this file gives the same figures on the code before.)"""
    o = _operands()
    gate_up = (torch.zeros(E, 64, K // 2, dtype=torch.uint8), torch.zeros(E, 64, K // 32, dtype=torch.uint8), None)  # I = 32
    down = (torch.zeros(E, 6, 16, dtype=torch.uint8), torch.zeros(E, 6, 1, dtype=torch.uint8), None)                 # [E, 6, 32]: h is [T, A, 32]
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", 1)
    out = bnb.moe_mlp_mxfp4(o["x"], *gate_up, *down, o["ids"], o["rw"])
    assert tuple(out.shape) == (T, 6)
    built = _launches(log, "mbnb_moegemm_plan")
    assert len(built) == len(CUTS)
    up_calls, down_calls = _launches(log, "mbnb_moegemm_gate_up_glu"), _launches(log, "mbnb_moegemm_down_sum")
    assert [_value(a[-3]) for a in up_calls] == [_value(a[-3]) for a in down_calls] == [_value(a[3]) for a in built]
    del log[:]
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
    bnb.moe_mlp_mxfp4(o["x"], *gate_up, *down, o["ids"], o["rw"])
    assert {name for name, _ in log} == {"mbnb_moemlp_gate_up_glu", "mbnb_moemlp_workspace_bytes", "mbnb_moemlp_down_sum"}
