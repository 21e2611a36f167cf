"""CPU-side checks of SwitchBackLinear and libmbnb_train.so, without a GPU: the C ABI (loads, exports what include/mbnb_train.h declares,
argument errors return a status before any device access, the workspace queries are host arithmetic), the kernel-name table against
tests/switchback_cases.py, and the module's surface against the reference's (nn/switchback.py)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch
from torch import nn

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _train_native
from mps_bitsandbytes_amd import functional as F
from tests import forms, switchback_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "train_kernels.hip")
ONE = ctypes.c_void_p(256)        # any non-NULL, 256-byte aligned value: validation must fail before a dereference


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "mbnb_train.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text)))


# ----------------------------------------------------------------------------- the C ABI
def test_library_exports_exactly_the_header():
    lib = _train_native.lib()
    names = _declared_symbols()
    assert len(names) == 8
    assert sorted(_train_native.EXPORTED_SYMBOLS) == names, "python binding and header disagree"
    out = subprocess.run(["nm", "-D", "--defined-only", _train_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)$", out, flags=re.M))) == names
    assert lib.mbnb_train_abi_version() == _train_native.ABI_VERSION == 1
    assert re.search(r"#define MBNB_TRAIN_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "mbnb_train.h")).read())


def test_library_uses_the_public_gemm_and_leaves_the_frozen_library_alone():
    """libmbnb_train.so imports libmbnb_hip's public entry points only, and libmbnb_hip.so exports nothing of this library."""
    out = subprocess.run(["nm", "-D", "--undefined-only", _train_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    imported = set(re.findall(r"\b(mbnb_[a-z0-9_]+)$", out, flags=re.M))
    assert imported == {"mbnb_gemm_dense", "mbnb_gemm_dense_workspace_bytes", "mbnb_last_error"}
    from mps_bitsandbytes_amd import _native
    hip = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"switchback|grad_weight|mbnb_train", hip)


def test_argument_errors_return_a_status_before_any_device_access():
    lib = _train_native.lib()
    fwd, gw = lib.mbnb_switchback_forward, lib.mbnb_linear_grad_weight
    assert fwd(ONE, 7, 4, 64, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1 and b"dtype" in lib.mbnb_train_last_error()
    assert fwd(ONE, 0, 4, 64, ONE, ONE, 8, None, ONE, None, 0, 4, None) == -1 and b"flags" in lib.mbnb_train_last_error()
    assert fwd(ONE, 0, -1, 64, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1 and b"negative" in lib.mbnb_train_last_error()
    assert fwd(None, 0, 4, 64, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1 and b"NULL" in lib.mbnb_train_last_error()
    assert fwd(ONE, 0, 4, 64, None, ONE, 8, None, ONE, None, 0, 0, None) == -1
    assert fwd(ONE, 0, 4, 0, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -2
    assert fwd(ctypes.c_void_p(257), 0, 4, 64, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1 and b"aligned" in lib.mbnb_train_last_error()
    assert fwd(ONE, 0, 1 << 30, 1 << 20, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -2 and b"too large" in lib.mbnb_train_last_error()
    assert gw(ONE, ONE, 4, 8, 64, 3, ONE, None, 0, 0, None) == -1 and b"dtype" in lib.mbnb_train_last_error()
    assert gw(ONE, ONE, 4, 8, 64, 0, ONE, None, 0, 8, None) == -1 and b"flags" in lib.mbnb_train_last_error()
    assert gw(ONE, ONE, -4, 8, 64, 0, ONE, None, 0, 0, None) == -1
    assert gw(None, ONE, 4, 8, 64, 0, ONE, None, 0, 0, None) == -1 and b"NULL" in lib.mbnb_train_last_error()
    assert gw(ONE, ONE, 4, 8, 64, 0, ctypes.c_void_p(257), None, 0, 0, None) == -1 and b"aligned" in lib.mbnb_train_last_error()
    # the transposing pass alone takes 16-bit data only
    assert gw(None, ONE, 4, 0, 64, 2, ONE, None, 0, 1, None) == -3 and b"16-bit" in lib.mbnb_train_last_error()
    # empty problems are a no-op success that names the route
    assert fwd(None, 0, 0, 64, None, None, 8, None, None, None, 0, 0, None) == 0
    assert lib.mbnb_train_last_kernel() == b"switchback_generic"
    assert gw(None, None, 4, 0, 64, 0, None, None, 0, 0, None) == 0
    assert lib.mbnb_train_last_kernel() == b"grad_w_generic"
    with pytest.raises(RuntimeError, match="status -1"):
        _train_native.check(-1, "unit")


def test_workspace_queries_are_host_arithmetic():
    lib = _train_native.lib()
    q_fwd, q_gw = lib.mbnb_switchback_forward_workspace_bytes, lib.mbnb_linear_grad_weight_workspace_bytes
    assert [lib.mbnb_train_padded_rows(m) for m in (0, 1, 64, 128, 129, 4095, 4096, 4097)] == [128, 128, 128, 128, 192, 4096, 4096, 4160]
    # dense route: Wd [N, K] of 16 bits (+ split-K partials, none at these shapes)
    assert q_fwd(4096, 4096, 4096, 1) == 4096 * 4096 * 2
    assert q_fwd(4096, 11008, 4096, 0) == 11008 * 4096 * 2
    assert q_fwd(300, 5003, 192, 0) == (5003 * 192 * 2 + 255) // 256 * 256
    # generic kernel only: f32, small M / N.K, K % 64 != 0, bad arguments
    assert q_fwd(4096, 4096, 4096, 2) == 0
    # small M: the GEMM's own plan may split K, and its partials follow Wd
    from mps_bitsandbytes_amd import _native
    assert q_fwd(16, 4096, 4096, 1) == 4096 * 4096 * 2 + _native.lib().mbnb_gemm_dense_workspace_bytes(16, 4096, 4096)
    assert q_fwd(1, 16384, 8192, 1) == 16384 * 8192 * 2 + _native.lib().mbnb_gemm_dense_workspace_bytes(1, 16384, 8192)
    assert q_fwd(1, 4096, 4096, 1) == 0 and q_fwd(8, 4096, 4096, 1) == 0 and q_fwd(64, 1024, 1024, 0) == 0
    assert q_fwd(4096, 4096, 4000, 1) == 0
    assert q_fwd(4096, 4096, 4096, 9) == 0 and q_fwd(-1, 8, 8, 0) == 0
    # weight gradient: dY^T [N, Mp] + X^T [K, Mp]
    assert q_gw(4096, 4096, 4096, 1) == 2 * 4096 * 4096 * 2
    assert q_gw(4096, 4096, 11008, 1) == (4096 + 11008) * 4096 * 2
    assert q_gw(100, 1024, 2048, 0) == (1024 + 2048) * 128 * 2
    assert q_gw(17, 4096, 4096, 0) == 2 * 4096 * 128 * 2 and q_gw(1, 8192, 8256, 1) == (8192 + 8256) * 128 * 2
    assert q_gw(17, 1024, 2048, 0) == 0 and q_gw(1, 4096, 4096, 1) == 0          # small products: the generic kernel
    assert q_gw(100, 1001, 1537, 0) == ((1001 * 128 * 2 + 255) // 256 + (1537 * 128 * 2 + 255) // 256) * 256
    assert q_gw(4096, 4096, 4096, 2) == 0 and q_gw(4096, 40, 100, 0) == 0 and q_gw(-1, 8, 8, 0) == 0


# ----------------------------------------------------------------------------- kernel names
def _name_table():
    src = open(SRC).read()
    m = re.search(r"kTrainKernelNames\[\]\s*=\s*\{(.*?)\};", src, flags=re.S)
    assert m, "train_kernels.hip: the kTrainKernelNames table is gone"
    return re.findall(r'"([^"]*)"', m.group(1))


def test_every_reported_kernel_name_is_the_kernel_of_a_case():
    names = _name_table()
    assert len(names) == 6 and len(set(names)) == 6
    src = open(SRC).read()
    assert "set_kernel_name" not in src, "libmbnb_train.so reports through its own table, not libmbnb_hip's record"
    # every name reaches g_kernel through the table: no other string literal is assigned to it
    assert not re.search(r"g_kernel\s*=\s*\"[^\"]", src)
    expected = {c["kernel"] for c in switchback_cases.CASES}
    assert set(names) == expected, (sorted(set(names) - expected), sorted(expected - set(names)))


# ----------------------------------------------------------------------------- forms behind the names: variants, limits, alignment, dtypes
_code = forms.code
MARKER = "enum { KN_SB_DQ"       # the host side of train_kernels.hip begins here (tests/forms.py)


def reported_words(src):
    """Every word a variant can hold: the literals of set_variant("...") and add_variant("...")."""
    return set(re.findall(r'\b(?:set|add)_variant\("([^"]*)"\)', _code(src)))


def uncovered_words(src, cases):
    """(words no case's variant holds, words of cases that the source never reports)."""
    words, have = reported_words(src), {w for c in cases for w in c["variant"].split()}
    return sorted(words - have), sorted(have - words)


def limit_counts(src):
    return forms.limit_counts(src, MARKER)


def unclaimed_limits(src):
    counts = limit_counts(src)
    return sorted(k for k in set(counts) | set(switchback_cases.LIMIT_COUNTS) if counts.get(k) != switchback_cases.LIMIT_COUNTS.get(k))


def alignment_tests(src):
    return forms.alignment_tests(src, MARKER)


def test_every_variant_word_the_source_reports_has_a_case_and_no_case_names_another():
    src = open(SRC).read()
    assert reported_words(src) == {"dq8x4", "dq8x1", "dq1", "bias8", "bias1", "nobias", "dy8", "dy1", "x8", "x1"}
    assert uncovered_words(src, switchback_cases.CASES) == ([], [])
    have = {(c["kernel"], c["variant"]) for c in switchback_cases.CASES}
    # the words as the launchers join them: the three Wd kernels alone, each bias word behind a vector Wd pass, the four pairs of transposes
    assert {("switchback_dq", w) for w in ("dq8x4", "dq8x1", "dq1")} <= have
    assert {("switchback_dq+dense", "dq8x4 " + b) for b in ("bias8", "bias1", "nobias")} | {("switchback_dq+dense", "dq8x1 bias8")} <= have
    assert {("grad_w_t+dense", f"{a} {b}") for a in ("dy8", "dy1") for b in ("x8", "x1")} | {("grad_w_t", "x8"), ("grad_w_t", "x1")} <= have
    assert all(c["variant"] == "" for c in switchback_cases.CASES if c["kernel"].endswith("generic"))
    entries = re.findall(r"^int (mbnb_\w+)\([^{]*\{\n(.*)\n", src, flags=re.M)
    assert len(entries) == 2 and all(first.strip() == "begin_call();" for _, first in entries), entries


def test_every_case_takes_the_name_and_the_variant_the_launchers_conditions_give():
    for c in switchback_cases.CASES:
        assert switchback_cases.model(c) == (c["kernel"], c["variant"]), (switchback_cases.case_id(c), switchback_cases.model(c))
    lib = _train_native.lib()
    for M in (0, 1, 63, 64, 65, 127, 128, 129, 4095, 4097):
        assert switchback_cases.padded_rows(M) == lib.mbnb_train_padded_rows(M)
    # the restated shape conditions against the library's own workspace queries (0 where the dense route does not apply)
    for c in switchback_cases.CASES:
        if c["op"] in ("forward", "grad_w") and "off" not in c and "view" not in c and not c.get("generic"):
            q = lib.mbnb_switchback_forward_workspace_bytes if c["op"] == "forward" else lib.mbnb_linear_grad_weight_workspace_bytes
            code = {"f16": 0, "bf16": 1, "f32": 2}[c["dt"]]
            assert (q(switchback_cases.rows_of(c), c["N"], c["K"], code) > 0) == c["kernel"].endswith("+dense"), switchback_cases.case_id(c)


def test_every_threshold_has_a_case_on_each_side():
    rows = [t[0] + str(t[1]) for t in switchback_cases.THRESHOLDS]
    assert len(rows) == len(set(rows))
    for what, ops, first, second in switchback_cases.THRESHOLDS:
        cs = [(c, switchback_cases.derived(c)) for c in switchback_cases.CASES if c["op"] in ops]
        assert any(first(c, d) for c, d in cs), f"{what} {ops}: no case on the first side"
        assert any(second(c, d) for c, d in cs), f"{what} {ops}: no case on the second side"


def test_every_limit_of_the_launchers_is_claimed_by_a_threshold_or_listed_as_having_no_case():
    m = switchback_cases
    assert unclaimed_limits(open(SRC).read()) == []
    rows = {t[0] for t in m.THRESHOLDS}
    assert set(m.LIMIT_CLAIMS) == set(m.LIMIT_COUNTS)
    for lit, claim in m.LIMIT_CLAIMS.items():
        for one in (claim if isinstance(claim, list) else [claim]):
            assert one in rows or (isinstance(one, tuple) and one[0] == "no case" and one[1]), (lit, one)
    for lit in ("1 << 31", "1 << 40", "0x7FFFFFFF", "kMaxElems"):
        assert m.LIMIT_CLAIMS[lit][0] == "no case"


def _pair(op, operand):
    return forms.pair(switchback_cases.CASES, op, operand)


def test_every_pointer_a_launcher_tests_has_a_pair_of_cases_that_differ_by_its_offset_alone():
    m = switchback_cases
    assert alignment_tests(open(SRC).read()) == set(m.OPERAND_ALIGNMENT_TESTED)
    for key, (op, operand) in list(m.OPERAND_ALIGNMENT_TESTED.items()) + [(k, k) for k in m.OPERAND_ALIGNMENT_ALSO]:
        pairs = _pair(op, operand)
        assert pairs and all((c["kernel"], c["variant"]) != (b["kernel"], b["variant"]) for c, b in pairs), key


def test_every_form_has_a_case_for_each_dtype_it_is_instantiated_for():
    m = switchback_cases
    for (name, variant), dts in m.INSTANTIATED.items():
        have = {c["dt"] for c in m.CASES if (c["kernel"], c["variant"]) == (name, variant)}
        assert set(dts) <= have, (name, variant, sorted(set(dts) - have))
    assert {c["kernel"] for c in m.CASES} <= {k[0] for k in m.INSTANTIATED}


def test_the_closure_fails_on_a_variant_a_limit_or_a_pointer_test_without_a_case():
    """Three scratch edits of the source, each caught by its check."""
    m = switchback_cases
    src = open(SRC).read()
    a = src.replace('add_variant("nobias");', 'if (N > 7) add_variant("nobias");\n            else add_variant("tiny");')
    assert a != src and uncovered_words(a, m.CASES) == (["tiny"], [])
    b = src.replace("if (N <= 65535) {", "if (N <= 65535 && K >= 24) {")
    assert b != src and unclaimed_limits(b) == ["24"]
    c = src.replace("ws_bytes >= yt_bytes + xt_bytes && aligned(dW, 16);", "ws_bytes >= yt_bytes + xt_bytes && aligned(dW, 16) && aligned(X, 16);")
    assert c != src and alignment_tests(c) - set(m.OPERAND_ALIGNMENT_TESTED) == {("gw_dispatch", "X", 16)}


def test_cases_are_well_formed():
    ids = [switchback_cases.case_id(c) for c in switchback_cases.CASES]
    assert len(ids) == len(set(ids))
    for c in switchback_cases.CASES:
        assert c["op"] in ("forward", "dequant", "grad_w", "transpose"), c
        assert isinstance(c["variant"], str) and set(c) <= {"op", "kernel", "variant", "M", "N", "K", "lead", "dt", "bias", "generic", "view", "off", "special"}, c
        for operand, off in c.get("off", {}).items():
            assert 0 < off < 16 and operand in {"forward": "x w bias out ws", "dequant": "w out", "grad_w": "dy x dW ws", "transpose": "x out"}[c["op"]].split(), c
        assert c["dt"] in ("f16", "bf16", "f32"), c
        assert ("M" in c) != ("lead" in c) or c["op"] == "dequant", c


# ----------------------------------------------------------------------------- the module against the reference's surface
def test_exports():
    from mps_bitsandbytes_amd.nn import SwitchBackLinear, SwitchBackLinearCallback
    assert bnb.SwitchBackLinear is SwitchBackLinear and bnb.SwitchBackLinearCallback is SwitchBackLinearCallback
    assert {"SwitchBackLinear", "SwitchBackLinearCallback"} <= set(bnb.__all__) & set(bnb.nn.__all__)
    from mps_bitsandbytes_amd.nn.switchback import SwitchBackFunction
    assert SwitchBackFunction is F._SwitchBackFunction


def test_constructor_signature_defaults_and_state():
    sig = inspect.signature(bnb.SwitchBackLinear.__init__)
    assert list(sig.parameters) == ["self", "in_features", "out_features", "bias", "compute_dtype", "device"]
    assert sig.parameters["bias"].default is True
    assert sig.parameters["compute_dtype"].default is torch.float16
    assert sig.parameters["device"].default is None
    assert list(inspect.signature(bnb.SwitchBackLinear.from_linear).parameters) == ["linear", "device"]
    m = bnb.SwitchBackLinear(100, 48)
    assert (m.in_features, m.out_features, m.compute_dtype, m._update_int8_pending) == (100, 48, torch.float16, False)
    assert m.weight_int8.dtype == torch.int8 and m.weight_int8.shape == (48, 100) and not m.weight_int8.any()
    assert m.weight_scales.dtype == torch.float32 and m.weight_scales.shape == (48,) and bool((m.weight_scales == 1).all())
    assert isinstance(m.weight_fp, nn.Parameter) and m.weight_fp.dtype == torch.float16 and not m.weight_fp.any()
    assert isinstance(m.bias, nn.Parameter) and m.bias.dtype == torch.float16 and m.bias.shape == (48,) and not m.bias.any()
    assert list(m.state_dict()) == ["weight_fp", "bias", "weight_int8", "weight_scales"]
    assert [n for n, _ in m.named_parameters()] == ["weight_fp", "bias"]
    assert m.extra_repr() == "in_features=100, out_features=48, bias=True"
    nb = bnb.SwitchBackLinear(64, 32, bias=False, compute_dtype=torch.bfloat16)
    assert nb.bias is None
    assert list(nb.state_dict()) == ["weight_fp", "weight_int8", "weight_scales"]
    assert nb.weight_fp.dtype == torch.bfloat16
    assert repr(nb) == "SwitchBackLinear(in_features=64, out_features=32, bias=False)"


def test_a_reference_checkpoint_loads_unchanged():
    """A state dict with the reference's keys, shapes and dtypes loads into the layer, bit for bit."""
    g = torch.Generator().manual_seed(3)
    sd = {"weight_fp": torch.randn(32, 64, generator=g).half(), "bias": torch.randn(32, generator=g).half(),
          "weight_int8": torch.randint(-127, 128, (32, 64), generator=g, dtype=torch.int8), "weight_scales": torch.rand(32, generator=g)}
    m = bnb.SwitchBackLinear(64, 32)
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k


def _cpu_quantize_rowwise(calls):
    """Stands in for the HIP quantize_rowwise on CPU tensors (the reference's formula) and records what it was given."""
    def q(t):
        calls.append(t)
        t2 = t.reshape(-1, t.shape[-1]).float()
        s = t2.abs().max(dim=-1).values.clamp(min=1e-8)
        return torch.clamp(torch.round(t2 * (127.0 / s.unsqueeze(-1))), -127, 127).to(torch.int8).view(t.shape), s
    return q


@pytest.mark.parametrize("dt,want", [(torch.float32, torch.float16), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)])
def test_from_linear_dtype_rule(monkeypatch, dt, want):
    calls = []
    monkeypatch.setattr(F, "quantize_rowwise", _cpu_quantize_rowwise(calls))
    g = torch.Generator().manual_seed(5)
    lin = nn.Linear(40, 24)
    with torch.no_grad():
        lin.weight.copy_(0.05 * torch.randn(24, 40, generator=g))
    lin = lin.to(dt)
    m = bnb.SwitchBackLinear.from_linear(lin)
    assert m.compute_dtype == want and m.weight_fp.dtype == want and m.bias.dtype == want
    assert torch.equal(m.weight_fp.data, lin.weight.data.to(want))
    assert torch.equal(m.bias.data, lin.bias.data.to(want))
    # the codes come from the ORIGINAL-precision weight, not from weight_fp
    assert len(calls) == 1 and calls[0].dtype == dt and torch.equal(calls[0], lin.weight.data)
    q, s = _cpu_quantize_rowwise([])(lin.weight.data)
    assert torch.equal(m.weight_int8, q) and torch.equal(m.weight_scales, s)
    no_bias = bnb.SwitchBackLinear.from_linear(nn.Linear(40, 24, bias=False).to(dt))
    assert no_bias.bias is None


def test_callback_collects_every_switchback_layer(monkeypatch):
    model = nn.Sequential(bnb.SwitchBackLinear(16, 32), nn.ReLU(), nn.Sequential(nn.Linear(32, 32), bnb.SwitchBackLinear(32, 8, bias=False)),
                          bnb.Linear8bit(8, 8))
    cb = bnb.SwitchBackLinearCallback(model)
    assert cb.switchback_layers == [model[0], model[2][1]]
    synced = []
    monkeypatch.setattr(bnb.SwitchBackLinear, "_update_int8_weights", lambda self: synced.append(self))
    cb.sync()
    assert synced == [model[0], model[2][1]]
    assert bnb.SwitchBackLinearCallback(nn.Linear(4, 4)).switchback_layers == []


def test_update_int8_pending_as_the_reference(monkeypatch):
    """forward re-quantises only in training mode with the flag set, then clears it; nothing sets the flag."""
    synced, calls = [], []
    monkeypatch.setattr(bnb.SwitchBackLinear, "_update_int8_weights", lambda self: synced.append(self))
    monkeypatch.setattr(F, "switchback_linear", lambda *a: calls.append(a) or a[0])
    m = bnb.SwitchBackLinear(8, 4)
    x = torch.zeros(2, 8)
    m.train()
    m(x)
    assert synced == [] and m._update_int8_pending is False
    m._update_int8_pending = True
    m.eval()
    m(x)
    assert synced == [] and m._update_int8_pending is True
    m.train()
    m(x)
    assert synced == [m] and m._update_int8_pending is False
    m(x)
    assert synced == [m]
    # the forward hands the layer's own tensors to the kernel call, in the reference's argument order
    assert all(a[1] is m.weight_int8 and a[2] is m.weight_scales and a[3] is m.weight_fp and a[4] is m.bias for a in calls)
    m.sync_weights()
    assert synced == [m, m]


def test_sync_weights_requantises_weight_fp(monkeypatch):
    calls = []
    monkeypatch.setattr(F, "quantize_rowwise", _cpu_quantize_rowwise(calls))
    m = bnb.SwitchBackLinear(64, 32)
    with torch.no_grad():
        m.weight_fp.fill_(0.5)
    m.sync_weights()
    assert len(calls) == 1 and calls[0].dtype == torch.float16
    assert bool((m.weight_int8 == 127).all()) and bool((m.weight_scales == 0.5).all())


def test_functional_entry_points_refuse_cpu_tensors():
    w = torch.zeros(4, 8, dtype=torch.int8)
    with pytest.raises(ValueError, match="cuda"):
        F.switchback_linear(torch.zeros(2, 8, dtype=torch.float16), w, torch.ones(4), torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="cuda"):
        F.linear_grad_weight(torch.zeros(2, 4, dtype=torch.float16), torch.zeros(2, 8, dtype=torch.float16))
