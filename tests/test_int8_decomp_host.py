"""CPU-side checks of the col+row INT8 and COO sparse operations and libmbnb_sparse.so, without a GPU: the seven names at the package
root, the C ABI (loads, exports what include/mbnb_sparse.h declares, argument errors return a status before any device access, the
workspace queries are host arithmetic), the kernel-name table against tests/int8_decomp_cases.py, argument errors of the Python
functions with the library stubbed, the emulation of tests/int8_decomp_emul.py against the committed goldens, and the exports of the
three existing libraries."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, _optim_native, _sparse_native, _train_native
from mps_bitsandbytes_amd import functional as F
from tests import forms, int8_decomp_cases
from tests import int8_decomp_emul as emul
from tests.goldenio import DT, HERE, from_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "sparse_kernels.hip")
HEADER = os.path.join(ROOT, "include", "mbnb_sparse.h")
ONE = ctypes.c_void_p(256)        # any non-NULL, 256-byte aligned value: validation must fail before a dereference
NAMES = ["quantize_colrow", "dequantize_colrow", "matmul_colrow", "sparse_coo_from_dense", "quantize_sparse_coo", "spmm_coo", "spmm_coo_int8"]


# ----------------------------------------------------------------------------- the public surface
def test_the_seven_names_are_exported_from_the_package_root():
    for name in NAMES:
        assert getattr(bnb, name) is getattr(F, name), name
        assert name in bnb.__all__, name


def test_signatures_are_the_references():
    want = {
        "quantize_colrow": ["tensor"],
        "dequantize_colrow": ["quantized", "row_scales", "col_scales", "dtype"],
        "matmul_colrow": ["input", "weight_int8", "weight_row_scales", "weight_col_scales", "bias", "dtype"],
        "sparse_coo_from_dense": ["tensor", "threshold"],
        "quantize_sparse_coo": ["row_indices", "col_indices", "values"],
        "spmm_coo": ["row_indices", "col_indices", "values", "dense", "sparse_rows", "sparse_cols"],
        "spmm_coo_int8": ["row_indices", "col_indices", "values_int8", "values_scale", "dense", "sparse_rows", "sparse_cols", "dtype"],
    }
    for name, params in want.items():
        sig = inspect.signature(getattr(bnb, name))
        assert list(sig.parameters) == params, name
    assert inspect.signature(bnb.dequantize_colrow).parameters["dtype"].default is torch.float16
    assert inspect.signature(bnb.matmul_colrow).parameters["dtype"].default is torch.float16
    assert inspect.signature(bnb.matmul_colrow).parameters["bias"].default is None
    assert inspect.signature(bnb.spmm_coo_int8).parameters["dtype"].default is torch.float16
    assert inspect.signature(bnb.sparse_coo_from_dense).parameters["threshold"].default == 0.0


# ----------------------------------------------------------------------------- the C ABI
def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_header():
    lib = _sparse_native.lib()
    names = _declared_symbols()
    assert len(names) == 14
    assert sorted(_sparse_native.EXPORTED_SYMBOLS) == names, "python binding and header disagree"
    out = subprocess.run(["nm", "-D", "--defined-only", _sparse_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)$", out, flags=re.M))) == names
    assert lib.mbnb_sparse_abi_version() == _sparse_native.ABI_VERSION == 1
    assert re.search(r"#define MBNB_SPARSE_ABI_VERSION 1\b", open(HEADER).read())
    header = open(HEADER).read()
    for const, value in (("MBNB_SPARSE_PASS_ONLY", _sparse_native.PASS_ONLY), ("MBNB_SPARSE_FORCE_GENERIC", _sparse_native.FORCE_GENERIC)):
        assert re.search(rf"#define {const} {value}\b", header)
    assert re.search(r"MBNB_COO_VALUES = 0, MBNB_COO_INT8_SCALAR = 1, MBNB_COO_INT8_ENTRY = 2", header)
    assert (_sparse_native.COO_VALUES, _sparse_native.COO_INT8_SCALAR, _sparse_native.COO_INT8_ENTRY) == (0, 1, 2)


def test_library_uses_the_public_gemm_and_the_existing_libraries_are_unchanged():
    """libmbnb_sparse.so imports libmbnb_hip's public entry points only; the three existing libraries export exactly what their
    bindings list (nothing of this library leaked into them, nothing was dropped)."""
    out = subprocess.run(["nm", "-D", "--undefined-only", _sparse_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(mbnb_[a-z0-9_]+)$", out, flags=re.M)) == {"mbnb_gemm_dense", "mbnb_gemm_dense_workspace_bytes", "mbnb_last_error"}
    for mod, count in ((_native, 30), (_optim_native, None), (_train_native, 8)):
        mod.lib()
        defined = subprocess.run(["nm", "-D", "--defined-only", mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)$", defined, flags=re.M)))
        assert exported == sorted(mod.EXPORTED_SYMBOLS), mod.__name__
        assert count is None or len(exported) == count, (mod.__name__, len(exported))
        assert not re.search(r"colrow|mbnb_coo|spmm|mbnb_sparse", defined), mod.__name__
    assert _native.lib().mbnb_abi_version() == 2 and _train_native.lib().mbnb_train_abi_version() == 1


def test_argument_errors_return_a_status_before_any_device_access():
    lib = _sparse_native.lib()
    err = lib.mbnb_sparse_last_error
    quant, deq, mm = lib.mbnb_colrow_quantize, lib.mbnb_colrow_dequantize, lib.mbnb_colrow_matmul
    assert quant(ONE, 7, 4, 8, ONE, ONE, ONE, ONE, 1 << 20, None) == -1 and b"dtype" in err()
    assert quant(ONE, 0, -1, 8, ONE, ONE, ONE, ONE, 1 << 20, None) == -1 and b"negative" in err()
    assert quant(ONE, 0, 0, 8, ONE, ONE, ONE, ONE, 1 << 20, None) == -2 and b"empty" in err()
    assert quant(None, 0, 4, 8, ONE, ONE, ONE, ONE, 1 << 20, None) == -1 and b"NULL" in err()
    assert quant(ONE, 0, 4, 8, ONE, ONE, ONE, None, 0, None) == -1 and b"workspace" in err()
    assert quant(ONE, 0, 4, 8, ONE, ONE, ONE, ONE, 8, None) == -1 and b"workspace" in err()
    assert quant(ctypes.c_void_p(257), 0, 4, 8, ONE, ONE, ONE, ONE, 1 << 20, None) == -1 and b"aligned" in err()
    assert quant(ONE, 0, 1 << 30, 1 << 20, ONE, ONE, ONE, ONE, 1 << 20, None) == -2 and b"too large" in err()
    assert deq(ONE, ONE, ONE, 4, 8, 5, ONE, None) == -1 and b"dtype" in err()
    assert deq(None, ONE, ONE, 4, 8, 0, ONE, None) == -1 and b"NULL" in err()
    assert deq(None, None, None, 0, 8, 0, None, None) == 0 and lib.mbnb_sparse_last_kernel() == b"colrow_dequant8"
    assert mm(ONE, 0, 4, 64, ONE, ONE, ONE, 8, None, ONE, None, 0, 4, None) == -1 and b"flags" in err()
    assert mm(None, 0, 4, 64, ONE, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1 and b"NULL" in err()
    assert mm(ONE, 0, 4, 0, ONE, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -2
    assert mm(ONE, 0, -4, 64, ONE, ONE, ONE, 8, None, ONE, None, 0, 0, None) == -1
    assert mm(None, 0, 0, 64, None, None, None, 8, None, None, None, 0, 0, None) == 0 and lib.mbnb_sparse_last_kernel() == b"colrow_generic"
    count, fill, cq, spmm = lib.mbnb_coo_count, lib.mbnb_coo_fill, lib.mbnb_coo_quantize, lib.mbnb_spmm_coo
    assert count(ONE, 3, 4, 8, 0.0, ONE, None) == -1 and b"dtype" in err()
    assert count(ONE, 0, 4, 8, 0.0, None, None) == -1 and b"NULL" in err()
    assert count(ONE, 0, 4, 8, float("nan"), ONE, None) == -1 and b"NaN" in err()
    assert fill(ONE, 0, 4, 8, 0.0, ONE, ONE, ONE, ONE, 33, None) == -2 and b"more entries" in err()
    assert fill(ONE, 0, 4, 8, 0.0, ONE, None, ONE, ONE, 3, None) == -1 and b"NULL" in err()
    assert fill(None, 0, 4, 8, 0.0, None, None, None, None, 0, None) == 0 and lib.mbnb_sparse_last_kernel() == b"coo_fill"
    assert cq(ONE, 0, 0, ONE, ONE, ONE, 4096, None) == -2 and b"nnz = 0" in err()
    assert cq(ONE, 0, 5, ONE, ONE, None, 0, None) == -1 and b"workspace" in err()
    assert cq(None, 0, 5, ONE, ONE, ONE, 4096, None) == -1 and b"NULL" in err()
    big = 1 << 30
    assert spmm(ONE, 16, ONE, 64, ONE, 0, None, 5, ONE, 0, 4, 4, 8, ONE, ONE, big, 0, None) == -1 and b"int32 or int64" in err()
    assert spmm(ONE, 64, ONE, 64, ONE, 3, None, 5, ONE, 0, 4, 4, 8, ONE, ONE, big, 0, None) == -1 and b"value kind" in err()
    assert spmm(ONE, 64, ONE, 64, ONE, 0, None, 5, ONE, 0, 4, 4, 8, ONE, ONE, big, 1, None) == -1 and b"flags" in err()
    assert spmm(ONE, 64, ONE, 64, ONE, 1, None, 5, ONE, 0, 4, 4, 8, ONE, ONE, big, 0, None) == -1 and b"NULL" in err()      # int8 values, no scale
    assert spmm(ONE, 64, ONE, 64, ONE, 0, None, 5, ONE, 0, 4, 4, 8, ONE, None, 0, 0, None) == -1 and b"workspace" in err()
    assert spmm(ONE, 64, ONE, 64, ONE, 0, None, 5, ONE, 0, 4, 4, 8, ONE, ONE, 16, 0, None) == -1 and b"workspace" in err()
    assert spmm(ONE, 64, ONE, 64, ONE, 0, None, 1 << 31, ONE, 0, 4, 4, 8, ONE, ONE, big, 0, None) == -2 and b"2^31" in err()
    assert spmm(None, 64, None, 64, None, 0, None, 0, None, 0, 0, 4, 8, None, None, 0, 0, None) == 0 and lib.mbnb_sparse_last_kernel() == b"spmm_coo8"
    with pytest.raises(RuntimeError, match="status -1"):
        _sparse_native.check(-1, "unit")


def test_workspace_queries_are_host_arithmetic():
    lib = _sparse_native.lib()
    q_quant, q_mm, q_spmm = lib.mbnb_colrow_quantize_workspace_bytes, lib.mbnb_colrow_matmul_workspace_bytes, lib.mbnb_spmm_coo_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256     # noqa: E731
    # row partials [R, chunks of 2048 columns] + column partials [blocks of 16 rows, C], f32 each
    assert q_quant(4096, 4096) == 4096 * 2 * 4 + 256 * 4096 * 4
    assert q_quant(4096, 11008) == 4096 * 6 * 4 + 256 * 11008 * 4
    assert q_quant(33, 100) == r256(33 * 4) + r256(3 * 100 * 4)
    assert q_quant(0, 8) == 0 and q_quant(-1, 8) == 0
    # matmul_colrow: Wd [N, K] of 16 bits (+ the GEMM's split-K partials) on the dense route, else nothing -- SwitchBack's rule
    tq = _train_native.lib().mbnb_switchback_forward_workspace_bytes
    for shape in [(4096, 4096, 4096, 1), (4096, 11008, 4096, 0), (300, 5003, 192, 0), (16, 4096, 4096, 1), (1, 16384, 8192, 1), (1, 4096, 4096, 1),
                  (8, 4096, 4096, 1), (64, 1024, 1024, 0), (4096, 4096, 4000, 1), (4096, 4096, 4096, 2), (4096, 4096, 4096, 9), (-1, 8, 8, 0)]:
        assert q_mm(*shape) == tq(*shape), shape
    assert q_mm(4096, 4096, 4096, 1) == 4096 * 4096 * 2 and q_mm(4096, 4096, 4096, 2) == 0
    # spmm: flag + row_ptr [rows + 1] + cursor [rows] + perm [nnz], int32 each
    assert q_spmm(100000, 1000) == 256 + r256(1001 * 4) + r256(1000 * 4) + r256(100000 * 4)
    assert q_spmm(0, 0) == 256 + 256 and q_spmm(1 << 31, 4) == 0 and q_spmm(-1, 4) == 0
    assert lib.mbnb_coo_quantize_workspace_bytes() == 4096


# ----------------------------------------------------------------------------- kernel names
def _name_table():
    src = open(SRC).read()
    m = re.search(r"kSparseKernelNames\[\]\s*=\s*\{(.*?)\};", src, flags=re.S)
    assert m, "sparse_kernels.hip: the kSparseKernelNames table is gone"
    return re.findall(r'"([^"]*)"', m.group(1))


def test_every_reported_kernel_name_is_the_kernel_of_a_case():
    names = _name_table()
    assert len(names) == 13 and len(set(names)) == 13
    src = open(SRC).read()
    assert "set_kernel_name" not in src, "libmbnb_sparse.so reports through its own table, not libmbnb_hip's record"
    assert not re.search(r"g_kernel\s*=\s*\"[^\"]", src)       # every name reaches g_kernel through the table
    expected = {c["kernel"] for c in int8_decomp_cases.CASES}
    assert set(names) == expected, (sorted(set(names) - expected), sorted(expected - set(names)))


# ----------------------------------------------------------------------------- forms behind the names: variants, limits, alignment, dtypes
_code = forms.code


def reported_variants(src):
    """Regexes of the variant strings the source can report: every set_variant("...") call, %d / %lld as a number."""
    fmts = re.findall(r'\bset_variant\("([^"]*)"', _code(src))
    return {"".join(r"\d+" if part in ("%d", "%lld") else re.escape(part) for part in re.split(r"(%lld|%d)", f)) for f in fmts}


def uncovered_variants(src, cases):
    """(patterns no case takes, variants of cases that no pattern gives)."""
    pats, have = reported_variants(src), {c["variant"] for c in cases}
    return (sorted(p for p in pats if not any(re.fullmatch(p, v) for v in have)),
            sorted(v for v in have if v and not any(re.fullmatch(p, v) for p in pats)))


MARKER = "enum { KN_CR_Q8"       # the host side of sparse_kernels.hip begins here (tests/forms.py)


def limit_counts(src):
    return forms.limit_counts(src, MARKER)


def alignment_tests(src):
    return forms.alignment_tests(src, MARKER)


def test_every_variant_the_source_reports_has_a_case_and_no_case_names_another():
    src = open(SRC).read()
    assert reported_variants(src) == {"wt", r"parts\d+", r"G\d+\ x\d+"}
    assert uncovered_variants(src, int8_decomp_cases.CASES) == ([], [])
    # every launching entry point empties the variant first
    entries = re.findall(r"^int (mbnb_\w+)\([^{]*\{\n(.*)\n", src, flags=re.M)
    assert len(entries) == 7 and all(first.strip() == "begin_call();" for _, first in entries), entries


def test_every_case_takes_the_name_and_the_variant_the_launchers_conditions_give():
    for c in int8_decomp_cases.CASES:
        assert int8_decomp_cases.model(c) == (c["kernel"], c["variant"]), (int8_decomp_cases.case_id(c), int8_decomp_cases.model(c))


def test_every_threshold_has_a_case_on_each_side():
    rows = [t[0] for t in int8_decomp_cases.THRESHOLDS]
    assert len(rows) == len(set(rows))
    for what, ops, first, second in int8_decomp_cases.THRESHOLDS:
        cs = [(c, int8_decomp_cases.derived(c)) for c in int8_decomp_cases.CASES if c["op"] in ops]
        assert any(first(c, d) for c, d in cs), f"{what}: no case on the first side"
        assert any(second(c, d) for c, d in cs), f"{what}: no case on the second side"


def unclaimed_limits(src):
    """Literals and tile constants of the source that LIMIT_COUNTS / LIMIT_CLAIMS do not know (or know with another count)."""
    m = int8_decomp_cases
    counts = limit_counts(src)
    consts = set(re.findall(r"constexpr int (\w+) = \d+;", _code(src)))
    return sorted(k for k in set(counts) | set(m.LIMIT_COUNTS) if counts.get(k) != m.LIMIT_COUNTS.get(k)) + sorted(consts ^ set(m.TILE_CONSTANTS))


def test_every_limit_of_the_launchers_is_claimed_by_a_threshold_or_listed_as_having_no_case():
    m = int8_decomp_cases
    assert unclaimed_limits(open(SRC).read()) == []
    rows = {t[0] for t in m.THRESHOLDS} | {m._CSR}
    assert set(m.LIMIT_CLAIMS) == set(m.LIMIT_COUNTS) | set(m.TILE_CONSTANTS)
    for lit, claim in m.LIMIT_CLAIMS.items():
        if isinstance(claim, tuple):
            assert claim[0] == "no case" and claim[1], lit
        else:
            assert set([claim] if isinstance(claim, str) else claim) <= rows, lit
    for lit in ("1 << 31", "1 << 40", "kMaxGrid", "kMaxElems"):
        assert m.LIMIT_CLAIMS[lit][0] == "no case"
    assert set(m.CSR_ROW_LENGTHS) >= {0, 1, 2, 3, 5, m.COO_SORT_LDS - 1, m.COO_SORT_LDS, m.COO_SORT_LDS + 1} and \
        [-(-r // m.SCAN_THREADS) for r in m.CSR_ROW_COUNTS] == [1, 2, 5]


def _pair(op, operand):
    return forms.pair(int8_decomp_cases.CASES, op, operand)


def test_every_pointer_a_launcher_tests_has_a_pair_of_cases_that_differ_by_its_offset_alone():
    m = int8_decomp_cases
    assert alignment_tests(open(SRC).read()) == set(m.OPERAND_ALIGNMENT_TESTED) | m.ALIGNMENT_REQUIRED
    for key, (op, operand) in m.OPERAND_ALIGNMENT_TESTED.items():
        pairs = _pair(op, operand)
        assert pairs and all((c["kernel"], c["variant"]) != (b["kernel"], b["variant"]) for c, b in pairs), key
    for op, operand in m.OPERAND_ALIGNMENT_FREE:
        pairs = _pair(op, operand)
        assert pairs and all((c["kernel"], c["variant"]) == (b["kernel"], b["variant"]) for c, b in pairs), (op, operand)


def test_every_form_has_a_case_for_each_dtype_it_is_instantiated_for():
    m = int8_decomp_cases
    for (name, variant), dts in m.INSTANTIATED.items():
        if name.startswith("spmm int8"):
            have = {c["dt"] for c in m.CASES if c["op"] == "spmm" and c["values"] == name.split()[1]}
        else:
            have = {c["dt"] for c in m.CASES if c["kernel"] == name and (variant is None or c["variant"] == variant or c["variant"].startswith(variant + " "))}
        assert set(dts) <= have, (name, variant, sorted(set(dts) - have))
    assert {c["kernel"] for c in m.CASES} <= {k[0] for k in m.INSTANTIATED}
    src = _code(open(SRC).read())
    assert "with_dtype" in src and not re.search(r"hipLaunchKernelGGL\(\(?k_\w+<(?:f16_t|bf16_t|float)\b", src), "every kernel template is instantiated through with_dtype: all three dtypes"


def test_the_closure_fails_on_a_variant_a_limit_or_a_pointer_test_without_a_case():
    """Three scratch edits of the source, each caught by its check."""
    m = int8_decomp_cases
    src = open(SRC).read()
    a = src.replace('set_variant("parts%d", nparts);', 'if (nparts == 3) set_variant("three");\n        else set_variant("parts%d", nparts);')
    assert a != src and uncovered_variants(a, m.CASES) == (["three"], [])
    b = src.replace("const bool vec = vec_shape && aligned(dense, 16)", "const bool vec = vec_shape && N >= 24 && aligned(dense, 16)")
    assert b != src and unclaimed_limits(b) == ["24"]
    c = src.replace("const bool vec = vec_shape && aligned(dense, 16)", "const bool vec = vec_shape && aligned(values, 16) && aligned(dense, 16)")
    assert c != src and alignment_tests(c) - set(m.OPERAND_ALIGNMENT_TESTED) - m.ALIGNMENT_REQUIRED == {("spmm_coo", "values", 16)}


def test_cases_are_well_formed():
    ids = [int8_decomp_cases.case_id(c) for c in int8_decomp_cases.CASES]
    assert len(ids) == len(set(ids))
    for c in int8_decomp_cases.CASES:
        assert c["op"] in ("quantize", "dequant", "matmul", "count", "from_dense", "quantize_coo", "spmm"), c
        assert c["dt"] in ("f16", "bf16", "f32"), c
        assert isinstance(c["variant"], str) and set(c) <= {"op", "kernel", "variant", "R", "C", "M", "N", "K", "lead", "dt", "bias", "generic", "view", "route",
                                                            "threshold", "density", "n", "rows", "cols", "index", "values", "off", "special"}, c
        for operand, off in c.get("off", {}).items():
            assert 0 < off < 16 and operand in {"quantize": "x q rs cs", "dequant": "q rm cm out", "matmul": "x w rm cm bias out ws",
                                                "spmm": "row col values dense out"}[c["op"]].split(), c
        if c["op"] == "spmm":
            assert c["index"] in ("sorted", "permuted", "int32", "duplicates") and c["values"] in ("T", "int8", "int8_entry"), c
            assert c["kernel"].endswith("_general") == bool(c.get("generic")), c


# ----------------------------------------------------------------------------- the Python functions, library stubbed
class _Stub:
    """Stands in for the loaded library: any call through it is a launch the test forbids."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the argument error must come before any call into the library")


@pytest.fixture
def stubbed(monkeypatch):
    monkeypatch.setattr(_sparse_native, "lib", lambda: _Stub())


def test_cpu_tensors_raise_the_error_of_the_other_ops(stubbed):
    z, v = torch.zeros(3, dtype=torch.long), torch.zeros(3)
    q = torch.zeros(4, 8, dtype=torch.int8)
    for call in (lambda: bnb.quantize_colrow(torch.zeros(4, 8)), lambda: bnb.dequantize_colrow(q, torch.ones(4), torch.ones(8)),
                 lambda: bnb.matmul_colrow(torch.zeros(2, 8), q, torch.ones(4), torch.ones(8)), lambda: bnb.sparse_coo_from_dense(torch.zeros(4, 8)),
                 lambda: bnb.quantize_sparse_coo(z, z, v), lambda: bnb.spmm_coo(z, z, v, torch.zeros(5, 2), 4, 5),
                 lambda: bnb.spmm_coo_int8(z, z, v.to(torch.int8), torch.ones(1), torch.zeros(5, 2), 4, 5)):
        with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
            call()


def test_argument_errors_raise_before_any_launch(stubbed, monkeypatch):
    monkeypatch.setattr(F, "_check_device", lambda *a, **k: None)      # CPU tensors stand in for device tensors: nothing may reach the library
    z, v, d = torch.zeros(3, dtype=torch.long), torch.zeros(3), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="Input must be 2D"):
        bnb.quantize_colrow(torch.zeros(8))
    with pytest.raises(ValueError, match="Input must be 2D"):
        bnb.quantize_colrow(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="row_scales has 3 elements, expected 4"):
        bnb.dequantize_colrow(torch.zeros(4, 8, dtype=torch.int8), torch.ones(3), torch.ones(8))
    with pytest.raises(ValueError, match="weight_col_scales has 4 elements, expected 8"):
        bnb.matmul_colrow(torch.zeros(2, 8), torch.zeros(4, 8, dtype=torch.int8), torch.ones(4), torch.ones(4))
    with pytest.raises(RuntimeError, match="input width"):
        bnb.matmul_colrow(torch.zeros(2, 7), torch.zeros(4, 8, dtype=torch.int8), torch.ones(4), torch.ones(8))
    with pytest.raises(TypeError, match="unsupported dtype"):
        bnb.matmul_colrow(torch.zeros(2, 8), torch.zeros(4, 8, dtype=torch.int8), torch.ones(4), torch.ones(8), dtype=torch.float64)
    with pytest.raises(ValueError):
        bnb.sparse_coo_from_dense(torch.zeros(8))
    with pytest.raises((RuntimeError, ValueError), match="nnz == 0"):
        bnb.quantize_sparse_coo(z[:0], z[:0], v[:0])
    with pytest.raises(ValueError, match="dense has 5 rows, the sparse matrix 4 columns"):
        bnb.spmm_coo(z, z, v, d, 4, 4)
    with pytest.raises(ValueError, match="differ in length"):
        bnb.spmm_coo(z[:2], z, v, d, 4, 5)
    with pytest.raises(ValueError, match="must be 1-D"):
        bnb.spmm_coo(z.view(1, 3), z, v, d, 4, 5)
    with pytest.raises(ValueError, match="dense must be 2-D"):
        bnb.spmm_coo(z, z, v, torch.zeros(5), 4, 5)
    with pytest.raises(ValueError, match="int64 or int32"):
        bnb.spmm_coo(z.to(torch.int16), z, v, d, 4, 5)
    with pytest.raises(ValueError, match="dense is torch.float16"):
        bnb.spmm_coo(z, z, v, d.half(), 4, 5)
    with pytest.raises(ValueError, match="expected 1 or 3"):
        bnb.spmm_coo_int8(z, z, v.to(torch.int8), torch.ones(2), d, 4, 5)
    with pytest.raises(ValueError, match="must be int8"):
        bnb.spmm_coo_int8(z, z, v, torch.ones(1), d, 4, 5)


# ----------------------------------------------------------------------------- the emulation against the committed goldens
def test_the_emulation_explains_the_goldens():
    """What the golden script asserted when it wrote the file, again on the committed file: statistics bit-equal, each code and Wd element
    the chain with s or with the next f32 below s; from_dense and quantize_sparse_coo bit-equal."""
    with open(os.path.join(HERE, "manifest_int8_decomp.json")) as f:
        manifest = json.load(f)["g12"]
    z = np.load(os.path.join(HERE, "g12_int8_decomp.npz"))
    kinds = {c["kind"] for c in manifest}
    assert kinds == {"colrow", "matmul_colrow", "from_dense", "quantize_sparse_coo", "spmm"}
    assert os.path.getsize(os.path.join(HERE, "g12_int8_decomp.npz")) < (1 << 20)
    low_used = 0
    for case in (c for c in manifest if c["kind"] == "colrow"):
        i, T = case["id"], DT[case["dtype"]]
        x = from_bits(z[f"cr{i}_x"], T)
        rm, cm = emul.colrow_stats(x)
        assert np.array_equal(rm.view(np.uint32), z[f"cr{i}_rm"]) and np.array_equal(cm.view(np.uint32), z[f"cr{i}_cm"]), case
        s, s_low = emul.colrow_scale(rm, cm), emul.colrow_scale(rm, cm, lower=True)
        gq = torch.from_numpy(z[f"cr{i}_q"])
        assert bool(emul.explained(gq, torch.from_numpy(emul.colrow_codes(x, s)), torch.from_numpy(emul.colrow_codes(x, s_low))).all()), case
        for t, To in DT.items():
            g = from_bits(z[f"cr{i}_wd_{t}"], To)
            exact = emul.colrow_wd(gq.numpy(), s, To)
            assert bool(emul.explained(g, exact, emul.colrow_wd(gq.numpy(), s_low, To)).all()), (case, t)
            low_used += int((emul.bits(g) != emul.bits(exact)).sum())
    assert low_used > 0, "the goldens should hold at least one element that shows torch's low sqrt"
    for case in (c for c in manifest if c["kind"] == "from_dense"):
        i, T = case["id"], DT[case["dtype"]]
        r, c, v = emul.coo_from_dense(from_bits(z[f"fd{i}_x"], T).view(case["rows"], case["cols"]), case["threshold"])
        assert np.array_equal(r.numpy(), z[f"fd{i}_row"]) and np.array_equal(c.numpy(), z[f"fd{i}_col"]), case
        assert torch.equal(emul.bits(v), emul.bits(from_bits(z[f"fd{i}_val"], T))), case
    for case in (c for c in manifest if c["kind"] == "quantize_sparse_coo"):
        i, T = case["id"], DT[case["dtype"]]
        q, scale = emul.coo_quantize(from_bits(z[f"qs{i}_v"], T))
        assert np.array_equal(q.numpy(), z[f"qs{i}_q"]) and np.array_equal(scale.numpy().view(np.uint32), z[f"qs{i}_scale"]), case
