"""
Host-side closure of tests/grad_cases.py over csrc/grad_kernels.hip, without a GPU: the instantiations the source compiles (its switch
arms and template arguments) all have a case, every literal its host side compares a size with is claimed by a THRESHOLDS row with a
case on each side (or listed as having none), the pointer tests are the ones the table knows, model(case) gives every case its
(kernel, variant), every offset operand stands in a pair that differs by that offset alone, and the guard checker catches a store one
element off either end of dX.  Scratch copies of the source with an added format arm, an added limit or a removed alignment test fail.
"""
import os
import re

import pytest
import torch

from tests import forms, grad_cases
from tests.grad_cases import CASES, INSTANTIATED, LIMIT_CLAIMS, LIMIT_COUNTS, THRESHOLDS, case_id, derived, model
from tests.guard import GuardedTorch, GuardViolation
from tests.test_elementwise_host import CSRC

SRC = os.path.join(CSRC, "grad_kernels.hip")
MARKER = "static bool is4("          # the first host function: the host side of grad_kernels.hip begins here
_WORD = {"MBNB_NF4": "nf4", "MBNB_FP4": "fp4", "MBNB_W_INT8_ROWWISE": "int8", "MBNB_W_FP8_E4M3": "fp8", "MBNB_W_DENSE": "dense",
         "f16_t": "f16", "bf16_t": "bf16", "float": "f32", "true": True, "false": False}


def _src():
    with open(SRC) as f:
        return f.read()


# ----------------------------------------------------------------------------------------------- instantiations
def scan_instantiated(src):
    """The INSTANTIATED table as the source has it: the values of every template argument a launcher passes a kernel."""
    code = forms.host_part(src, MARKER)

    def words(pattern):
        found = re.findall(pattern, code)
        assert found, pattern
        return tuple(dict.fromkeys(_WORD.get(w, w) for w in found))

    return {
        "k_dequant_t": dict(T=words(r"\bdequant_t_dispatch<(\w+)>\("), FMT=words(r"\blaunch_dequant_t<T, (\w+)>\("),
                            NESTED=words(r"\(k_dequant_t<T, FMT, (\w+)>\)")),
        "k_grad_generic": dict(T=words(r"\bgeneric_out<(\w+)>\("), O=words(r"\blaunch_generic<T, (\w+)>\("),
                               FMT=words(r"\blaunch_generic_fmt<T, O, (\w+)>\("), NESTED=words(r"\(k_grad_generic<T, O, FMT, (\w+)>\)")),
    }


def _same_axes(a, b):
    return {k: {ax: set(v) for ax, v in axes.items()} for k, axes in a.items()} == {k: {ax: set(v) for ax, v in axes.items()} for k, axes in b.items()}


def test_the_table_lists_the_instantiations_of_the_source():
    got = scan_instantiated(_src())
    assert _same_axes(got, INSTANTIATED), got
    assert len(grad_cases.instantiations("k_grad_generic")) == 63 and len(grad_cases.instantiations("k_dequant_t")) == 14
    # the switch arms: one per format in each dispatcher, the dense format their default
    code = forms.host_part(_src(), MARKER)
    assert len(re.findall(r"\bcase MBNB_\w+:", code)) == 2 * 4 + 2 + 2 and len(re.findall(r"\bdefault:", code)) == 4


def test_every_instantiation_has_a_case():
    have = {grad_cases.instantiation(c) for c in CASES}
    for kernel in INSTANTIATED:
        missing = sorted(str(i) for i in grad_cases.instantiations(kernel) if (kernel, i) not in have)
        assert missing == [], f"{kernel}: no case runs {missing}"
    # both store forms of every instantiation of the pass, and every value of every axis on its own
    variants = {c["variant"] for c in CASES if c["kernel"] == "grad_t"}
    for T, _, f, n in grad_cases.instantiations("k_dequant_t"):
        for store in ("vec", "scalar"):
            assert f"grad_t {f} {T} {'nested' if n else 'plain'} {store}" in variants
    for kernel, axes in INSTANTIATED.items():
        for axis, values in axes.items():
            col = {"T": 0, "O": 1, "FMT": 2, "NESTED": 3}[axis]
            assert set(values) <= {inst[col] for k, inst in have - {None} if k == kernel}, (kernel, axis)


def test_every_autograd_pair_of_dtypes_meets_every_format_and_nested_absmax():
    for T in grad_cases.DTS:
        for O in grad_cases.DTS:
            cs = [c for c in CASES if c["kernel"] == "grad_generic" and c["dt"] == T and c.get("xdt", T) == O]
            assert {grad_cases.fmt_word(c) for c in cs} == set(grad_cases.FORMATS), (T, O)
            assert any(grad_cases.nested(c) for c in cs), (T, O)


# ----------------------------------------------------------------------------------------------- limits and pointer tests
def unclaimed_limits(src):
    counts = forms.limit_counts(src, MARKER)
    return sorted(k for k in set(counts) | set(LIMIT_COUNTS) if counts.get(k) != LIMIT_COUNTS.get(k))


def alignment_masks(src):
    """The masks of the host side's pointer tests, in source order: (p & 15) == 0 and its kin."""
    return [int(m) for m in re.findall(r"& (\d+)\) == 0", forms.host_part(src, MARKER))]


def test_every_threshold_has_a_case_on_each_side():
    rows = [t[0] for t in THRESHOLDS]
    assert len(rows) == len(set(rows))
    for what, ops, first, second in THRESHOLDS:
        cs = [(c, derived(c)) for c in CASES if c["op"] in ops]
        assert any(first(c, d) for c, d in cs), f"{what} {ops}: no case on the first side"
        assert any(second(c, d) for c, d in cs), f"{what} {ops}: no case on the second side"


def test_every_limit_of_the_host_side_is_claimed_by_a_threshold_or_listed_as_having_no_case():
    assert unclaimed_limits(_src()) == []
    rows = {t[0] for t in THRESHOLDS}
    assert set(LIMIT_CLAIMS) == set(LIMIT_COUNTS)
    claimed = set()
    for lit, claim in LIMIT_CLAIMS.items():
        for one in (claim if isinstance(claim, list) else [claim]):
            assert one in rows or (isinstance(one, tuple) and one[0] == "no case" and one[1]), (lit, one)
            claimed.add(one)
    assert rows <= claimed, sorted(rows - claimed)
    for lit in ("1 << 31", "0x7FFFFFFF"):
        assert LIMIT_CLAIMS[lit][0] == "no case"
    # the row limit of the generic kernel is gone: its launcher refuses a column count alone
    code = forms.host_part(_src(), MARKER)
    assert "MBNB_ERR_UNSUPPORTED" in code and not re.search(r"GRAD_GM\s*>\s*65535", code)


def test_the_pointer_tests_are_the_ones_the_table_knows():
    src = _src()
    assert alignment_masks(src) == grad_cases.ALIGNMENT_MASKS
    assert len(re.findall(r"reinterpret_cast<uintptr_t>", forms.host_part(src, MARKER))) == 4      # out, W, the workspace, dY
    for op, operand in grad_cases.OPERAND_ALIGNMENT_TESTED:
        pairs = forms.pair(CASES, op, operand)
        assert pairs and any((c["kernel"], c["variant"]) != (b["kernel"], b["variant"]) for c, b in pairs), (op, operand)
    for op, operand in grad_cases.OPERAND_ALIGNMENT_FREE:
        pairs = forms.pair(CASES, op, operand)
        assert pairs and all((c["kernel"], c["variant"]) == (b["kernel"], b["variant"]) for c, b in pairs), (op, operand)


def test_every_offset_operand_stands_in_a_pair_that_differs_by_that_offset_alone():
    offset = {(c["op"], k) for c in CASES for k in c.get("off", {})}
    assert offset == grad_cases.OPERAND_ALIGNMENT_TESTED | grad_cases.OPERAND_ALIGNMENT_FREE
    for op, operand in offset:
        for c, b in forms.pair(CASES, op, operand):
            assert {k: v for k, v in c.items() if k not in ("off", "kernel", "variant")} == {k: v for k, v in b.items() if k not in ("kernel", "variant")}
        assert forms.pair(CASES, op, operand), (op, operand)
    # the packed weight: legal at 4 and 12 bytes off 16, refused (generic in the full call) at 1 and 2
    by_off = {c["off"]["w"]: c["kernel"] for c, _ in forms.pair(CASES, "grad_t", "w") if c["fmt"] == "4bit"}
    assert by_off == {4: "grad_t", 12: "grad_t", 1: "unsupported", 2: "unsupported"}
    by_off = {c["off"]["w"]: c["kernel"] for c, _ in forms.pair(CASES, "grad_abi", "w") if c["fmt"] == "4bit"}
    assert by_off == {4: "grad_t+dense", 1: "grad_generic", 2: "grad_generic"}


# ----------------------------------------------------------------------------------------------- the model
def test_every_case_takes_the_name_and_the_variant_the_launchers_conditions_give():
    for c in CASES:
        assert model(c) == (c["kernel"], c["variant"]), (case_id(c), model(c))
    # the smallest shape the plan splits: nothing smaller along the contraction does
    M, N, K = (grad_cases.SPLIT[k] for k in "MNK")
    assert grad_cases.gemm_dense_plan(M, K, N)[1] > 1 and (N // 64) % -(-(N // 64) // grad_cases.gemm_dense_plan(M, K, N)[1]) != 0
    assert all(grad_cases.gemm_dense_plan(m, k, n)[1] == 1 for n in range(128, N, 64) for m in (1, 4, 64, 255, 256) for k in (8, 72, 264, 520))


def test_the_restated_workspace_query_is_the_librarys():
    from mps_bitsandbytes_amd import _native
    q = _native.lib().mbnb_linear_grad_input_workspace_bytes
    code = {"nf4": 0, "fp4": 1, "int8": _native.W_INT8_ROWWISE, "fp8": _native.W_FP8_E4M3, "dense": _native.W_DENSE}
    n = 0
    for c in CASES:
        if c["op"] != "grad_t":
            assert q(c["M"], c["N"], c["K"], code[grad_cases.fmt_word(c)], grad_cases.DTS.index(c["dt"])) == grad_cases.ws_query(c), case_id(c)
            n += 1
    assert n > 100


# ----------------------------------------------------------------------------------------------- the guard checker
@pytest.mark.parametrize("where", ["past", "before"])
def test_the_guard_checker_catches_a_store_one_element_off_dx(where):
    g = GuardedTorch()
    g.begin(0x5A, (), "grad_abi case")
    dX = g.place_empty("dx", (5, 72), torch.bfloat16, "cpu", 2)
    dX.fill_(1.0)
    g.check()
    a = g.allocs[0]
    words = a.buf.view(torch.int16)
    assert a.start % 2 == 0
    if where == "past":
        words[(a.start + a.nbytes) // 2] = 0x3F80
        match = r"buffer 'dx' \(720 bytes, fill 0x5A\).*0 bytes past its end"
    else:
        words[a.start // 2 - 1] = 0x3F80
        match = r"buffer 'dx' \(720 bytes, fill 0x5A\).*(1|2) bytes before its start"
    with pytest.raises(GuardViolation, match=match):
        g.check()


def test_a_workspace_is_carved_off_its_256_byte_alignment():
    g = GuardedTorch()
    g.begin(0xFF, (), "grad_abi case")
    ws = g.place_empty("ws", (512,), torch.uint8, "cpu", 16)
    assert (ws.data_ptr() - g.allocs[0].buf.data_ptr()) % 256 == 16
    g.check()


# ----------------------------------------------------------------------------------------------- the closure has teeth
def test_the_closure_fails_on_a_format_arm_a_limit_or_a_removed_pointer_test():
    src = _src()
    arm = "        case MBNB_W_FP8_E4M3: return launch_dequant_t<T, MBNB_W_FP8_E4M3>("
    a = src.replace(arm, "        case 7: return launch_dequant_t<T, MBNB_W_NEW>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);\n" + arm)
    assert a != src and not _same_axes(scan_instantiated(a), INSTANTIATED)
    assert "MBNB_W_NEW" in scan_instantiated(a)["k_dequant_t"]["FMT"]
    b = src.replace("if (M <= 0 || N < 128 ||", "if (M <= 0 || N < 128 || K > 24 ||")
    assert b != src and unclaimed_limits(b) == ["24"]
    c = src.replace(" && (reinterpret_cast<uintptr_t>(dY) & 15) == 0", "")
    assert c != src and alignment_masks(c) != grad_cases.ALIGNMENT_MASKS


def test_cases_are_well_formed():
    keys = {"op", "kernel", "variant", "M", "N", "K", "dt", "xdt", "fmt", "qt", "bs", "cs", "bias", "xexp", "bad", "off", "ws"}
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    esize = {"f16": 2, "bf16": 2, "f32": 4}
    for c in CASES:
        assert set(c) <= keys, (case_id(c), set(c) - keys)
        assert c["op"] in grad_cases.OPERANDS and c["dt"] in grad_cases.DTS and c.get("xdt", "f16") in grad_cases.DTS
        assert c["fmt"] in ("4bit", "int8", "fp8", "dense") and (c["fmt"] == "4bit" or not {"qt", "bs", "cs"} & set(c))
        assert ("M" in c) == (c["op"] != "grad_t") and c.get("ws") in (None, "null", "short", "nosplit")
        for operand, off in c.get("off", {}).items():
            assert operand in grad_cases.OPERANDS[c["op"]] and 0 < off <= 16, case_id(c)
            if operand in ("dy", "out"):
                assert off % esize[c["dt"]] == 0
            if operand == "dx":
                assert off % esize[c.get("xdt", c["dt"])] == 0
        if "ws" in c or "off" in c and c["op"] != "grad_t":
            assert c["op"] == "grad_abi", case_id(c)
        if c.get("bias"):
            assert c["op"] == "grad"
        if "x" in c.get("bad", ""):
            assert c["N"] > 9
        if "w" in c.get("bad", ""):
            assert not c.get("cs")
        lo, hi = c.get("xexp", (0, 0))
        assert (-8 <= lo and hi <= 4) if c["dt"] == "f16" else (-40 <= lo and hi <= 40)
        # no LLM-sized operand
        assert c["N"] * c["K"] <= 1 << 19 and c.get("M", 1) * max(c["N"], c["K"]) <= 1 << 22, case_id(c)
