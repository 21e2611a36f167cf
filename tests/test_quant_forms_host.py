"""
Host-side checks of the quantise / dequantise form tests, without a GPU: the guard checker of tests/guard.py has teeth (on CPU
tensors), and the table of tests/quant_cases.py is closed over the names, the alignment tests and the thresholds of the launchers
in csrc/quant_kernels.hip.
"""
import os
import re

import pytest
import torch

from tests import quant_cases
from tests.guard import FILLS, GUARD, GuardedTorch, GuardViolation
from tests.quant_cases import ALIGNMENT_TESTED, CASES, INSTANTIATED, THRESHOLDS, buffers, case_id, derived, model_form
from tests.test_elementwise_host import CSRC, _reported_names


# ----------------------------------------------------------------------------------------------- the guard checker
def _alloc(fill, n=40, dtype=torch.int8, offset=0):
    g = GuardedTorch()
    g.begin(fill, [("q", offset)], "quantize_rowwise q8_row_regs")
    t = g.empty(n, dtype=dtype, device="cpu")
    return g, t, g.allocs[0]


@pytest.mark.parametrize("offset", [0, 1, 8])
def test_guarded_empty_is_filled_offset_and_banded(offset):
    g, t, a = _alloc(0x5A, 40, torch.int8, offset)
    assert t.data_ptr() % 16 == offset and t.shape == (40,) and bool((t == 0x5A).all())
    assert a.start >= GUARD and a.buf.numel() - a.start - a.nbytes >= GUARD
    t.fill_(3)
    g.check()                      # writing every element of the payload touches no band


def test_one_byte_past_the_end_is_reported_with_its_offset():
    g, t, a = _alloc(0xFF)
    a.buf[a.start + a.nbytes + 5] = 0
    with pytest.raises(GuardViolation, match=r"quantize_rowwise q8_row_regs: a write outside buffer 'q' \(40 bytes, fill 0xFF\).*5 bytes past its end \(offset \+5\)"):
        g.check()


def test_one_byte_before_the_start_is_reported_with_its_offset():
    g, t, a = _alloc(0x5A, 16, torch.float32, 4)
    a.buf[a.start - 3] = 0
    with pytest.raises(GuardViolation, match=r"buffer 'q' \(64 bytes, fill 0x5A\).*3 bytes before its start \(offset -3\)"):
        g.check()


def test_a_dword_store_over_the_end_of_a_packed_buffer_is_caught():
    """What a 4-bit quantiser without its tail guard does: a whole dword stored where two bytes remain."""
    g, t, a = _alloc(0xFF, 6, torch.uint8)
    a.buf[a.start + 4:a.start + 8] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
    with pytest.raises(GuardViolation, match=r"0 bytes past its end \(offset \+0\)"):
        g.check()


def test_a_placed_tensor_keeps_its_values_and_its_bands():
    g = GuardedTorch()
    g.begin(0x5A, (), "op form")
    x = torch.arange(24, dtype=torch.float16).view(4, 6)
    y = g.place("in", x, 2)
    assert torch.equal(x, y) and y.data_ptr() % 16 == 2 and y.is_contiguous()
    g.check()


def test_an_unwritten_element_is_caught_under_the_two_fills():
    """The oracle's code at element 7 is -1, the byte 0xFF: a kernel that skips the element passes under the 0xFF fill alone."""
    want = torch.arange(-8, 8, dtype=torch.int8)
    assert want[7] == -1
    verdicts = []
    for fill in FILLS:
        g, t, _ = _alloc(fill, 16)
        t[:7] = want[:7]
        t[8:] = want[8:]            # element 7 is never written
        g.check()
        verdicts.append(torch.equal(t, want))
    assert verdicts == [True, False]


# ----------------------------------------------------------------------------------------------- closure over the names
def _launcher_names():
    names, prefixes = _reported_names(only="quant_kernels.hip")
    assert not prefixes
    return names


def test_every_form_the_launchers_report_has_a_case_and_no_case_names_another():
    names = _launcher_names()
    assert len(names) >= 40
    forms = {c["form"] for c in CASES}
    assert sorted(names - forms) == [], "a quantisation launcher reports a form that no case of tests/quant_cases.py takes"
    assert sorted(forms - names) == [], "a case names a form the launchers never report"


def test_every_form_has_a_case_for_every_dtype_it_is_instantiated_for():
    for form in sorted({c["form"] for c in CASES}):
        have = {c["dt"] for c in CASES if c["form"] == form}
        assert set(INSTANTIATED.get(form, quant_cases.DTS)) <= have, (form, have)


def test_every_case_takes_the_form_the_launchers_conditions_give():
    for c in CASES:
        assert model_form(c) == c["form"], f"{case_id(c)}: the launcher's conditions give {model_form(c)!r}"


def test_every_alignment_tested_form_has_a_misaligned_case_for_each_buffer_it_tests():
    for form, tests in ALIGNMENT_TESTED.items():
        for buf, fallback in tests:
            hits = []
            for c in CASES:
                al = c.get("align", {})
                if c["form"] != fallback or not al.get(buf):
                    continue
                rest = {k: v for k, v in al.items() if k != buf}
                if model_form(dict(c, align=rest)) == form:      # this buffer's offset alone sends the case to the fallback
                    hits.append(c)
            assert hits, f"no case takes {fallback!r} because {buf!r} of an otherwise {form!r} call is misaligned"
    # every pointer a launcher tests is in ALIGNMENT_TESTED (or internal: rows8_wt's two, the flat form's packed): 7 through aligned16()
    # and 11 spelled out.  A test added to or removed from the launchers changes these counts
    with open(os.path.join(CSRC, "quant_kernels.hip")) as f:
        src = f.read()
    assert (len(re.findall(r"\baligned16\(", src)), len(re.findall(r"reinterpret_cast<uintptr_t>", src))) == (1 + 7, 1 + 11), \
        "an alignment test was added to or removed from the launchers: update ALIGNMENT_TESTED and its cases"


def test_misaligned_cases_use_offsets_the_buffers_can_have():
    esize = {"f16": 2, "bf16": 2, "f32": 4}
    for c in CASES:
        for buf, off in c.get("align", {}).items():
            assert 0 < off < 16, case_id(c)
            assert buf == "in" or buf in buffers(c) or (c.get("out") and buf in ("packed", "out")), (case_id(c), buf)
            if buf == "in" and c["op"].startswith("quantize") or c["op"] == "double_quant" and buf == "in":
                assert off % esize[c["dt"]] == 0, case_id(c)
            if buf in ("absmax", "absmax2", "scales", "col_stats", "row_stats"):
                assert off % 4 == 0, case_id(c)
            if buf == "out" and c["op"] != "dequant_absmax":
                assert off % esize[c["dt"]] == 0, case_id(c)


def test_every_threshold_has_a_case_on_each_side():
    for what, ops, below, above in THRESHOLDS:
        for op in ops:
            cs = [(c, derived(c)) for c in CASES if c["op"] == op]
            assert any(below(c, d) for c, d in cs), f"{what}: no {op} case on the first side"
            assert any(above(c, d) for c, d in cs), f"{what}: no {op} case on the second side"


def test_non_finite_values_are_planted_in_every_form_of_quantize_4bit():
    for stem in ("q4_tiny", "q4_wave", "q4_rows", "q4_rows2", "q4_big"):
        kinds = set()
        for c in CASES:
            if c["form"].startswith(stem) and "bad" in c and not c.get("given"):
                kinds |= {k for k, _ in c["bad"]}
        assert kinds == {"nan", "+inf", "-inf"}, (stem, kinds)
    for bs in (1, 2, 4):
        assert any(c["form"] == "q4_tiny" and c["bs"] == bs and "bad" in c for c in CASES)
    assert any(c.get("given") and "bad" in c for c in CASES)
    for c in CASES:
        if "bad" in c:
            assert c["op"] == "quantize_4bit" and not c.get("cs")
            blocks = {i // c["bs"] for _, i in c["bad"]}
            assert len(blocks) == len(c["bad"]) and all(i < derived(c)["numel"] for _, i in c["bad"]), case_id(c)


def test_cases_are_well_formed():
    keys = {"op", "form", "shape", "dt", "bs", "qt", "cs", "given", "kind", "out", "align", "bad", "large", "slabs", "xfail"}
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in CASES:
        assert set(c) <= keys, set(c) - keys
        assert c["op"] in quant_cases.BUFFERS and c["dt"] in quant_cases.DTS
        if c["op"] in ("quantize_4bit", "dequantize_4bit"):
            assert c["qt"] in ("nf4", "fp4") and c["bs"] & (c["bs"] - 1) == 0
        if c.get("slabs"):
            assert derived(c)["numel"] > 1 << 31 and "large" in c
        if derived(c)["numel"] >= 1 << 27:
            assert "large" in c, case_id(c)
