"""
Host-side checks of the element-wise machinery, without a GPU: the checker of tests/elementwise.py has teeth (on CPU tensors),
and the table of tests/kernel_cases.py names every kernel the library can report.
"""
import glob
import os
import re

import pytest
import torch

from tests import kernel_cases, quant_cases
from tests.elementwise import assert_linear_elementwise, expected_nonfinite
from tests.goldenio import rel_fro

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mps_bitsandbytes_amd", "csrc")


def _operands(dt, M=48, N=40, K=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g).to(dt)
    Wd = (0.05 * torch.randn(N, K, generator=g)).to(dt)
    b = torch.randn(N, generator=g).to(dt)
    return X, Wd, b


def _exact(X, Wd, b):
    return X.double() @ Wd.double().t() + b.double()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_checker_passes_correctly_rounded_and_f32_accumulated_results(dt):
    X, Wd, b = _operands(dt)
    assert assert_linear_elementwise(_exact(X, Wd, b).to(dt), X, Wd, b, dt, dt, "cpu") <= 1.0
    y32 = (X.float() @ Wd.float().t() + b.float()).to(dt)            # f32 accumulation in torch's order, one rounding
    assert assert_linear_elementwise(y32, X, Wd, b, dt, dt, "cpu") <= 1.0
    assert assert_linear_elementwise(y32.float(), X, Wd, b, dt, torch.float32, "cpu") <= 1.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_checker_fails_one_element_off_by_one_percent(dt):
    X, Wd, b = _operands(dt)
    r = _exact(X, Wd, b)
    y = r.to(dt)
    i, n = 17, 23
    y[i, n] = (r[i, n] + 0.01 * r[i, n].abs()).to(dt)
    assert y[i, n] != r[i, n].to(dt)
    with pytest.raises(AssertionError, match=r"1 of 1920 elements out of bounds; worst at \(row 17, col 23\)"):
        assert_linear_elementwise(y, X, Wd, b, dt, dt, "cpu")


def test_checker_fails_one_nan():
    dt = torch.bfloat16
    X, Wd, b = _operands(dt)
    y = _exact(X, Wd, b).to(dt)
    y[5, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \(row 5, col 3\).*tile \(row, col\) at 256: \(0, 0\)"):
        assert_linear_elementwise(y, X, Wd, b, dt, dt, "cpu")


def test_checker_fails_an_error_in_a_small_row_that_rel_fro_passes():
    dt = torch.bfloat16
    X, Wd, b = _operands(dt)
    b = torch.zeros_like(b)
    X[9] *= 2.0 ** -10
    r = _exact(X, Wd, b)
    y = r.to(dt)
    y[9, 4] = (r[9, 4] * 1.01).to(dt)
    assert y[9, 4] != r[9, 4].to(dt)
    assert rel_fro(y, r) <= 2e-3                  # the norm-wise gate of the bf16 parity tests passes it
    with pytest.raises(AssertionError, match=r"worst at \(row 9, col 4\)"):
        assert_linear_elementwise(y, X, Wd, b, dt, dt, "cpu")


def test_checker_fails_an_unrounded_weight():
    """A kernel that multiplied the f32 decode without rounding it to the weight dtype misses by up to u_T * S: the checker sees it."""
    dt = torch.bfloat16
    X, Wd, b = _operands(dt, K=4096)
    # each weight off by a quarter of a bf16 ulp, in the direction that adds up in row 0: what rounding would have removed
    W32 = Wd.double() * (1 + 2.0 ** -9 * torch.sign(X[0].double()[None, :] * Wd.double()))
    y = (X.double() @ W32.t() + b.double()).to(dt)
    with pytest.raises(AssertionError):
        assert_linear_elementwise(y, X, Wd, b, dt, dt, "cpu")


def test_nonfinite_values_stay_in_their_row_and_column():
    dt = torch.float16
    X, Wd, b = _operands(dt, M=8, N=6, K=64)
    X[1, 3] = float("nan")
    X[3, 5] = float("inf")
    Wd[:, 5] = 0.25                 # every product with X[3, 5] is +inf
    Wd[:, 7] = 0.5
    Wd[2, 7] = 0.0
    X[3, 7] = float("-inf")         # ... and -inf * 0 in column 2 -> NaN; -inf * 0.25 elsewhere: +inf and -inf -> NaN
    X[6, 5] = float("inf")
    Wd[4, 0] = float("nan")
    nan, pos, neg = expected_nonfinite(X, Wd, b)
    assert nan[1].all() and nan[:, 4].all() and nan[3].all()
    assert pos[6, [0, 1, 2, 3, 5]].all() and not neg.any()
    r = _exact(torch.where(torch.isfinite(X), X, 0), torch.where(torch.isfinite(Wd), Wd, 0), b)
    y = r.to(dt)
    y[nan] = float("nan")
    y[pos] = float("inf")
    assert assert_linear_elementwise(y, X, Wd, b, dt, dt, "cpu") <= 1.0
    leak = y.clone()
    leak[2, 1] = float("nan")       # a NaN out of its row
    with pytest.raises(AssertionError, match=r"worst at \(row 2, col 1\)"):
        assert_linear_elementwise(leak, X, Wd, b, dt, dt, "cpu")
    lost = y.clone()
    lost[1, 2] = 0.0                # a NaN that vanished
    with pytest.raises(AssertionError, match=r"worst at \(row 1, col 2\)"):
        assert_linear_elementwise(lost, X, Wd, b, dt, dt, "cpu")


# ----------------------------------------------------------------------------------------------- closure over the kernel names
def _reported_names(only=None):
    """(names, prefixes): every string literal passed to set_kernel_name in csrc/*.hip and *.h (`only`: in that file alone), and for a
    formatted name the text of its snprintf format before the first conversion."""
    names, prefixes = set(), set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if only is not None and os.path.basename(path) != only:
            continue
        with open(path) as f:
            src = f.read()
        for m in re.finditer(r"\bset_kernel_name\(", src):
            i, depth = m.end(), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(src[i], 0)
                i += 1
            arg = src[m.end():i - 1]
            if "const char" in arg:
                continue            # the declaration / definition
            lits = re.findall(r'"((?:[^"\\]|\\.)*)"', arg)
            if lits:
                names.update(lits)
                continue
            fmts = re.findall(r'snprintf\(\s*' + re.escape(arg.strip()) + r'\s*,[^,]*,\s*"([^"]*)"', src[:m.start()])
            assert fmts, f"{os.path.basename(path)}: set_kernel_name({arg.strip()}) passes neither a literal nor a formatted name"
            prefixes.add(fmts[-1].split("%")[0])
    return names, prefixes


def test_the_name_scan_sees_the_library():
    names, prefixes = _reported_names()
    assert {"gemv", "dequant+dense", "i8_transpose+dense", "dense 128x128", "dense 256x256_splitk", "grad_t+dense_splitk"} <= names
    assert prefixes == {"dense_nb "}


def test_every_reported_kernel_name_is_the_kernel_of_a_case():
    names, prefixes = _reported_names()
    expected = {c["kernel"] for c in kernel_cases.CASES} | {c["form"] for c in quant_cases.CASES}
    assert sorted((names | prefixes) - expected) == []
    assert sorted(expected - (names | prefixes)) == [], "a case names a kernel the library never reports"


def test_cases_are_well_formed():
    keys = {"op", "kernel", "M", "N", "K", "lead", "dt", "out", "qt", "bs", "cs", "fmt", "bias", "fused", "view", "xexp", "bad",
            "tile", "slices", "ldw", "n_out", "xfail"}
    ids = [kernel_cases.case_id(c) for c in kernel_cases.CASES]
    assert len(set(ids)) == len(ids)
    for c in kernel_cases.CASES:
        assert set(c) <= keys, set(c) - keys
        assert c.get("dt", "f16") in ("f16", "bf16", "f32") and c.get("out", "f16") in ("f16", "bf16", "f32")
        lo, hi = c.get("xexp", (0, 0))
        if c.get("dt") == "bf16" and (lo, hi) != (0, 0):
            assert c.get("out", "bf16") in ("bf16", "f32") and -40 <= lo and hi <= 40
        if c.get("dt") == "f16" and (lo, hi) != (0, 0):
            assert -8 <= lo and hi <= 4
