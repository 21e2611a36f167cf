"""
The planting plan of tests/nonfinite.py, without a GPU: the positions are the ones the kernels treat specially, every pass of every
table case keeps the promises the GPU test relies on, no (kernel name, variant) pair with a floating activation is left without a
planted case, and the operand rules of tests/elementwise.py (expected_nonfinite) give the classes of an explicit IEEE evaluation.
"""
import math

import pytest
import torch

from tests import gemm_variant_cases, kernel_cases, nonfinite
from tests.elementwise import expected_nonfinite

ALL_CASES = kernel_cases.CASES + gemm_variant_cases.CASES
PLANTED = [c for c in ALL_CASES if c["op"] in nonfinite.ACTIVATION_OPS]
INF = float("inf")


def test_positions_are_the_special_places_of_the_contraction():
    assert nonfinite.positions(1) == [0]
    assert nonfinite.positions(72) == [0, 36, 63, 64, 71]                       # mfma128 1x64x72: the tail chunk starts at 64
    assert nonfinite.positions(2080) == [0, 1040, 2047, 2048, 2079]             # k_gemv4: one 32-k chunk in the second trip
    assert nonfinite.positions(4160) == [0, 2080, 4095, 4096, 4127, 4128, 4159]
    assert nonfinite.positions(640, 256) == [0, 255, 256, 320, 511, 512, 575, 576, 607, 608, 639]
    for L in (1, 2, 31, 32, 33, 96, 127, 1088, 8128, 16448):
        P = nonfinite.positions(L)
        assert P == sorted(set(P)) and P[0] == 0 and P[-1] == L - 1 and L // 2 in P
        for g in nonfinite.WIDTHS:
            start = (L - 1) // g * g                                              # the last g-wide step holds L - 1
            assert start in P and start <= L - 1 < start + g
            assert start == 0 or start - 1 in P


def _check_passes(rows, L, slice_len):
    P = nonfinite.positions(L, slice_len)
    ps = nonfinite.passes(rows, L, slice_len)
    inf_at = {}
    for one in ps:
        planted_rows = [r for r, _, _ in one]
        assert len(planted_rows) == len(set(planted_rows)), "two plants in one row"
        assert all(0 <= r < rows and k in P for r, k, _ in one)
        nans = [p for p in one if math.isnan(p[2])]
        if rows >= 3:
            assert len(nans) == 1 and len(planted_rows) < rows, "a pass needs a NaN row and an untouched row"
            assert len(one) >= 2, "a pass without an Inf"
        elif rows == 2:
            assert len(one) == 1
        else:
            assert len(one) == 1 and not nans
        for r, k, v in one:
            if not math.isnan(v):
                assert abs(v) == INF and k not in inf_at, "a position planted twice"
                inf_at[k] = v
    assert sorted(inf_at) == P, "every position receives an Inf in some pass"
    assert [inf_at[k] for k in P] == [INF if j % 2 == 0 else -INF for j in range(len(P))], "the signs alternate along the positions"
    if rows == 2:
        nan_passes = [one[0] for one in ps if math.isnan(one[0][2])]
        assert [(r, k) for r, k, _ in nan_passes] == [(0, P[0]), (1, P[-1])]
    if rows == 1:
        assert len(ps) == len(P)
    return len(ps)


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 16, 17, 300])
@pytest.mark.parametrize("L", [1, 72, 96, 1088, 2080, 4160])
def test_passes_keep_their_promises(rows, L):
    _check_passes(rows, L, None)
    _check_passes(rows, L, 64 if L > 64 else None)


def test_every_table_case_with_a_floating_activation_is_planted_at_every_position():
    launches = 0
    for c in PLANTED:
        rows, L, sl = nonfinite.rows_of(c), nonfinite.contraction(c), nonfinite.slice_length(c)
        if "lead" in c:
            assert rows == math.prod(c["lead"])
        launches += _check_passes(rows, L, sl)
        name = c["kernel"]
        if "splitk" in name:
            assert sl is not None, kernel_cases.case_id(c)
            P = nonfinite.positions(L, sl)
            for s in range(1, (L + sl - 1) // sl):
                assert s * sl in P and s * sl - 1 in P, (kernel_cases.case_id(c), s)
        else:
            assert sl is None, kernel_cases.case_id(c)
    assert len(PLANTED) >= 250 and launches >= len(PLANTED)


def _pairs(cases):
    return {(c["kernel"], c.get("variant")) for c in cases}


def test_no_name_variant_pair_with_a_floating_activation_is_left_out():
    """Every case of both tables whose op is fed a floating activation is planted, so every (name, variant) pair of those ops is; the
    pairs left out belong to the ops named in tests/test_gpu_nonfinite.py's docstring, and to nothing else."""
    out = [c for c in ALL_CASES if c["op"] not in nonfinite.ACTIVATION_OPS]
    assert {c["op"] for c in out} == {"matmul_int8", "grad_t", "outlier_linear", "embedding_4bit", "embedding_8bit"}
    for pair in _pairs(ALL_CASES):
        ops = {c["op"] for c in ALL_CASES if (c["kernel"], c.get("variant")) == pair}
        if ops & set(nonfinite.ACTIVATION_OPS):
            assert pair in _pairs(PLANTED)
            assert any(nonfinite.case_passes(c) for c in PLANTED if (c["kernel"], c.get("variant")) == pair)
    # the weight-side plants: every 4-bit, int8 and FP8 weight case, and matmul_int8's scales
    assert {c["op"] for c in ALL_CASES if c["op"] in nonfinite.WEIGHT_OPS} == set(nonfinite.WEIGHT_OPS)


def test_expected_nonfinite_equals_an_explicit_ieee_evaluation():
    """The operand rules against (X[:, None, :] * W[None, :, :]).sum(-1) in float64, on an example that holds every rule: a NaN
    activation, Infs of either sign meeting positive, negative and exact-zero weights, two Infs of opposite effect in one dot
    product, an Inf weight, a NaN weight row, an Inf and a NaN bias, and untouched rows and columns."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 9, 8, 40
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    W[2, 7] = 0.0                    # an exact-zero weight under the +Inf of row 1
    W[5, 39] = -0.0                  # ... and a negative zero under the -Inf of row 2
    X[0, 3] = float("nan")
    X[1, 7] = INF
    X[2, 39] = -INF
    X[3, 0] = INF
    X[3, 20] = INF                   # row 3: columns where W[n, 0] and W[n, 20] differ in sign give Inf - Inf
    X[5, 11] = 0.0                   # a zero activation under the Inf weight
    W[4, 11] = INF
    W[6, 1] = float("nan")
    b[7] = -INF
    b[1] = float("nan")
    want = nonfinite.classes(nonfinite.ieee_linear(X, W, b))
    nan, pos, neg = expected_nonfinite(X, W, b)
    got = nan * 1 + pos * 2 + neg * 3
    assert torch.equal(got, want), (got, want)
    for cls in (0, 1, 2, 3):
        assert bool((want == cls).any()), f"the example holds no element of class {cls}"
    assert bool((want[8] == 0)[[0, 2, 3, 5]].all()), "an untouched row stays finite under finite weights and bias"
    # without a bias, and the transposed roles of the input gradient (dY . Wd, the contraction over N)
    want = nonfinite.classes(nonfinite.ieee_linear(X, W))
    nan, pos, neg = expected_nonfinite(X, W)
    assert torch.equal(nan * 1 + pos * 2 + neg * 3, want)
    assert bool((want[1, 2] == 1)) and bool((want[2, 5] == 1)), "Inf times an exact zero is NaN"
    assert int((want[3] == 1).sum()) > 0 and int((want[3] == 2).sum()) > 0, "row 3 holds Inf - Inf and plain +Inf columns"
