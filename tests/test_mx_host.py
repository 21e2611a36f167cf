"""CPU-side checks of the OCP MX format and libmbnb_mx.so, without a GPU: the numpy emulation (tests/mx_emul.py) against values
written out by hand, the lossless generator and the exactness of every exact GEMM case that tests/test_gpu_mx.py runs, the forms
tables of tests/test_gpu_mx_forms.py (exactness, coverage, the planting plan, and a mutant of the GEMM per table), the C ABI
(loads, exports what include/mbnb_mx.h declares, argument errors as a status before any device access), and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _mx_native as mxn
from tests import mx_cases as cases, mx_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_mx.h")


def _block(values, fill=0.0):
    """one row of 32 f32 values: `values` first, `fill` behind them"""
    row = np.full((1, 32), fill, dtype=np.float32)
    row[0, :len(values)] = values
    return row


def _fp4_codes(codes):
    return emul.unpack(codes, "fp4")[0]


# ----------------------------------------------------------------------------- the emulation, by hand
def test_fp4_ties_go_to_the_even_code():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]                  # values 0, 1, 1, 2, 2, 4, 4
    for scale_exp in (-3, 0, 7):
        x = _block([6.0] + ties + [-t for t in ties]) * np.float32(2.0 ** scale_exp)
        codes, scales = emul.quantize(x, "fp4")
        assert scales[0, 0] == 127 + scale_exp
        c = _fp4_codes(codes)
        assert c[0] == 7
        assert list(c[1:8]) == want and list(c[8:15]) == [w | 8 for w in want]
    # just off a tie, by one ulp of f32
    near = np.array([0.25, 0.75, 2.5, 5.0], dtype=np.float32)
    up, down = np.nextafter(near, np.float32(8)), np.nextafter(near, np.float32(0))
    c = _fp4_codes(emul.quantize(_block([6.0] + list(up) + list(down)), "fp4")[0])
    assert list(c[1:9]) == [1, 2, 5, 7, 0, 1, 4, 6]


def test_fp4_saturates_everything_in_6_to_8():
    # v / 2: 3 -> 3, 3.25 -> 3, 3.5 -> 4 (the tie), 3.99.. -> 4
    for v, half_code in ((6.0, 5), (6.5, 5), (7.0, 6), (np.nextafter(np.float32(8), np.float32(0)), 6)):
        codes, scales = emul.quantize(_block([v, -v, v / 2]), "fp4")
        assert scales[0, 0] == 127 and list(_fp4_codes(codes)[:3]) == [7, 15, half_code]
        assert emul.decode_f64(codes, scales, "fp4")[0, 0] == 6.0 and emul.decode_f64(codes, scales, "fp4")[0, 1] == -6.0


def test_amax_at_and_just_below_a_power_of_two():
    below = np.nextafter(np.float32(4), np.float32(0))       # 3.99..: E = 128, byte 126 (fp4): scaled 7.99.. -> 6
    for elem, emax in (("fp4", 2), ("fp8", 8)):
        codes, scales = emul.quantize(_block([4.0, 1.0]), elem)
        assert scales[0, 0] == 129 - emax
        assert emul.decode_f64(codes, scales, elem)[0, 0] == 4.0 and emul.decode_f64(codes, scales, elem)[0, 1] == 1.0
        codes, scales = emul.quantize(_block([below, 1.0]), elem)
        assert scales[0, 0] == 128 - emax
        want = 3.0 if elem == "fp4" else 3.5                 # fp4: 7.99.. saturates at 6, times 2^-1; fp8: 511.99.. saturates at 448, times 2^-7
        assert emul.decode_f64(codes, scales, elem)[0, 0] == want


def test_zero_subnormal_and_top_exponent_blocks():
    for elem in ("fp4", "fp8"):
        z = _block([])
        z[0, 3] = -0.0
        codes, scales = emul.quantize(z, elem)
        assert scales[0, 0] == 0
        c = emul.unpack(codes, elem)[0]
        assert c[3] == (8 if elem == "fp4" else 0x80) and not c[:3].any() and not c[4:].any()      # the sign of zero is kept
        # a subnormal amax: E = 0, byte 0, every element scaled by 2^127: 2^-149 * 2^127 = 2^-22, far below half the smallest value;
        # -2^-130 * 2^127 = -2^-3: fp4 -> -0 (below the tie at .25), fp8 -> -(2^-3): exponent field 4, mantissa 0
        sub = _block([np.float32(2.0 ** -149), -np.float32(2.0 ** -130)])
        codes, scales = emul.quantize(sub, elem)
        c = emul.unpack(codes, elem)[0]
        assert scales[0, 0] == 0 and c[0] == 0
        assert c[1] == ((0x80 | (4 << 3)) if elem == "fp8" else 8)
    # E = 254: byte 252 (fp4) / 246 (fp8)
    big = np.float32(1.5 * 2.0 ** 127)
    for elem, byte in (("fp4", 252), ("fp8", 246)):
        codes, scales = emul.quantize(_block([big, -big / 2]), elem)
        assert scales[0, 0] == byte
        d = emul.decode_f64(codes, scales, elem)[0]
        assert d[0] == float(big) and d[1] == -float(big) / 2


def test_non_finite_blocks_get_the_nan_scale_and_zero_codes():
    for elem in ("fp4", "fp8"):
        for bad in (np.nan, np.inf, -np.inf):
            x = np.concatenate([_block([1.0, bad, 3.0], fill=2.0), _block([1.0, 2.0, 3.0])], axis=1)
            codes, scales = emul.quantize(x, elem)
            assert list(scales[0]) == [255, 127 + 1 - emul.EMAX[elem]]
            assert not emul.unpack(codes, elem)[0, :32].any() and emul.unpack(codes, elem)[0, 32:].any()
            d = emul.decode_f64(codes, scales, elem)[0]
            assert np.isnan(d[:32]).all() and list(d[32:35]) == [1.0, 2.0, 3.0]


def test_decode_of_all_fp4_codes_under_the_edge_scale_bytes():
    values = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    codes = np.array([[c | (c << 4) for c in range(16)]], dtype=np.uint8)     # 32 elements: every code twice
    for byte in (0, 1, 127, 254, 255):
        d = emul.decode_f64(codes, np.array([[byte]], dtype=np.uint8), "fp4")[0]
        for c in range(16):
            want = float("nan") if byte == 255 else (-1 if c & 8 else 1) * values[c & 7] * 2.0 ** (byte - 127)
            got = d[2 * c:2 * c + 2]
            assert (np.isnan(got).all() if byte == 255 else (got == want).all() and (np.signbit(got) == bool(c & 8)).all()), (c, byte)
    # e4m3: the corners of the table
    d = emul.decode_f64(np.array([[0x01, 0x08, 0x7E, 0xFE, 0x7F, 0xFF, 0x38, 0x80] * 4], dtype=np.uint8), np.array([[127]], dtype=np.uint8), "fp8")[0]
    assert list(d[:4]) == [2.0 ** -9, 2.0 ** -6, 448.0, -448.0] and np.isnan(d[4:6]).all() and d[6] == 1.0 and d[7] == 0 and np.signbit(d[7])


def test_fp8_rounds_to_nearest_even_and_saturates():
    # scaled values (anchor 448 -> byte 127): 17 -> 16 or 18? grid step at [16, 32) is 2: 17 is a tie -> even mantissa (16);
    # 19 -> 20; 464 -> 448 (saturates; 480 would be the tie to 512); 2^-10 -> 0 (tie to even), 3 * 2^-10 -> 2 * 2^-9
    x = _block([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, -17.0])
    codes, scales = emul.quantize(x, "fp8")
    d = emul.decode_f64(codes, scales, "fp8")[0]
    assert scales[0, 0] == 127 and list(d[:6]) == [448.0, 16.0, 20.0, 0.0, 2 * 2.0 ** -9, -16.0]
    for v in (449.0, 480.0, 500.0, 511.0):
        codes, scales = emul.quantize(_block([v]), "fp8")
        assert codes[0, 0] == 0x7E and scales[0, 0] == 127


# ----------------------------------------------------------------------------- the lossless generator and the exact cases
def test_lossless_rows_quantise_to_exactly_their_codes():
    x = emul.lossless(17, 1024, seed=5)
    for dtype in (torch.bfloat16, torch.float16):
        assert (cases.to_dtype(x, dtype).double().numpy() == x).all()        # exactly representable
    want_codes, want_scales = emul.lossless_codes(x)
    codes, scales = emul.quantize(x, "fp4")
    assert (codes == want_codes).all() and (scales == want_scales).all()
    assert set(np.unique(scales)) == {126, 127, 128}
    assert (emul.decode_f64(codes, scales, "fp4") == x).all()
    c8, s8 = emul.quantize(x, "fp8")
    assert (s8 == want_scales - 6).all()
    assert (emul.decode_f64(c8, s8, "fp8") == x).all()
    scaled = np.abs(np.ldexp(x.reshape(17, 32, 32), (127 - s8.astype(np.int64))[..., None]))
    assert (scaled % 32 == 0).all() and scaled.max() <= 384


@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)))
def test_every_exact_gemm_case_is_exact_in_f32(index):
    case = cases.EXACT_CASES[index]
    x, w, bias = cases.exact_operands(case, index)
    prod_unit = 2.0 ** -4
    assert ((x[:1] * w[:1]) % prod_unit == 0).all()
    total = np.abs(x) @ np.abs(w).T + (0 if bias is None else np.abs(bias)[None, :])
    assert total.max() < 2.0 ** 20, total.max()              # f32 accumulation in ANY order is exact: multiples of 2^-4 below 2^20
    assert ((x @ w.T) % prod_unit == 0).all()


def test_the_exact_cases_cover_every_listed_size():
    TM, TN, KS = cases.TM, cases.TN, cases.KS
    Ms, Ns, Ks = ({c[i] for c in cases.EXACT_CASES} for i in range(3))
    assert Ms == {1, 15, 16, 17, TM - 1, TM, TM + 1, 2 * TM + 3}
    assert Ns >= {1, 16, 17, TN - 1, TN + 1, 2 * TN + 5}
    assert Ks == {32, 96, 128, 160, KS, KS + 32, 3 * KS + 32}
    assert {c[3] for c in cases.EXACT_CASES} == {"fp4", "fp8"} and len({c[4] for c in cases.EXACT_CASES}) == 3
    assert {c[5] for c in cases.EXACT_CASES} == {True, False}


# ----------------------------------------------------------------------------- the forms tables
def _bytes_over_nonzero_codes(codes, scales, elem):
    """the scale bytes of the blocks that hold a non-zero element"""
    c = emul.unpack(codes, elem)
    live = ((c & (7 if elem == "fp4" else 0x7F)) != 0).reshape(c.shape[0], -1, 32).any(axis=2)
    return set(np.unique(scales[live]).tolist())


@pytest.mark.parametrize("index", range(len(cases.WIDE_CASES)))
def test_every_wide_case_is_lossless_and_exact_in_f32(index):
    case = cases.WIDE_CASES[index]
    M, N, K, act, x_dtype, _, _ = case
    x, w, w_codes, w_scales, a, c = cases.wide_operands(case, index)
    assert (cases.to_dtype(x, x_dtype).double().numpy() == x).all()                      # the input dtype holds x
    xc, xs = emul.quantize(x, act)
    assert (emul.decode_f64(xc, xs, act) == x).all() and (emul.decode_f64(w_codes, w_scales, "fp4") == w).all()
    _, qs = emul.quantize(np.where(np.abs(w) < 2.0 ** 127, w, 0), "fp4")                 # where w is an f32, the quantiser agrees
    small = (np.abs(w).reshape(N, -1, 32).max(axis=2) < 2.0 ** 127)
    assert (qs[small] == w_scales[small]).all()
    unit = np.ldexp(1.0, (a[:, None] + c[None, :] - 4))
    assert ((x[:, None, :5] * w[None, :, :5]) % unit[..., None] == 0).all()
    total = (np.abs(x) @ np.abs(w).T) / unit
    assert total.max() < 2.0 ** 24, total.max()                  # multiples of the unit below 2^24 of it: exact in f32 in any order
    r = x @ w.T
    assert (r % unit == 0).all() and (np.abs(r) < 2.0 ** 100).all() and (np.abs(r[r != 0]) > 2.0 ** -100).all()
    assert (emul.linear_f64(xc, xs, act, w_codes, w_scales) == r).all()
    assert (emul.gemm_as_kernel(xc, xs, act, w_codes, w_scales) == r).all()


def test_the_wide_cases_reach_the_ends_of_the_scale_byte():
    w_bytes, a_bytes = set(), {"fp4": set(), "fp8": set()}
    top_code_under_254 = False
    for index, case in enumerate(cases.WIDE_CASES):
        x, w, w_codes, w_scales, _, _ = cases.wide_operands(case, index)
        w_bytes |= _bytes_over_nonzero_codes(w_codes, w_scales, "fp4")
        wc = emul.unpack(w_codes, "fp4").reshape(w.shape[0], -1, 32)
        top_code_under_254 |= bool((((wc & 7) == 7).any(axis=2) & (w_scales == 254)).any())
        xc, xs = emul.quantize(x, case[3])
        a_bytes[case[3]] |= _bytes_over_nonzero_codes(xc, xs, case[3])
        assert case[4] in (torch.float32, torch.bfloat16)
    assert w_bytes >= {0, 1, 253, 254} and top_code_under_254, sorted(w_bytes)
    assert 0 in a_bytes["fp4"] and max(a_bytes["fp4"]) == 252, sorted(a_bytes["fp4"])
    assert 0 in a_bytes["fp8"] and max(a_bytes["fp8"]) == 246, sorted(a_bytes["fp8"])
    shapes = {c[:3] for c in cases.WIDE_CASES}
    assert shapes == {(17, 19, 256), (cases.TM + 1, cases.TN + 1, 3 * cases.KS + 64)}
    for shape in shapes:
        assert {(c[3], c[5], c[6]) for c in cases.WIDE_CASES if c[:3] == shape} == \
            {(a, o, t) for a in ("fp4", "fp8") for o in (torch.float32, torch.bfloat16) for t in ("low", "high")}
        assert {c[4] for c in cases.WIDE_CASES if c[:3] == shape} == {torch.float32, torch.bfloat16}


@pytest.mark.parametrize("index", range(len(cases.RANGE_CASES)))
def test_every_range_case_leaves_the_f32_range_where_it_says(index):
    case = cases.RANGE_CASES[index]
    name, M, N, K, a3, c, x_dtype, out_dtype = case
    x, w, w_codes, w_scales = cases.range_operands(case, index)
    assert (cases.to_dtype(x, x_dtype).double().numpy() == x).all()
    for act in ("fp4", "fp8"):
        xc, xs = emul.quantize(x, act)
        assert (emul.decode_f64(xc, xs, act) == x).all()
    assert (emul.decode_f64(w_codes, w_scales, "fp4") == w).all()
    r = x @ w.T
    assert ((r >= 0) == (np.arange(M) % 2 == 0)[:, None]).all() and (r != 0).all()      # one sign per row: partial sums are monotone
    a = np.array([a3[i % 3] for i in range(M)])
    unit = np.ldexp(1.0, a + c - 4)[:, None]
    assert (r % unit == 0).all() and (np.abs(r) / unit).max() < 2.0 ** 24
    top = np.abs(x).max(axis=1)[:, None] * np.abs(w).max(axis=1)[None, :]
    if name == "overflow":
        big = (a + c == 120)
        assert big.any() and (~big).any() and top.max() < 2.0 ** 128                     # no single product overflows
        assert (np.abs(r[big]) >= 2.0 ** 128).all() and (np.abs(r[~big]) < 2.0 ** 100).all()
        want = cases.expected_range_output(r, out_dtype)
        assert bool(torch.isinf(want[torch.from_numpy(big)]).all()) and bool(torch.isfinite(want[torch.from_numpy(~big)]).all())
        assert bool((want[0] == float("inf")).all()) == bool(big[0]) and (not big[1] or bool((want[1] == float("-inf")).all()))
    elif name == "f16-overflow":
        assert out_dtype == torch.float16 and (np.abs(r) < 2.0 ** 100).all()
        want = cases.expected_range_output(r, out_dtype)
        assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any()) and not bool(torch.isnan(want).any())
    else:
        assert name == "subnormal" and out_dtype == torch.float32
        assert (np.abs(r) < 2.0 ** -126).all() and (r % 2.0 ** -149 == 0).all() and top.max() < 2.0 ** -126
        want = cases.expected_range_output(r, out_dtype)
        if cases.SUBNORMAL_RESULTS_KEPT:
            assert (want.double().numpy() == r).all()
        else:
            assert bool((want == 0).all()) and (np.signbit(want.numpy()) == (r < 0)).all()


@pytest.mark.parametrize("index", range(len(cases.FP8_CODE_CASES)))
def test_fp8_code_cases_place_every_code_at_every_k_of_the_step(index):
    case = cases.FP8_CODE_CASES[index]
    M, N, K = case
    x, codes, w_codes, w_scales = cases.fp8_code_operands(case)
    assert x.dtype == np.float32 and K <= 512
    xc, xs = emul.quantize(x, "fp8")
    assert (xs == 127).all() and (xc == codes).all()                                      # x quantises to exactly the table's codes
    places = cases.fp8_anchor_places(M, K)
    k = np.arange(K)
    anchor = (k[None, :] % 32) == np.repeat(places, 32, axis=1)
    assert (codes[anchor] == 0x7E).all() and (anchor.reshape(M, -1, 32).sum(axis=2) == 1).all()
    # coverage: every finite code at every k mod 128 = (low / high half, g, byte of the lane's 16), outside the anchors
    seen = np.zeros((256, 128), dtype=bool)
    free = ~anchor
    seen[codes[free], np.broadcast_to(k % 128, codes.shape)[free]] = True
    classes = {(p // 64, (p % 64) // 16, p % 16) for p in range(128)}
    assert len(classes) == 2 * 4 * 16
    assert seen[list(cases.E4M3_FINITE)].all() and not seen[[0x7F, 0xFF]].any()
    assert len(cases.E4M3_FINITE) == 254 and {0x00, 0x80, 0x01, 0x81, 0x07, 0x7E, 0xFE} <= set(cases.E4M3_FINITE)
    # every element of x meets exactly one non-zero weight, which is +-1 under byte 127
    wd = emul.decode_f64(w_codes, w_scales, "fp4")
    assert set(np.unique(wd)) == {-1.0, 0.0, 1.0} and ((wd != 0).sum(axis=0) == 1).all()
    xd = x.astype(np.float64)
    assert ((xd * 512) % 1 == 0).all() and (np.abs(xd) @ np.abs(wd).T).max() < 2.0 ** 15  # multiples of 2^-9 below 2^15: exact in any order
    assert (emul.gemm_as_kernel(xc, xs, "fp8", w_codes, w_scales) == xd @ wd.T).all()


def test_the_nan_plan_meets_every_place_with_every_k_block():
    assert cases.NAN_M == cases.TM + 17 and cases.NAN_N == cases.TN + 17 and cases.NAN_K == 3 * cases.KS + 64 and cases.NAN_BLOCKS == 14
    assert cases.NAN_PLACES == (0, 5, 15, 16, 47, 64, 100, 127, 128, cases.NAN_M - 1) and len(cases.NAN_PLAN) == 14
    pairs, values = set(), set()
    for run in cases.NAN_PLAN:
        assert [p for p, _, _, _ in run] == list(cases.NAN_PLACES)
        assert len({b for _, b, _, _ in run}) == len(run)                                 # each place in a different k block
        for p, b, e, v in run:
            assert 0 <= b < 14 and 0 <= e < 32
            pairs.add((p, b))
            values.add((b, repr(v)))
    assert pairs == {(p, b) for p in cases.NAN_PLACES for b in range(14)}
    assert values == {(b, repr(v)) for b in range(14) for v in cases.NAN_VALUES}          # every block, the ragged two included, sees all three
    # the places: every fragment i, every g, both wm waves, the second tile
    frag = {(p // cases.TM, (p % cases.TM) // 64, (p % 64) // 16, (p % 16) // 4) for p in cases.NAN_PLACES}
    assert {f[0] for f in frag} == {0, 1} and {f[1] for f in frag} == {0, 1} and {f[2] for f in frag} == {0, 1, 2, 3} and {f[3] for f in frag} == {0, 1, 3}
    x, w = cases.nan_operands()
    assert (np.abs(x) @ np.abs(w).T).max() < 2.0 ** 20


@pytest.mark.parametrize("index", range(len(cases.K64_CASES)))
def test_every_k64_case_is_exact_in_f32(index):
    case = cases.K64_CASES[index]
    x, w = cases.k64_operands(case, index)
    assert case[2] % cases.KS == 64
    assert ((x @ w.T) % 2.0 ** -4 == 0).all() and (np.abs(x) @ np.abs(w).T).max() < 2.0 ** 20


def test_the_k64_and_cross_tables_are_complete():
    assert {c[2] for c in cases.K64_CASES} == {64, 192}
    assert {(c[0], c[1]) for c in cases.K64_CASES if c[2] == 192 and c[3] == "fp8"} == {(m, n) for m in (1, 17, cases.TM + 1) for n in (1, 17, cases.TM + 1)}
    assert len(set(cases.K64_CASES)) == len(cases.K64_CASES) == 2 * 2 * 9
    dts = (torch.float32, torch.bfloat16, torch.float16)
    assert set(cases.CROSS_CASES) == {(x, b, o, a) for x in dts for b in (None,) + dts for o in dts for a in ("fp4", "fp8")}
    assert len(cases.CROSS_CASES) == 72 and cases.CROSS_SHAPE == (17, 19, 160)
    x, w, bias = cases.cross_operands()
    for dt in dts:
        assert (cases.to_dtype(x, dt).double().numpy() == x).all() and (cases.to_dtype(bias, dt).double().numpy() == bias).all()
    assert ((x @ w.T + bias) % 2.0 ** -4 == 0).all() and (np.abs(x) @ np.abs(w).T + np.abs(bias)).max() < 2.0 ** 20
    assert {c[:2] for c in cases.RANDOM_CASES} >= {(x, x) for x in dts} and {c[3] for c in cases.RANDOM_CASES} == {"normal", "heavy"}
    assert {g * k // 8 % 256 == 0 for g, k in cases.ABI_SHAPES} == {True, False}


# each mutant of the GEMM fails one of the new tables; the NaN-mask and subnormal mutants pass every old exact case
def _mutant_differs(mutate, x_codes, x_scales, act, w_codes, w_scales):
    good = emul.linear_f64(x_codes, x_scales, act, w_codes, w_scales)
    bad = emul.gemm_as_kernel(x_codes, x_scales, act, w_codes, w_scales, mutate=mutate)
    return not np.array_equal(good, bad, equal_nan=True)


def _old_exact_cases_differ(mutate):
    out = []
    for index, case in enumerate(cases.EXACT_CASES):
        x, w, _ = cases.exact_operands(case, index)
        out.append(_mutant_differs(mutate, *emul.quantize(x, case[3]), case[3], *emul.quantize(w, "fp4")))
    return out


def test_the_unmutated_walk_is_the_plain_product_on_the_old_cases():
    assert not any(_old_exact_cases_differ(None))


def test_mutant_fp8_lane_map_fails_the_code_and_wide_cases():
    x, _, w_codes, w_scales = cases.fp8_code_operands(cases.FP8_CODE_CASES[0])
    assert _mutant_differs("fp8_lane_map", *emul.quantize(x, "fp8"), "fp8", w_codes, w_scales)
    x, _, w_codes, w_scales, _, _ = cases.wide_operands(cases.WIDE_CASES[0], 0)
    assert cases.WIDE_CASES[0][3] == "fp8" and _mutant_differs("fp8_lane_map", *emul.quantize(x, "fp8"), "fp8", w_codes, w_scales)


def test_mutant_subnormal_bit_fails_the_code_cases_and_passes_the_old_ones():
    for case in cases.FP8_CODE_CASES:
        x, _, w_codes, w_scales = cases.fp8_code_operands(case)
        assert _mutant_differs("subnormal_bit", *emul.quantize(x, "fp8"), "fp8", w_codes, w_scales)
    assert not any(_old_exact_cases_differ("subnormal_bit"))


def test_mutant_nan_mask_fails_the_plan_and_passes_the_old_cases():
    x, w = cases.nan_operands()
    w_codes, w_scales = emul.quantize(w, "fp4")
    for act in ("fp4", "fp8"):
        xb = x.copy()
        for p, b, e, v in cases.NAN_PLAN[0]:
            xb[p, 32 * b + e] = v
        assert _mutant_differs("nan_mask_fr", *emul.quantize(xb, act), act, w_codes, w_scales)
    assert not any(_old_exact_cases_differ("nan_mask_fr"))


def test_mutant_tail_half_fails_every_k64_case():
    for index, case in enumerate(cases.K64_CASES):
        x, w = cases.k64_operands(case, index)
        assert _mutant_differs("tail_half", *emul.quantize(x, case[3]), case[3], *emul.quantize(w, "fp4")), case


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_library_loads_and_exports_what_the_header_declares():
    lib = mxn.lib()
    assert lib.mbnb_mx_abi_version() == mxn.ABI_VERSION
    header = open(HEADER).read()
    assert int(re.search(r"#define MBNB_MX_ABI_VERSION (\d+)", header).group(1)) == mxn.ABI_VERSION
    declared = set(re.findall(r"\b(mbnb_mx_\w+)\s*\(", header))
    assert declared == set(mxn.EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name)
    for macro, value in (("TILE_M", mxn.TM), ("TILE_N", mxn.TN), ("K_STEP", mxn.KS)):
        assert int(re.search(rf"#define MBNB_MX_{macro} (\d+)", header).group(1)) == value
    makefile = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*mx$", makefile, flags=re.M) and re.search(r"^mx_SRCS\s*:=\s*mx_kernels\.hip$", makefile, flags=re.M)
    assert lib.mbnb_mx_last_launch() == b"" or b"mx_" in lib.mbnb_mx_last_launch()


def test_workspace_bytes():
    lib = mxn.lib()
    r256 = lambda b: (b + 255) // 256 * 256
    for M, K in ((1, 32), (17, 160), (33, 1024), (4096, 4096)):
        assert lib.mbnb_mx_workspace_bytes(M, K, mxn.FP4) == r256(M * K // 2) + r256(M * K // 32)
        assert lib.mbnb_mx_workspace_bytes(M, K, mxn.FP8) == r256(M * K) + r256(M * K // 32)
    assert lib.mbnb_mx_workspace_bytes(1, 32, mxn.FP4) == 512 and lib.mbnb_mx_workspace_bytes(0, 32, mxn.FP8) == 0
    assert lib.mbnb_mx_workspace_bytes(4, 48, mxn.FP4) == mxn.ERR_SHAPE and b"32" in lib.mbnb_mx_last_error()
    assert lib.mbnb_mx_workspace_bytes(4, 64, 2) == mxn.ERR_ARG and b"format" in lib.mbnb_mx_last_error()
    with pytest.raises(RuntimeError, match="status -2"):
        mxn.workspace_bytes(4, 48, mxn.FP4)


def test_argument_errors_are_a_status_before_any_device_access():
    lib = mxn.lib()
    err = lambda: lib.mbnb_mx_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first
    # quantize
    assert lib.mbnb_mx_quantize(P, 4, 64, 3, mxn.FP4, P, P, None) == mxn.ERR_ARG and b"dtype" in err()
    assert lib.mbnb_mx_quantize(P, 4, 64, 0, 2, P, P, None) == mxn.ERR_ARG and b"format" in err()
    assert lib.mbnb_mx_quantize(P, 4, 48, 0, mxn.FP4, P, P, None) == mxn.ERR_SHAPE and b"multiple" in err()
    assert lib.mbnb_mx_quantize(P, -1, 64, 0, mxn.FP4, P, P, None) == mxn.ERR_SHAPE
    assert lib.mbnb_mx_quantize(P, 4, 0, 0, mxn.FP4, P, P, None) == mxn.ERR_SHAPE
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.mbnb_mx_quantize(args[0], 4, 64, 0, mxn.FP8, args[1], args[2], None) == mxn.ERR_ARG and b"NULL" in err()
    assert lib.mbnb_mx_quantize(P + 8, 4, 64, 0, mxn.FP4, P, P, None) == mxn.ERR_ARG and b"misaligned" in err()
    assert lib.mbnb_mx_quantize(P, 4, 64, 0, mxn.FP4, P + 4, P, None) == mxn.ERR_ARG and b"misaligned" in err()
    assert lib.mbnb_mx_quantize(None, 0, 64, 0, mxn.FP4, None, None, None) == 0         # empty work: a no-op success
    # dequantize
    assert lib.mbnb_mx_dequantize(P, P, 4, 64, 5, 0, P, None) == mxn.ERR_ARG and b"format" in err()
    assert lib.mbnb_mx_dequantize(P, P, 4, 64, mxn.FP4, -1, P, None) == mxn.ERR_ARG and b"dtype" in err()
    assert lib.mbnb_mx_dequantize(P, P, 4, 33, mxn.FP4, 0, P, None) == mxn.ERR_SHAPE
    assert lib.mbnb_mx_dequantize(P, None, 4, 64, mxn.FP4, 0, P, None) == mxn.ERR_ARG and b"NULL" in err()
    assert lib.mbnb_mx_dequantize(P, P, 4, 64, mxn.FP4, 0, P + 2, None) == mxn.ERR_ARG and b"misaligned" in err()
    assert lib.mbnb_mx_dequantize(None, None, 0, 64, mxn.FP4, 0, None, None) == 0
    # linear
    ws = lib.mbnb_mx_workspace_bytes(4, 64, mxn.FP8)

    def linear(x=P, M=4, K=64, xd=1, w=P, s=P, N=8, act=mxn.FP8, bias=None, bd=0, out=P, od=1, wsp=P, wsb=ws):
        return lib.mbnb_mx_linear(x, M, K, xd, w, s, N, act, bias, bd, out, od, wsp, wsb, None)

    assert linear(xd=7) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(od=3) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(bias=P, bd=9) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(act=3) == mxn.ERR_ARG and b"format" in err()
    assert linear(K=80) == mxn.ERR_SHAPE and b"multiple" in err()
    assert linear(N=0) == mxn.ERR_SHAPE
    for name in ("x", "w", "s", "out"):
        assert linear(**{name: None}) == mxn.ERR_ARG and b"NULL" in err(), name
    assert linear(x=P + 8) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(w=P + 2) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(out=P + 1) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(bias=P + 2, bd=2) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(wsb=ws - 1) == mxn.ERR_WORKSPACE and b"workspace" in err()
    assert linear(wsp=None) == mxn.ERR_WORKSPACE
    assert linear(wsp=P + 8) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(M=0, x=None, out=None, wsp=None, wsb=0) == 0
    with pytest.raises(RuntimeError, match="status -1"):
        mxn.check(-1, "unit")


def test_the_new_sources_report_through_last_launch_only():
    src = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "mx_kernels.hip")).read()
    assert '#include "host.h"' in src and '#include "common.h"' not in src
    assert "last_launch()" in src


# ----------------------------------------------------------------------------- the Python surface
def test_names_are_exported():
    for name in ("quantize_mx", "dequantize_mx", "quantize_mxfp4", "dequantize_mxfp4", "matmul_mxfp4", "LinearMXFP4"):
        assert name in bnb.__all__ and hasattr(bnb, name), name
    assert "LinearMXFP4" in bnb.nn.__all__ and bnb.nn.LinearMXFP4 is bnb.LinearMXFP4
    assert len(bnb.__all__) == len(set(bnb.__all__))


def test_signatures():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.quantize_mx) == [("tensor", E), ("elem", "fp4")]
    assert params(bnb.dequantize_mx) == [("codes", E), ("scales", E), ("elem", "fp4"), ("dtype", torch.bfloat16)]
    assert params(bnb.quantize_mxfp4) == [("tensor", E)]
    assert params(bnb.dequantize_mxfp4) == [("codes", E), ("scales", E), ("dtype", torch.bfloat16)]
    assert params(bnb.matmul_mxfp4) == [("input", E), ("weight", E), ("weight_scales", E), ("bias", None), ("act_format", "fp8"), ("dtype", None)]
    assert params(bnb.LinearMXFP4.__init__)[:5] == [("self", E), ("in_features", E), ("out_features", E), ("bias", True), ("act_format", "fp8")]


def test_value_errors_on_cpu_tensors_widths_and_formats():
    x = torch.zeros(4, 64)
    codes, scales = torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8)
    for call in (lambda: bnb.quantize_mx(x), lambda: bnb.quantize_mxfp4(x), lambda: bnb.quantize_mx(x, "fp8"),
                 lambda: bnb.dequantize_mx(codes, scales), lambda: bnb.dequantize_mxfp4(codes, scales),
                 lambda: bnb.matmul_mxfp4(x, codes, scales), lambda: bnb.matmul_mxfp4(x, codes, scales, act_format="fp4")):
        with pytest.raises(ValueError, match="cuda"):
            call()
    for call in (lambda: bnb.quantize_mx(x, "fp6"), lambda: bnb.dequantize_mx(codes, scales, "int4"),
                 lambda: bnb.matmul_mxfp4(x, codes, scales, act_format="bf16")):
        with pytest.raises(ValueError, match="format"):
            call()
    with pytest.raises(ValueError, match="32"):
        bnb.LinearMXFP4(48, 8)
    with pytest.raises(ValueError, match="format"):
        bnb.LinearMXFP4(64, 8, act_format="fp6")
    with pytest.raises(ValueError):
        bnb.quantize_mx(torch.zeros(4, 48))


def test_linear_mxfp4_buffers_state_dict_and_grad_refusal():
    layer = bnb.LinearMXFP4(64, 8)
    sd = layer.state_dict()
    assert set(sd) == {"weight", "weight_scales", "bias"}
    assert sd["weight"].dtype == torch.uint8 and tuple(sd["weight"].shape) == (8, 32)
    assert sd["weight_scales"].dtype == torch.uint8 and tuple(sd["weight_scales"].shape) == (8, 2)
    assert isinstance(layer.bias, torch.nn.Parameter) and tuple(layer.bias.shape) == (8,)
    assert set(bnb.LinearMXFP4(64, 8, bias=False).state_dict()) == {"weight", "weight_scales"}
    other = bnb.LinearMXFP4(64, 8, act_format="fp4")
    sd["weight"] = torch.arange(8 * 32, dtype=torch.uint8).reshape(8, 32)
    other.load_state_dict(sd)
    assert torch.equal(other.weight, sd["weight"]) and other.act_format == "fp4"
    assert "mxfp4" in repr(layer)
    x = torch.zeros(2, 64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer(x)
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.matmul_mxfp4(torch.zeros(2, 64), layer.weight, layer.weight_scales, layer.bias)     # the bias Parameter requires grad
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        layer(x)
