"""CPU-side checks of the weight-only MXFP4 decode linear, without a GPU: the C ABI (the header, the binding and the
library agree; every argument error is a status before any device access), the Python surface (`act_format="none"`), and the case
tables of tests/mx_decode_cases.py: every exact case is exact in f32 in ANY summation order, and stays inside the normal f32 range
unless the case says otherwise."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _mx_native as mxn
from tests import mx_cases, mx_decode_cases as cases, mx_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_mx.h")
NORMAL_MIN, NORMAL_MAX = 2.0 ** -126, 2.0 ** 128


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_header_binding_and_library_agree():
    lib = mxn.lib()
    header = open(HEADER).read()
    assert mxn.ABI_VERSION == 2 and lib.mbnb_mx_abi_version() == 2
    assert int(re.search(r"#define MBNB_MX_ABI_VERSION (\d+)", header).group(1)) == 2
    declared = set(re.findall(r"\b(mbnb_mx_\w+)\s*\(", header))
    assert declared == set(mxn.EXPORTED_SYMBOLS) and "mbnb_mx_linear_weight_only" in declared
    assert getattr(lib, "mbnb_mx_linear_weight_only")
    assert int(re.search(r"#define MBNB_MX_DECODE_ROWS (\d+)", header).group(1)) == mxn.DECODE_ROWS == 16
    n_args = len(re.search(r"int mbnb_mx_linear_weight_only\(([^)]*)\)", header).group(1).split(","))
    assert n_args == len(mxn._SIGNATURES["mbnb_mx_linear_weight_only"][1]) == 12


def test_argument_errors_of_the_weight_only_linear_are_a_status_before_any_device_access():
    lib = mxn.lib()
    err = lambda: lib.mbnb_mx_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first

    def linear(x=P, M=4, K=64, xd=1, w=P, s=P, N=8, bias=None, bd=0, out=P, od=1):
        return lib.mbnb_mx_linear_weight_only(x, M, K, xd, w, s, N, bias, bd, out, od, None)

    assert linear(xd=7) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(xd=-1) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(od=3) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(bias=P, bd=9) == mxn.ERR_ARG and b"dtype" in err()
    assert linear(K=80) == mxn.ERR_SHAPE and b"multiple" in err()
    assert linear(K=0) == mxn.ERR_SHAPE and linear(M=-1) == mxn.ERR_SHAPE
    assert linear(N=0) == mxn.ERR_SHAPE and linear(N=-3) == mxn.ERR_SHAPE
    assert linear(M=2 ** 20, N=2 ** 20, K=2 ** 10) == mxn.ERR_SHAPE
    for name in ("x", "w", "s", "out"):
        assert linear(**{name: None}) == mxn.ERR_ARG and b"NULL" in err(), name
    assert linear(x=P + 8) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(w=P + 2) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(out=P + 1) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(out=P + 2, od=2) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(bias=P + 2, bd=2) == mxn.ERR_ARG and b"misaligned" in err()
    assert linear(bias=P + 1, bd=1) == mxn.ERR_ARG and b"misaligned" in err()
    # the launch grid: 2^26 f32 rows in passes of 8 times 2^12 weight rows in workgroups of 16 is 2^31 workgroups
    assert linear(M=2 ** 26, N=2 ** 12, K=32, xd=2) == mxn.ERR_SHAPE and b"workgroups" in err()
    # empty work: a no-op success, pointers unread
    assert linear(M=0, x=None, w=None, s=None, out=None) == 0
    # the quantising entry points keep refusing every other element format
    assert lib.mbnb_mx_workspace_bytes(4, 64, 2) == mxn.ERR_ARG and b"format" in err()
    assert lib.mbnb_mx_linear(P, 4, 64, 1, P, P, 8, 2, None, 0, P, 1, P, 1 << 20, None) == mxn.ERR_ARG and b"format" in err()


def test_the_source_keeps_to_host_h_and_last_launch():
    src = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "mx_kernels.hip")).read()
    assert "k_mx_decode" in src and '#include "host.h"' in src and '#include "common.h"' not in src
    assert "set_kernel_name" not in src and "set_kernel_variant" not in src and '"mx_decode %s MT%d"' in src and "k_mx_decode_mfma" in src
    makefile = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "Makefile")).read()
    assert re.search(r"^mx_SRCS\s*:=\s*mx_kernels\.hip$", makefile, flags=re.M)
    # the MFMA form's K walk and reduction are mx_decode.h's, the text the expert kernels call too: defined there once, called here once
    shared = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "mx_decode.h")).read()
    assert '#include "mx_decode.h"' in src
    for name in ("tile_walk", "tile_reduce"):
        definition = re.compile(r"^__device__ __forceinline__ [\w ]+ " + name + r"\(", flags=re.M)
        assert len(definition.findall(shared)) == 1 and not definition.search(src), name
    assert len(re.findall(r"\btile_walk<\w+>\(", src)) == 1 == len(re.findall(r"\btile_reduce\(", src))
    for inner in ("__builtin_amdgcn_permlane32_swap", "mfma16(", "decode8_16<"):
        assert inner in shared and inner not in src, inner


# ----------------------------------------------------------------------------- the Python surface
def test_signatures_are_unchanged_and_none_is_accepted():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.matmul_mxfp4) == [("input", E), ("weight", E), ("weight_scales", E), ("bias", None), ("act_format", "fp8"), ("dtype", None)]
    assert params(bnb.LinearMXFP4.__init__)[:5] == [("self", E), ("in_features", E), ("out_features", E), ("bias", True), ("act_format", "fp8")]
    assert params(bnb.LinearMXFP4.from_linear)[:2] == [("linear", E), ("act_format", "fp8")]
    assert "none" in bnb.matmul_mxfp4.__doc__ and "dequantise" in bnb.matmul_mxfp4.__doc__
    layer = bnb.LinearMXFP4(64, 8, act_format="none")
    assert layer.act_format == "none" and "act_format=none" in repr(layer) and "mxfp4" in repr(layer)
    # "none" gets past the format check: the next refusal is the CPU tensor
    x = torch.zeros(4, 64)
    codes, scales = torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        bnb.matmul_mxfp4(x, codes, scales, act_format="none")
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        layer(x)


def test_state_dict_round_trip_with_none():
    layer = bnb.LinearMXFP4(64, 8, act_format="none")
    sd = layer.state_dict()
    assert set(sd) == {"weight", "weight_scales", "bias"}
    sd["weight"] = torch.arange(8 * 32, dtype=torch.uint8).reshape(8, 32)
    sd["weight_scales"] = torch.arange(16, dtype=torch.uint8).reshape(8, 2)
    other = bnb.LinearMXFP4(64, 8, act_format="none")
    other.load_state_dict(sd)
    assert torch.equal(other.weight, sd["weight"]) and torch.equal(other.weight_scales, sd["weight_scales"]) and other.act_format == "none"
    quantising = bnb.LinearMXFP4(64, 8)                      # the buffers are the same whatever the activation format
    quantising.load_state_dict(other.state_dict())
    assert torch.equal(quantising.weight, sd["weight"]) and quantising.act_format == "fp8"


def test_what_is_still_refused():
    x = torch.zeros(4, 64)
    codes, scales = torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.uint8)
    for fmt in ("bf16", "fp6", "None", None, 0):
        with pytest.raises(ValueError, match="format"):
            bnb.matmul_mxfp4(x, codes, scales, act_format=fmt)
    for fmt in ("bf16", "fp6"):
        with pytest.raises(ValueError, match="format"):
            bnb.LinearMXFP4(64, 8, act_format=fmt)
    with pytest.raises(ValueError, match="format"):
        bnb.quantize_mx(x, "none")
    with pytest.raises(ValueError, match="format"):
        bnb.dequantize_mx(codes, scales, "none")
    layer = bnb.LinearMXFP4(64, 8, act_format="none")
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer(torch.zeros(2, 64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.matmul_mxfp4(x, layer.weight, layer.weight_scales, layer.bias, act_format="none")   # the bias Parameter requires grad


# ----------------------------------------------------------------------------- the tables
def _walk(x, w_codes, w_scales):
    """(block partial sums P[m, n, b] = sum_{k in b} x * value(code), unscaled; their scaled values) in float64, as k_mx_decode forms them"""
    M, K = x.shape
    c = emul.unpack(w_codes, "fp4").astype(np.int64)
    v = np.where(c & 8, -emul.FP4_GRID[c & 7], emul.FP4_GRID[c & 7])
    P = np.einsum("mbk,nbk->mnb", x.reshape(M, -1, 32), v.reshape(v.shape[0], -1, 32))
    return P, np.ldexp(P, (w_scales.astype(np.int64) - 127)[None, :, :])


def _normal_or_zero(a):
    a = np.abs(a[a != 0])
    return a.size == 0 or (a.min() >= NORMAL_MIN and a.max() < NORMAL_MAX)


@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)))
def test_every_exact_case_is_exact_in_f32_in_any_order(index):
    case = cases.EXACT_CASES[index]
    M, N, K, x_dtype, _, _ = case
    x, w, bias = cases.exact_operands(case, index)
    assert (cases.to_dtype(x, x_dtype).double().numpy() == x).all()
    w_codes, w_scales = emul.quantize(w, "fp4")
    assert (emul.decode_f64(w_codes, w_scales, "fp4") == w).all()
    unit = 2.0 ** -4                                          # x and w are multiples of 2^-2; the unscaled products too (values of 2^-1 up)
    total = np.abs(x) @ np.abs(w).T + (0 if bias is None else np.abs(bias)[None, :])
    assert total.max() / unit < 2.0 ** 24, total.max()
    P, scaled = _walk(x, w_codes, w_scales)
    assert (P % 2.0 ** -3 == 0).all() and (scaled % unit == 0).all() and np.abs(P).max() < 2.0 ** 20
    assert (scaled.sum(axis=2) == x @ w.T).all()
    assert _normal_or_zero(P) and _normal_or_zero(scaled) and _normal_or_zero(x @ w.T)


def test_the_exact_cases_cover_every_listed_size():
    Ms, Ns, Ks = ({c[i] for c in cases.EXACT_CASES} for i in range(3))
    assert Ms >= set(range(1, 18)) | {32, 33}
    assert Ns >= {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 1041}
    assert Ks == {32, 64, cases.CHUNK - 32, cases.CHUNK, cases.CHUNK + 32, 2 * cases.CHUNK + 32, 96, 128, 160, 1056, 2080} and 4128 in Ks
    sixteen = [c for c in cases.EXACT_CASES if c[3] != torch.float32]
    assert {c[3] for c in sixteen} == {torch.bfloat16, torch.float16} and {c[4] for c in cases.EXACT_CASES} == set(cases.DTYPES)
    assert {c[0] for c in sixteen} >= set(range(1, 18)) | {32, 33} and {c[5] for c in sixteen} == {True, False}
    # both 16-bit dtypes meet every K in both forms (one row: FMA; more: MFMA)
    assert {c[2] for c in sixteen if c[0] == 1} == Ks == {c[2] for c in sixteen if c[0] >= 2} and 2 * cases.ROUND + 32 == cases.CHUNK + 32
    # the f32 rows reach every FMA form past one lane-chunk
    f32 = [c for c in cases.EXACT_CASES if c[3] == torch.float32]
    assert {cases.decode_rows(c[0], c[3]) for c in f32 if c[2] > cases.CHUNK} == {1, 4, 8} and {cases.decode_rows(c[0], c[3]) for c in f32} == {1, 2, 4, 8}
    assert [cases.decode_rows(M, torch.bfloat16) for M in (1, 2, 3, 16, 17, 33)] == [1, 16, 16, 16, 16, 16]
    assert [cases.decode_rows(M, torch.float32) for M in (1, 2, 3, 5, 8, 9, 16, 33)] == [1, 2, 4, 8, 8, 8, 8, 8]
    assert cases.launch_text(5, torch.bfloat16) == "mx_decode_mfma bf16 MT16" and cases.launch_text(1, torch.float16) == "mx_decode f16 MT1"
    assert cases.launch_text(5, torch.float32) == "mx_decode f32 MT8"


@pytest.mark.parametrize("index", range(len(cases.WIDE_CASES)))
def test_every_wide_case_is_exact_and_normal(index):
    case = cases.WIDE_CASES[index]
    M, N, K, x_dtype, _, which = case
    x, w, w_codes, w_scales, a, c = cases.wide_operands(case, index)
    assert (cases.to_dtype(x, x_dtype).double().numpy() == x).all() and _normal_or_zero(x)
    assert (emul.decode_f64(w_codes, w_scales, "fp4") == w).all()
    P, scaled = _walk(x, w_codes, w_scales)
    unit = np.ldexp(1.0, a[:, None] + c[None, :] - 4)
    assert (scaled % unit[..., None] == 0).all()
    total = (np.abs(x) @ np.abs(w).T) / unit
    assert total.max() < 2.0 ** 24, total.max()               # multiples of the unit below 2^24 of it: exact in f32 in any order
    # inside a block the unscaled products are multiples of one unit too, and far fewer than 2^24 of it
    t = cases.WIDE_T[which][0]
    tb = np.array([t[b % len(t)] for b in range(K // 32)])
    p_unit = np.ldexp(1.0, a[:, None, None] + tb[None, None, :] - 3)      # x: multiples of 2^(a + t - 2), values: of 2^-1
    assert (P % p_unit == 0).all() and (np.abs(P) / p_unit).max() < 2.0 ** 24
    r = x @ w.T
    assert (scaled.sum(axis=2) == r).all() and (r != 0).all()
    assert _normal_or_zero(P) and _normal_or_zero(scaled) and _normal_or_zero(r)
    assert (np.abs(r) < 2.0 ** 100).all() and (np.abs(r) > 2.0 ** -100).all()


def test_the_wide_cases_reach_the_listed_scale_bytes_at_the_first_middle_and_last_block():
    nb = cases.WIDE_K // 32
    assert nb == 129 and nb % 8 == 1
    seen = {b: set() for b in (0, 64, nb - 1)}
    top_under_254 = set()
    for index, case in enumerate(cases.WIDE_CASES):
        _, w, w_codes, w_scales, _, _ = cases.wide_operands(case, index)
        wc = emul.unpack(w_codes, "fp4").reshape(w.shape[0], nb, 32)
        live = ((wc & 7) != 0).any(axis=2)
        for b in seen:
            seen[b] |= set(w_scales[live[:, b], b].tolist())
            if (((wc[:, b] & 7) == 7).any(axis=1) & (w_scales[:, b] == 254)).any():
                top_under_254.add(b)
        assert case[3] in (torch.bfloat16, torch.float32)
    for b, s in seen.items():
        assert s >= {0, 1, 253, 254}, (b, sorted(s))
    assert top_under_254 == set(seen)
    every = set()
    for index, case in enumerate(cases.WIDE_CASES):
        every |= set(np.unique(cases.wide_operands(case, index)[3]).tolist())
    assert every >= {0, 1, 126, 127, 128, 253, 254}, sorted(every)


def test_the_subnormal_cases_have_normal_operands_and_partial_sums():
    assert len(cases.SUBNORMAL_CASES) == 2
    for index, case in cases.SUBNORMAL_CASES:
        x, w, w_codes, w_scales = mx_cases.range_operands(case, index)
        assert case[7] == torch.float32 and (cases.to_dtype(x, case[6]).double().numpy() == x).all() and _normal_or_zero(x)
        P, scaled = _walk(x, w_codes, w_scales)
        r = x @ w.T
        assert _normal_or_zero(P) and (np.abs(r) < NORMAL_MIN).all() and (r != 0).all() and (r % 2.0 ** -149 == 0).all()
        assert (scaled % 2.0 ** -149 == 0).all() and (scaled.sum(axis=2) == r).all()
        want = cases.expected_subnormal_output(r)
        if cases.SUBNORMAL_RESULTS_KEPT:
            assert (want.double().numpy() == r).all()
        else:
            assert bool((want == 0).all()) and (np.signbit(want.numpy()) == (r < 0)).all()


def test_the_nan_cross_random_and_offset_tables():
    M, N, K = cases.NAN_SHAPE
    assert K == 2 * cases.CHUNK + 32 and cases.NAN_BLOCKS == (0, 64, K // 32 - 1) and 0 <= cases.NAN_COLUMN < N and M == 3
    assert cases.X_BAD_KS == (0, 31, 32, cases.CHUNK - 1, cases.CHUNK, K - 1)
    x, w = cases.nan_operands()
    assert (np.abs(x) @ np.abs(w).T).max() < 2.0 ** 20
    assert cases.CROSS_SHAPE == (3, 5, 64) and len(cases.CROSS_CASES) == 36 == len(set(cases.CROSS_CASES))
    x, w, bias = cases.cross_operands()
    for dt in cases.DTYPES:
        assert (cases.to_dtype(x, dt).double().numpy() == x).all() and (cases.to_dtype(bias, dt).double().numpy() == bias).all()
    assert (np.abs(x) @ np.abs(w).T + np.abs(bias)).max() < 2.0 ** 20
    assert cases.RANDOM_SHAPES == ((5, 261, 1056), (16, 133, 4128)) and {c[1] for c in cases.RANDOM_CASES} == set(cases.DTYPES)
    for off in cases.OFFSETS:
        assert off["x"] % 16 == 0 and off["w_codes"] % 16 == 0
    assert {o["x"] for o in cases.OFFSETS} == {0, 16, 32, 48} == {o["w_codes"] for o in cases.OFFSETS}
    assert {o["w_scales"] % 4 for o in cases.OFFSETS} == {1, 2, 3} and any(o["out"] % 2 for o in cases.OFFSETS)
    for M, N, K in cases.OFFSET_SHAPES:
        xo, wo = emul.lossless(M, K, seed=18001), emul.lossless(N, K, seed=18002)
        assert (np.abs(xo) @ np.abs(wo).T).max() + 8 < 2.0 ** 20
    assert cases.COMPOSED_SHAPE == (17, 9, 128)
