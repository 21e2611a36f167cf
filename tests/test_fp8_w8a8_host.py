"""The W8A8 FP8 linear without a GPU: exports, refusals, the Python surface, the numpy restatement of the row
quantiser on hand-written values, and the exact GEMM cases of tests/test_gpu_fp8_w8a8.py shown to be lossless."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8_native as fn
from tests import mx_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32, F32_, BF16_, F16_ = 0, 1, 2, torch.float32, torch.bfloat16, torch.float16      # the C ABI's codes; torch's dtypes


def quantize_rows(x):
    """x [M, K], anything that converts to f32 exactly -> (codes uint8 [M, K], scales f32 [M]) by include/mbnb_fp8.h's rule"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    top = (x.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1)
    amax = top.view(np.float32)
    bad, zero = top >= 0x7F800000, top == 0
    with np.errstate(all="ignore"):
        scales = (amax / np.float32(448.0)).astype(np.float32)
        r = (np.float32(448.0) / amax).astype(np.float32)
        p = np.abs(x * r[:, None]).astype(np.float32).astype(np.float64)     # ONE f32 product
    p = np.where(np.isnan(p), 0.0, p)                                         # 0 x an overflowed r: the element was a zero
    codes = emul._nearest_even_code(p, emul.FP8_GRID) | (np.signbit(x).astype(np.uint8) << 7)
    codes = np.where((bad | zero)[:, None], 0, codes).astype(np.uint8)
    scales = np.where(bad, np.float32(np.nan), np.where(zero, np.float32(0.0), scales)).astype(np.float32)
    return codes, scales


def decode(codes):                 # E4M3 codes (no NaN code) -> float64
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c & 0x80, -1.0, 1.0) * emul.FP8_GRID[c & 0x7F]


def code_of(values):               # exactly representable values -> their E4M3 codes
    v = np.asarray(values, dtype=np.float64)
    c = np.searchsorted(emul.FP8_GRID, np.abs(v))
    assert (emul.FP8_GRID[c] == np.abs(v)).all()
    return (c | (np.signbit(v) << 7)).astype(np.uint8)


def test_the_restatement_on_hand_written_rows():
    row = np.zeros((6, 16), dtype=np.float32)
    # row 0: amax 448, so r = 1: ties between neighbouring codes go to the even code, both ways, and the subnormal tie
    row[0, :8] = [448.0, 1.0625, 1.1875, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, 17.0, -0.0]
    row[1, :3] = [1.0, -0.5, 0.999]         # amax 1 -> r = 448: the maximum lands on 448 (0x7E), half of it on 224, nothing is clipped
    # row 2: all zeros; row 3: an Inf; row 4: a NaN; row 5: a subnormal maximum (r overflows: the zeros stay zeros)
    row[3, 5], row[4, 15], row[5, 0] = np.inf, np.nan, 2.0 ** -140
    codes, scales = quantize_rows(row)
    assert codes[0, :8].tolist() == [0x7E, 0x38, 0x3A, 0xB8, 0x00, 0x02, 0x58, 0x80]     # 1.0625 -> 1.0, 1.1875 -> 1.25, 17 -> 16
    assert codes[1, :3].tolist() == [0x7E, 0xF6, 0x7E] and scales[1] == np.float32(1.0) / np.float32(448.0)
    assert scales[0] == 1.0 and scales[2] == 0.0 and np.isnan(scales[3]) and np.isnan(scales[4]) and not codes[2:5].any()
    assert codes[5].tolist() == [0x7E] + [0] * 15 and scales[5] == np.float32(2.0 ** -140) / np.float32(448.0)


# The tile is 256 x 128 below MBNB_FP8_WIDE_TILES wide tiles and 256 x 256 from there up; K-step 128, two K-steps in flight, so 400
# = (2 + 1) K-steps + 16 takes every stage twice and ends on a partial step.  K 16 and 112 end inside the first step, 144 in the second.
EXACT_M, EXACT_N = (1, fn.TM - 1, fn.TM, fn.TM + 1), (1, fn.TN_NARROW - 1, fn.TN_NARROW, fn.TN_NARROW + 1)
EXACT_K = (16, 112, 128, 144, (fn.STEPS_IN_FLIGHT + 1) * fn.KS + 16)
EXACT_SHAPES = [(M, N, K) for M in EXACT_M for N in EXACT_N for K in EXACT_K]
# The 256 x 256 tile needs 256 of its tiles.  (M, N, K, out dtype, bias dtype): tile-exact, tile + 1 and one-row / 255-column last
# tiles, N % 4 == 0 (vector stores) and not; K = 400 and 912 put real data of K-step t + 2 into a freed stage, 3 and 8 times
WIDE_CASES = [(16 * fn.TM, 16 * fn.TN, 400, F32_, None), (16 * fn.TM + 1, 16 * fn.TN + 4, 400, BF16_, F16_),
              (15 * fn.TM + 1, 16 * fn.TN - 1, 400, F16_, BF16_), (16 * fn.TM, 16 * fn.TN + 4, 912, BF16_, F32_),
              (15 * fn.TM + 1, 16 * fn.TN - 1, 144, F32_, F32_)]


def exact_case(M, N, K, seed=0):
    """codes that decode to integers in [-8, 8], power-of-two scales, a small integer bias: (a, sA, w, sW, bias), numpy"""
    rng = np.random.default_rng(1000 * seed + M + 7 * N + 13 * K)
    a, w = rng.integers(-8, 9, (M, K)), rng.integers(-8, 9, (N, K))
    sA, sW = 2.0 ** rng.integers(-2, 2, M), 2.0 ** rng.integers(-2, 2, N)
    return code_of(a), sA.astype(np.float32), code_of(w), sW.astype(np.float32), rng.integers(-4, 5, N).astype(np.float32)


def test_every_exact_case_is_lossless():
    """sum |a w| < 2^24: every partial sum is an integer f32 holds, in any order; the scaled sum plus the bias is a multiple of 2^-4
    below 2^20, so every f32 step of the epilogue is exact and the one rounding to the output dtype is the only one"""
    for M, N, K in EXACT_SHAPES + [c[:3] for c in WIDE_CASES]:
        a, sA, w, sW, bias = exact_case(M, N, K)
        A, W = torch.from_numpy(decode(a)).float(), torch.from_numpy(decode(w)).float()
        assert (A == A.round()).all() and A.abs().max() <= 8 and (W == W.round()).all() and W.abs().max() <= 8 and K <= 1024
        S = (A.abs() @ W.abs().T).double()                                       # integers below 2^24: exact in f32
        assert S.max() < 2.0 ** 24 and min(sA.min(), sW.min()) >= 0.25 and (np.log2(sA) % 1 == 0).all() and (np.log2(sW) % 1 == 0).all()
        assert (S * torch.from_numpy(sA)[:, None] * torch.from_numpy(sW)[None, :] + torch.from_numpy(np.abs(bias))[None, :]).max() < 2.0 ** 20


def test_header_binding_and_library_agree_on_the_exports():
    header = open(os.path.join(ROOT, "include", "mbnb_fp8.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_fp8_\w+)\s*\(", code)))
    out = subprocess.run(["nm", "-D", "--defined-only", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert declared == sorted(fn.EXPORTED_SYMBOLS) == sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))
    assert len(declared) == 7 and fn.lib().mbnb_fp8_abi_version() == fn.ABI_VERSION == int(re.search(r"MBNB_FP8_ABI_VERSION (\d+)", header).group(1))
    needed = subprocess.run(["readelf", "-d", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in "".join(line for line in needed.splitlines() if "NEEDED" in line)
    for macro, value in dict(TILE_M=fn.TM, TILE_N=fn.TN, TILE_N_NARROW=fn.TN_NARROW, K_STEP=fn.KS, STEPS_IN_FLIGHT=fn.STEPS_IN_FLIGHT, WIDE_TILES=fn.WIDE_TILES).items():
        assert int(re.search(rf"#define MBNB_FP8_{macro} (\d+)", header).group(1)) == value


P = 4096            # a pointer that is aligned and never dereferenced: every call below is refused, or has M == 0
ARGS = {      # in the order of the C signature; the stream (NULL) follows
    "quantize_rows": dict(x=P, xdt=F32, M=4, K=32, q=P, sA=P),
    "matmul": dict(a=P, sA=P, M=4, K=32, w=P, sW=P, N=8, bias=None, bdt=BF16, out=P, odt=BF16),
    "linear": dict(x=P, xdt=BF16, M=4, K=32, w=P, sW=P, N=8, bias=None, bdt=BF16, out=P, odt=BF16, ws=P, wsb=1 << 20),
}


def _call(name, **kw):
    return getattr(fn.lib(), "mbnb_fp8_" + name)(*{**ARGS[name], **kw}.values(), None)


REFUSALS = [
    ("quantize_rows", dict(xdt=3), fn.ERR_ARG, "unknown dtype"), ("quantize_rows", dict(K=24), fn.ERR_SHAPE, "multiple of 16"),
    ("quantize_rows", dict(K=0), fn.ERR_SHAPE, "K = 0"), ("quantize_rows", dict(M=-1), fn.ERR_SHAPE, "M = -1"),
    ("quantize_rows", dict(M=1 << 31), fn.ERR_SHAPE, "exceed one launch"), ("quantize_rows", dict(q=None), fn.ERR_ARG, "NULL"),
    ("quantize_rows", dict(x=P + 8), fn.ERR_ARG, "misaligned x or q"), ("quantize_rows", dict(q=P + 4), fn.ERR_ARG, "misaligned x or q"),
    ("matmul", dict(odt=-1), fn.ERR_ARG, "unknown dtype"), ("matmul", dict(bias=P, bdt=7), fn.ERR_ARG, "unknown dtype"),
    ("matmul", dict(K=40), fn.ERR_SHAPE, "multiple of 16"), ("matmul", dict(K=-16), fn.ERR_SHAPE, "K = -16"),
    ("matmul", dict(N=0), fn.ERR_SHAPE, "N = 0"), ("matmul", dict(M=-2), fn.ERR_SHAPE, "M = -2"),
    ("matmul", dict(M=1 << 30, N=1 << 30), fn.ERR_SHAPE, "N = "), ("matmul", dict(a=None), fn.ERR_ARG, "NULL a or sA"),
    ("matmul", dict(sW=None), fn.ERR_ARG, "NULL w, sW or out"), ("matmul", dict(a=P + 1), fn.ERR_ARG, "misaligned a"),
    ("matmul", dict(w=P + 8), fn.ERR_ARG, "misaligned w"), ("matmul", dict(out=P + 1), fn.ERR_ARG, "misaligned sW, out or bias"),
    ("linear", dict(xdt=5), fn.ERR_ARG, "unknown dtype"), ("linear", dict(K=8), fn.ERR_SHAPE, "multiple of 16"),
    ("linear", dict(x=None), fn.ERR_ARG, "NULL x"), ("linear", dict(x=P + 2), fn.ERR_ARG, "misaligned x"),
    ("linear", dict(w=None), fn.ERR_ARG, "NULL w, sW or out"), ("linear", dict(ws=None), fn.ERR_WORKSPACE, "workspace of 0 bytes, 512 needed"),
    ("linear", dict(wsb=511), fn.ERR_WORKSPACE, "workspace of 511 bytes, 512 needed"), ("linear", dict(ws=P + 8), fn.ERR_ARG, "misaligned workspace"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_every_refusal_is_a_status_and_a_text_before_any_hip_call(index):
    name, args, status, text = REFUSALS[index]
    assert _call(name, **args) == status and text in fn.lib().mbnb_fp8_last_error().decode(), (args, fn.lib().mbnb_fp8_last_error())


def test_no_rows_is_a_no_op_and_the_workspace_is_codes_then_scales():
    assert _call("quantize_rows", M=0, x=None, q=None, sA=None) == 0 == _call("matmul", M=0, a=None, sA=None, w=None, sW=None, out=None)
    assert _call("linear", M=0, x=None, w=None, sW=None, out=None, ws=None, wsb=0) == 0 == fn.workspace_bytes(0, 16)
    assert fn.workspace_bytes(4, 32) == 512 and fn.workspace_bytes(33, 1024) == 33 * 1024 + 256 and fn.workspace_bytes(5, 48) == 256 + 256 and fn.lib().mbnb_fp8_workspace_bytes(4, 8) == fn.ERR_SHAPE


def test_signatures_and_refusals_of_the_python_surface():
    for f, names, default in ((bnb.quantize_fp8_rows, ["tensor"], None), (bnb.linear_fp8_w8a8, ["input", "weight", "weight_scales", "bias", "dtype"], None),
                              (bnb.matmul_fp8_w8a8, ["A", "A_scales", "weight", "weight_scales", "bias", "dtype"], torch.bfloat16)):
        sig = inspect.signature(f).parameters
        assert list(sig) == names and getattr(bnb.functional, f.__name__) is f and f.__name__ in bnb.__all__
        assert "dtype" not in sig or sig["dtype"].default is default
    x, w, s = torch.zeros(2, 32), torch.zeros(8, 32, dtype=torch.uint8), torch.ones(8)
    for call in (lambda: bnb.quantize_fp8_rows(x), lambda: bnb.linear_fp8_w8a8(x, w, s), lambda: bnb.matmul_fp8_w8a8(w, s, w, s)):
        with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
            call()
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.linear_fp8_w8a8(x.requires_grad_(), w, s)
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.matmul_fp8_w8a8(w, s, w, s, bias=torch.zeros(8, requires_grad=True))


def test_linear_fp8_keeps_its_constructor_and_state_dict():
    assert bnb.LinearFP8.act_format == "none" and "act_format" not in inspect.signature(bnb.LinearFP8.__init__).parameters
    layer = bnb.LinearFP8(32, 8)
    keys = sorted(layer.state_dict())
    layer.act_format = "fp8"
    assert sorted(layer.state_dict()) == keys == ["bias", "weight_fp8", "weight_scales"] and bnb.LinearFP8.act_format == "none"
    with pytest.raises(NotImplementedError, match="inference-only"):     # LinearMXFP4's convention: the bias is a Parameter
        layer(torch.zeros(2, 32))
    with torch.no_grad(), pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        layer(torch.zeros(2, 32))
