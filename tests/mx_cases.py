"""The case tables and input builders that tests/test_mx_host.py, tests/test_gpu_mx.py and tests/test_gpu_mx_forms.py share (the
format: tests/mx_emul.py; the forms tables: DESIGN.md §26)."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _mx_native as mxn
from tests import mx_emul as emul

TM, TN, KS = mxn.TM, mxn.TN, mxn.KS

# Exact GEMM: (M, N, K, activation format, output dtype, bias).  Every value of
#   M in {1, 15, 16, 17, TM - 1, TM, TM + 1, 2 TM + 3}, N in {1, 16, 17, TN - 1, TN + 1, 2 TN + 5} (and TN, the aligned N),
#   K in {32, 96, 128, 160, KS, KS + 32, 3 KS + 32}
# has a case, and every pair of dimensions a ragged and an aligned one.
EXACT_CASES = [
    (1, 1, 32, "fp8", torch.bfloat16, False),
    (15, 16, 96, "fp4", torch.float16, True),
    (16, 17, 128, "fp8", torch.float32, True),
    (17, TN - 1, 160, "fp4", torch.bfloat16, False),
    (TM - 1, TN + 1, 3 * KS + 32, "fp8", torch.float16, True),
    (TM, 16, KS, "fp4", torch.float32, False),
    (TM + 1, 2 * TN + 5, 32, "fp8", torch.bfloat16, True),
    (2 * TM + 3, 1, 128, "fp4", torch.bfloat16, True),
    (TM, TN, 3 * KS + 32, "fp8", torch.bfloat16, False),
    (2 * TM + 3, 2 * TN + 5, KS + 32, "fp4", torch.float16, False),
    (16, TN, 96, "fp8", torch.float16, False),
    (17, 16, 3 * KS + 32, "fp4", torch.float32, True),
    (1, 2 * TN + 5, KS, "fp4", torch.bfloat16, False),
    (15, TN + 1, 128, "fp8", torch.float32, False),
    (TM - 1, 17, 96, "fp4", torch.bfloat16, True),
    (TM + 1, TN - 1, KS, "fp8", torch.float16, True),
]


def exact_operands(case, index):
    """(x float64 [M, K], w float64 [N, K], bias float64 [N] or None) of an exact case: lossless rows, a bias of small integers"""
    M, N, K, _, _, has_bias = case
    x = emul.lossless(M, K, seed=1000 + 2 * index)
    w = emul.lossless(N, K, seed=1001 + 2 * index)
    bias = np.random.default_rng(3000 + index).integers(-8, 9, size=N).astype(np.float64) if has_bias else None
    return x, w, bias


def to_dtype(values, dtype):
    """float64 array -> torch tensor of `dtype`, one rounding (the values used here are exact in f32 or round once from it)"""
    return torch.from_numpy(np.ascontiguousarray(values)).to(torch.float32).to(dtype)


def as_f32(t):
    return t.to(torch.float32).numpy()


# ---------------------------------------------------------------- the quantiser's data sets
def _ulp_neighbours(t):
    """t, and t one unit in the last place of its dtype below and above (by magnitude), as one tensor [3, ...]"""
    if t.dtype == torch.float32:
        bits = t.view(torch.int32)
        return torch.stack([t, (bits - 1).view(torch.float32), (bits + 1).view(torch.float32)])
    bits = t.view(torch.int16)
    return torch.stack([t, (bits - 1).view(t.dtype), (bits + 1).view(t.dtype)])


def _midpoints(elem):
    grid = emul.GRID[elem]
    return (grid[:-1] + grid[1:]) / 2


def _anchor(elem):
    return 6.0 if elem == "fp4" else 448.0        # fixes the block's scale: amax in [4, 8) or [256, 512)


def _blocks_from(values, anchor, dtype):
    """A 1-D tensor of `dtype` -> blocks [n, 32], each with `anchor` (a float) at element 0 and 31 values behind it (zero padded)"""
    n = (values.numel() + 30) // 31
    out = torch.zeros(n, 32, dtype=dtype)
    flat = torch.zeros(n * 31, dtype=dtype)
    flat[:values.numel()] = values
    out[:, 1:] = flat.reshape(n, 31)
    out[:, 0] = anchor
    return out


def quantiser_blocks(kind, elem, dtype):
    """Blocks [n, 32] of `dtype` for one data set of the quantiser test"""
    rng = np.random.default_rng(sum(map(ord, kind + elem + str(dtype))))
    if kind == "binades":                         # normal data spread over 40 binades
        v = rng.standard_normal((64, 32)) * np.exp2(rng.integers(-20, 20, size=(64, 32)))
        if dtype == torch.float16:
            v = v * 2.0 ** -4                     # keep the top of the spread inside f16
        return to_dtype(v, dtype)
    scales = (-6, 0, 5) if dtype == torch.float16 else (-100, -6, 0, 60)
    if kind == "midpoints":                       # every rounding midpoint, and one ulp of the input dtype to either side of it
        out = []
        for s in scales:
            mids = to_dtype(_midpoints(elem) * 2.0 ** s, dtype)
            vals = _ulp_neighbours(mids).reshape(-1)
            sign = torch.tensor([1.0, -1.0], dtype=dtype).repeat((vals.numel() + 1) // 2)[:vals.numel()]
            out.append(_blocks_from(vals * sign, _anchor(elem) * 2.0 ** s, dtype))
        return torch.cat(out)
    if kind == "saturating":                      # amax itself above the largest element value: (6, 8) and (448, 512)
        top, limit = (6.0, 8.0) if elem == "fp4" else (448.0, 512.0)
        out = []
        for s in scales:
            fr = (top + np.array([2.0 ** -6, 0.1, 0.3, 0.5, 0.8, 1.0 - 2.0 ** -6]) * (limit - top)) * 2.0 ** s
            vals = to_dtype(np.concatenate([fr, -fr, fr * 0.5, fr * 0.25]), dtype)
            out.append(_blocks_from(vals, float(fr[-1]), dtype))
            out.append(_blocks_from(-vals, -float(fr[0]), dtype))
        return torch.cat(out)
    assert kind == "special"                      # zero, subnormal and non-finite blocks
    z = torch.zeros(8, 32, dtype=dtype)
    z[1, 1::2] = -0.0
    tiny = torch.finfo(dtype).smallest_normal
    z[2] = to_dtype(rng.integers(-7, 8, size=32) * (tiny / 8), dtype)            # a subnormal amax of the input dtype
    z[3] = to_dtype(rng.standard_normal(32), dtype)
    z[3, 5] = float("nan")
    z[4] = to_dtype(rng.standard_normal(32), dtype)
    z[4, 31] = float("inf")
    z[5] = to_dtype(rng.standard_normal(32), dtype)
    z[5, 0] = float("-inf")
    z[6] = torch.finfo(dtype).max                                                # E = 254 in f32
    z[6, 1::3] = -torch.finfo(dtype).max / 3
    z[7] = to_dtype(rng.standard_normal(32) * tiny * 4, dtype)                   # around the smallest normal: scale byte 0 or near it
    return z


QUANT_KINDS = ("binades", "midpoints", "saturating", "special")
QUANT_SHAPES = ((1, 32), (3, 96), (17, 160), (64, 1024))


def quantiser_input(kind, elem, dtype, rows, K):
    """[rows, K] of `dtype`: the data set's blocks, repeated to fill the shape"""
    blocks = quantiser_blocks(kind, elem, dtype)
    need = rows * K // 32
    idx = torch.arange(need) % blocks.shape[0]
    return blocks[idx].reshape(rows, K // 32, 32).reshape(rows, K).contiguous()


# ============================================================================= forms and limits (tests/test_gpu_mx_forms.py)
# DESIGN.md §26.  Every table below is closed by tests/test_mx_host.py on the CPU: exactness, byte / code / position coverage,
# the planting plan, the dtype cross.
X_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
K_RAGGED = 3 * KS + 64                            # 14 k blocks, two of them in the ragged last K-step

# ---------------------------------------------------------------- A. wide-scale exact GEMM
# Two sets of per-block offsets t_b (emul.wide).  "low": x rows span 2^(t - 2) .. 2^(t + 2), w columns 2^(-t - 4) .. 2^(-t): t = 123
# puts the activation's amax at the top of f32 (exponent field 254: byte 252 fp4, 246 fp8) and the weight on bytes 0 .. 4; t = -125
# puts the activation on fp4 bytes 0 .. 4 over non-zero codes.  "high": x rows 2^t .. 2^(t + 4): t = -127 puts the weight on
# bytes 250 .. 254 (code 7 under byte 254 is 6 * 2^127, no f32) against activation blocks of 2^-127 .. 2^-123.
WIDE_T = {"low": ((123, 122, 60, 0, -60, -118, -125, 1), -1, -3),
          "high": ((-127, -126, -60, 0, 60, 121, 120, 1), 1, -3)}
WIDE_CASES = [(M, N, K, act, (torch.float32, torch.bfloat16)[(i + j + l) % 2], out_dtype, which)
              for i, (M, N, K) in enumerate(((17, 19, 256), (TM + 1, TN + 1, K_RAGGED)))
              for j, act in enumerate(("fp8", "fp4"))
              for l, out_dtype in enumerate((torch.float32, torch.bfloat16))
              for which in ("low", "high")]


def wide_operands(case, index):
    """(x float64, w float64, w codes, w scale bytes, a_i, c_j) of a WIDE case; the weight's codes come from its values directly"""
    M, N, K, _, _, _, which = case
    t, a0, c0 = WIDE_T[which]
    x, w, a, c = emul.wide(M, N, K, t, a0, c0, seed=4000 + 2 * index)
    w_codes, w_scales = lossless_codes_checked(w)
    return x, w, w_codes, w_scales, a, c


def lossless_codes_checked(w):
    """emul.lossless_codes with the byte range asserted (an exponent outside E8M0 would wrap in uint8)"""
    v = w.reshape(w.shape[0], -1, 32)
    e = np.floor(np.log2(np.abs(v).max(axis=2))).astype(np.int64) - 2 + 127
    assert e.min() >= 0 and e.max() <= 254, (e.min(), e.max())
    codes, scales = emul.lossless_codes(w)
    assert (scales == e).all()
    return codes, scales


# Results outside the normal f32 range: (name, M, N, K, a_i = a[i % 3], c, x dtype, output dtype); operands emul.one_signed, so a
# row's products share a sign and no partial sum passes the whole one.
#   overflow      rows with a + c = 120: no product reaches 2^128, every sum does; rows with a = 0 stay ordinary numbers
#   f16-overflow  sums near 2^15, 2^19, 2^23: f32 holds them exactly, f16 rounds the larger ones to +-Inf
#   subnormal     a + c = -140: sums of multiples of 2^-144 below 2^-126
RANGE_CASES = [
    ("overflow", 17, 19, 256, (60, 60, 0), 60, torch.bfloat16, torch.float32),
    ("overflow", 17, 19, 256, (60, 0, 60), 60, torch.float32, torch.bfloat16),
    ("f16-overflow", 17, 19, 256, (0, 4, 8), 4, torch.float16, torch.float16),
    ("subnormal", 17, 19, 256, (-70, -70, -72), -70, torch.float32, torch.float32),
    ("subnormal", 17, 19, 256, (-70, -72, -70), -70, torch.bfloat16, torch.float32),
]


def range_operands(case, index):
    _, M, N, K, a3, c, _, _ = case
    a = np.array([a3[i % 3] for i in range(M)])
    x, w = emul.one_signed(M, N, K, a, np.full(N, c), seed=4500 + 2 * index)
    w_codes, w_scales = lossless_codes_checked(w)
    return x, w, w_codes, w_scales


# What k_gemm_mx's accumulator does with a result below 2^-126, as measured on the MI355X: True = the f32
# subnormal is kept, correctly rounded; False = a zero of the result's sign.
SUBNORMAL_RESULTS_KEPT = True


def expected_range_output(r64, out_dtype):
    """the float64 result -> what the kernel must store: one rounding, and the measured treatment of f32 subnormals"""
    y = to_dtype(r64, torch.float32)
    if not SUBNORMAL_RESULTS_KEPT:
        tiny = y.abs() < 2.0 ** -126
        y = torch.where(tiny, torch.copysign(torch.zeros_like(y), y), y)
    return y.to(out_dtype)


# ---------------------------------------------------------------- B. every E4M3 code at every k position of the K-step
E4M3_FINITE = tuple(c for c in range(256) if c & 0x7F != 0x7F)              # 254 codes, +-0 and the subnormals among them
FP8_CODE_N = 33                                   # column j sums the k with k % 33 == j: three column fragments, <= 14 terms each
FP8_CODE_CASES = [(2 * len(E4M3_FINITE), FP8_CODE_N, KS), (2 * TM + 3, FP8_CODE_N, K_RAGGED)]


def fp8_anchor_places(M, K):
    """[M, K / 32]: the place (0 or 1) of the anchor 448 in each block: it alternates with the K-step and with i // 254, so every
    k mod 128 is free of it in some K-step or some band of rows"""
    return ((np.arange(K // 32)[None, :] // 4) + (np.arange(M)[:, None] // len(E4M3_FINITE))) % 2


def fp8_code_operands(case):
    """(x float32 [M, K], its E4M3 codes [M, K], w codes [N, K / 2], w scale bytes): row i holds code E4M3_FINITE[(i + k) % 254] at
    k, except the anchor 448 (code 0x7E, byte 127, so the scaled values are the inputs); column j has +-1 (codes 2 / 10, byte 127)
    at the k with k % 33 == j and zeros elsewhere, so every element of x reaches exactly one output, and a column sums at most 14
    values of at most 448 (the anchors, whose place moves from row to row, are summed like any other element)"""
    M, N, K = case
    table = np.array(E4M3_FINITE, dtype=np.uint8)
    i, k = np.arange(M)[:, None], np.arange(K)[None, :]
    codes = table[(i + k) % len(table)]
    place = np.repeat(fp8_anchor_places(M, K), 32, axis=1)
    codes = np.where(k % 32 == place, 0x7E, codes).astype(np.uint8)
    x = emul.decode_f64(codes, np.full((M, K // 32), 127, dtype=np.uint8), "fp8").astype(np.float32)
    wk = np.arange(K)
    one = np.where((wk // N) % 2 == 0, 2, 10)
    wc = np.where(wk[None, :] % N == np.arange(N)[:, None], one[None, :], 0).astype(np.uint8)
    w_codes = (wc[:, 0::2] | (wc[:, 1::2] << 4)).astype(np.uint8)
    return x, codes, w_codes, np.full((N, K // 32), 127, dtype=np.uint8)


# ---------------------------------------------------------------- C. NaN masks at every fragment place
NAN_M, NAN_N, NAN_K = TM + 17, TN + 17, K_RAGGED
NAN_PLACES = (0, 5, 15, 16, 47, 64, 100, 127, 128, NAN_M - 1)              # rows of x, and columns of the output (NAN_M == NAN_N)
NAN_VALUES = (float("nan"), float("inf"), float("-inf"))
NAN_BLOCKS = NAN_K // 32
# run r plants place q's bad value in k block (q + r) % 14, at element (7 q + 3 r) % 32 of it
NAN_PLAN = [[(p, (q + r) % NAN_BLOCKS, (7 * q + 3 * r) % 32, NAN_VALUES[(q + 2 * r) % 3]) for q, p in enumerate(NAN_PLACES)]
            for r in range(NAN_BLOCKS)]


def nan_operands():
    x = emul.lossless(NAN_M, NAN_K, seed=5001)
    w = emul.lossless(NAN_N, NAN_K, seed=5002)
    return x, w


# ---------------------------------------------------------------- D. K % 128 == 64
K64_CASES = [(M, N, K, act) for K in (64, 192) for act in ("fp8", "fp4") for M in (1, 17, TM + 1) for N in (1, 17, TM + 1)]


def k64_operands(case, index):
    M, N, K, _ = case
    return emul.lossless(M, K, seed=6000 + 2 * index), emul.lossless(N, K, seed=6001 + 2 * index)


# ---------------------------------------------------------------- E. the dtype cross at (17, 19, 160)
CROSS_SHAPE = (17, 19, 160)
CROSS_CASES = [(xd, bd, od, act) for act in ("fp8", "fp4") for xd in X_DTYPES for bd in (None,) + X_DTYPES for od in OUT_DTYPES]


def cross_operands():
    M, N, K = CROSS_SHAPE
    bias = np.random.default_rng(7003).integers(-8, 9, size=N).astype(np.float64)
    return emul.lossless(M, K, seed=7001), emul.lossless(N, K, seed=7002), bias


# ---------------------------------------------------------------- F. guarded, offset operands
ABI_SHAPES = ((1, 32), (3, 96), (17, 160), (8, 256), (64, 1024))           # rows x K / 8 groups: 4, 36, 340 and 256, 8192
SCALE_OFFSETS = (0, 1, 3)
LINEAR_OFFSETS = [dict(w_scales=1, out=1, bias=1, workspace=16), dict(w_scales=3, out=1, bias=0, workspace=0),
                  dict(w_scales=0, out=0, bias=1, workspace=16)]           # w_scales in bytes, out / bias in elements, workspace in bytes

# ---------------------------------------------------------------- G. random data: (x dtype, output dtype, activation format, data)
RANDOM_SHAPE = (TM + 37, TN + 5, 1024)
RANDOM_CASES = [(xd, od, act, kind) for act in ("fp8", "fp4")
                for xd, od, kind in ((torch.bfloat16, torch.bfloat16, "normal"), (torch.float16, torch.float16, "normal"),
                                     (torch.float32, torch.float32, "normal"), (torch.float32, torch.float16, "normal"),
                                     (torch.bfloat16, torch.float32, "heavy"), (torch.float16, torch.float16, "heavy"))]


def random_operands(x_dtype, kind):
    """(x, w, bias): N(0, 1) x N(0, 0.02^2); "heavy" multiplies 1 % of x's columns by 64, the shape of LLM activations, so the block
    bytes spread within a row"""
    from mps_bitsandbytes_amd import synthetic
    M, N, K = RANDOM_SHAPE
    x = synthetic.normal((M, K), torch.float32, seed=8001)
    if kind == "heavy":
        cols = np.random.default_rng(8004).choice(K, size=K // 100, replace=False)
        x[:, torch.from_numpy(cols)] *= 64.0
    w = synthetic.normal((N, K), torch.bfloat16, seed=8002, std=0.02)
    bias = synthetic.normal((N,), torch.bfloat16, seed=8003, std=0.1)
    return x.to(x_dtype), w, bias


# ---------------------------------------------------------------- I. past 2^31 bytes
BIG_M, BIG_N, BIG_K, BIG_PATTERN = 65536 + 129, 16, 32768, 251
BIG_ROWS = tuple(range(4)) + tuple(range(BIG_M - 140, BIG_M))
