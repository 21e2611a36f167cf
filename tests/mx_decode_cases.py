"""The case tables of the weight-only MXFP4 decode linear, shared by tests/test_mx_decode_host.py (which closes them
on the CPU) and tests/test_gpu_mx_decode.py.  The format and the generators: tests/mx_emul.py.

The constants the edges follow (csrc/mx_kernels.hip).  k_mx_decode, the FMA form (one 16-bit row, and every f32 call): a wave pass
covers CHUNK = 2048 k of a weight row (64 lanes x one MX block); a workgroup pass serves MT = 1, 2, 4 or 8 activation rows and
4 RW weight rows with RW = 1 (MT 1), 2 (MT 2, 4) or 4 (MT 8) rows per wave, so a workgroup's weight rows end at N = 4, 8 and 16.
k_mx_decode_mfma (2 and more 16-bit rows): a workgroup owns 16 weight rows and passes of 16 activation rows; its 8 waves take
k-steps of STEP = 128 k in turn, so a round of the workgroup is ROUND = 1024 k, and it requests two rounds at a time."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _mx_native as mxn
from tests import mx_cases, mx_emul as emul

CHUNK, STEP, ROUND = 2048, 128, 1024
ROWS = mxn.DECODE_ROWS
FMA_ROWS = ROWS // 2
X16 = (torch.bfloat16, torch.float16)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
to_dtype, as_f32 = mx_cases.to_dtype, mx_cases.as_f32


def decode_rows(M, x_dtype):
    """the activation rows per pass the host picks (csrc/mx_kernels.hip decode_mfma, decode_rows)"""
    if x_dtype != torch.float32 and M >= 2:
        return ROWS
    mt = 1
    while mt < M and mt < FMA_ROWS:
        mt *= 2
    return mt


def launch_text(M, x_dtype):
    name = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[x_dtype]
    form = "mx_decode_mfma" if x_dtype != torch.float32 and M >= 2 else "mx_decode"
    return f"{form} {name} MT{decode_rows(M, x_dtype)}"


# ---------------------------------------------------------------- exact cases: (M, N, K, x dtype, out dtype, bias)
# every M of 1 .. 17, 32, 33; N on both sides of the rows per wave (1, 2, 4) and per workgroup (4, 8, 16); K of one block, two,
# a k-step of the MFMA form minus / exactly / plus one block, a round of its workgroup plus one block, one lane-chunk of the FMA
# form minus / exactly / plus one block, and two chunks plus one block.  The issue's list (bf16 and f16 x) first; then f32 rows,
# which are lossless too and are the only way into the FMA forms MT 2, 4, 8.
EXACT_MS = tuple(range(1, 18)) + (32, 33)
EXACT_NS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
EXACT_KS = (32, 64, CHUNK - 32, CHUNK, CHUNK + 32, 2 * CHUNK + 32, STEP - 32, STEP, STEP + 32, ROUND + 32)
EXACT_CASES = [(M, EXACT_NS[(3 * i) % len(EXACT_NS)], EXACT_KS[i % len(EXACT_KS)], X16[i % 2], DTYPES[i % 3], bool((i // 2) % 2))
               for i, M in enumerate(EXACT_MS)]
# every K against a full pass of rows with N past one workgroup, every N at the chunk edge, one row against every K
EXACT_CASES += [(ROWS, 17, K, X16[(i + 1) % 2], DTYPES[(i + 1) % 3], bool(i % 2)) for i, K in enumerate(EXACT_KS)]
EXACT_CASES += [((1, 2, 3, 5, 9)[i % 5], N, (CHUNK + 32, CHUNK - 32)[i % 2], X16[i % 2], DTYPES[(i + 2) % 3], bool((i + 1) % 2))
                for i, N in enumerate(EXACT_NS)]
EXACT_CASES += [(1, 5, K, X16[i % 2], DTYPES[i % 3], bool(i % 2)) for i, K in enumerate(EXACT_KS)]
# two rounds of the MFMA workgroup plus a block, and an N of many workgroups
EXACT_CASES += [(2, 9, 2 * ROUND + 32, torch.bfloat16, torch.float16, True), (3, 1041, STEP + 32, torch.bfloat16, torch.bfloat16, True)]
EXACT_CASES += [(M, N, K, torch.float32, DTYPES[i % 3], bool(i % 2))
                for i, (M, N, K) in enumerate(((1, 5, CHUNK + 32), (2, 9, CHUNK - 32), (3, 7, 2 * CHUNK + 32), (4, 8, 64), (5, 17, CHUNK + 32),
                                               (8, 16, CHUNK), (9, 15, 32), (16, 33, STEP + 32), (17, 3, CHUNK - 32)))]


def exact_operands(case, index):
    """(x float64 [M, K], w float64 [N, K], bias float64 [N] or None): lossless rows, a bias of small integers"""
    M, N, K, _, _, has_bias = case
    x = emul.lossless(M, K, seed=11000 + 2 * index)
    w = emul.lossless(N, K, seed=11001 + 2 * index)
    bias = np.random.default_rng(13000 + index).integers(-8, 9, size=N).astype(np.float64) if has_bias else None
    return x, w, bias


# ---------------------------------------------------------------- scale bytes: (M, N, K, x dtype, out dtype, which)
# emul.wide: x[i, block b] = lossless * 2^(a_i + t_b), w[j, block b] = lossless * 2^(c_j - t_b).  The offsets t_b repeat with
# period 8, and K = 2 CHUNK + 32 has 129 blocks, so t[0] lies on the first block (0), the first block of the second lane-chunk
# (64, the middle) and the last block (128).  "low": t_b = 123 puts the weight on bytes 0 .. 4 and x near 2^94; "high": t_b = -127
# puts it on bytes 250 .. 254 (code 7 under byte 254 is 6 * 2^127, no f32) and x near 2^-96; t_b = -1, 0 give bytes 123 .. 128.
# a_0 is chosen so that x, every block's unscaled partial sum and every result are normal f32 numbers.
WIDE_T = {"low": ((123, 122, 60, 0, -1, -60, 1, -2), -30, -3),
          "high": ((-127, -126, -60, 0, -1, 60, 1, -2), 30, -3)}
WIDE_K = 2 * CHUNK + 32
WIDE_CASES = [(M, N, WIDE_K, xd, od, which)
              for (M, N), xd, od in (((3, 9), torch.bfloat16, torch.float32), ((5, 5), torch.float32, torch.bfloat16),
                                     ((16, 17), torch.bfloat16, torch.bfloat16), ((9, 4), torch.float32, torch.float32))
              for which in ("low", "high")]


def wide_operands(case, index):
    """(x float64, w float64, w codes, w scale bytes, a_i, c_j)"""
    M, N, K, _, _, which = case
    t, a0, c0 = WIDE_T[which]
    x, w, a, c = emul.wide(M, N, K, t, a0, c0, seed=14000 + 2 * index)
    w_codes, w_scales = mx_cases.lossless_codes_checked(w)
    return x, w, w_codes, w_scales, a, c


# A result below 2^-126 (mx_cases.RANGE_CASES "subnormal": sums of multiples of 2^-144 below 2^-126, from normal x and normal
# partial sums under scales near 2^-70).  What k_mx_decode's f32 FMA does with it, as measured on the MI355X:
# True = the f32 subnormal is kept, exactly; False = a zero of the result's sign.
SUBNORMAL_RESULTS_KEPT = True
SUBNORMAL_CASES = [(i, c) for i, c in enumerate(mx_cases.RANGE_CASES) if c[0] == "subnormal"]


def expected_subnormal_output(r64):
    y = to_dtype(r64, torch.float32)
    if not SUBNORMAL_RESULTS_KEPT:
        y = torch.where(y.abs() < 2.0 ** -126, torch.copysign(torch.zeros_like(y), y), y)
    return y


# ---------------------------------------------------------------- NaN scale bytes and non-finite activations
NAN_SHAPE = (3, 9, 2 * CHUNK + 32)                 # 129 blocks
NAN_COLUMN = 5
NAN_BLOCKS = (0, 64, 128)                          # the first, the first of the second lane-chunk, the last
X_BAD_ROW = 1
X_BAD_KS = (0, 31, 32, CHUNK - 1, CHUNK, NAN_SHAPE[2] - 1)      # k = 0, a block boundary, the lane-chunk boundary, K - 1
X_BAD_VALUES = (float("inf"), float("-inf"), float("nan"))


def nan_operands():
    M, N, K = NAN_SHAPE
    return emul.lossless(M, K, seed=15001), emul.lossless(N, K, seed=15002)


# ---------------------------------------------------------------- random data, the dtype cross, operand offsets
RANDOM_SHAPES = ((5, 261, 1056), (16, 133, 2 * CHUNK + 32))
RANDOM_CASES = [(shape, xd, od) for shape in RANDOM_SHAPES for xd, od in zip(DTYPES, (torch.bfloat16, torch.float32, torch.float16))]


def random_operands(shape, x_dtype):
    """x ~ N(0, 1) in x_dtype, w ~ N(0, 0.02^2) in f32 (to be quantised), bias ~ N(0, 1) in f32"""
    M, N, K = shape
    g = torch.Generator().manual_seed(16000 + M)
    x = torch.randn(M, K, generator=g).to(x_dtype)
    w = torch.randn(N, K, generator=g) * 0.02
    bias = torch.randn(N, generator=g)
    return x, w, bias


CROSS_SHAPE = (3, 5, 64)
CROSS_CASES = [(xd, bd, od) for xd in DTYPES for bd in (None,) + DTYPES for od in DTYPES]


def cross_operands():
    M, N, K = CROSS_SHAPE
    x, w = emul.lossless(M, K, seed=17001), emul.lossless(N, K, seed=17002)
    bias = np.random.default_rng(17003).integers(-8, 9, size=N).astype(np.float64)
    return x, w, bias


# bytes off a 16-byte boundary for x and the codes (16-byte steps), elements for out and bias, bytes for the scales
OFFSET_SHAPES = ((3, 9, 96), (17, 5, CHUNK + 32))
OFFSETS = [dict(x=16, w_codes=0, w_scales=1, out=1, bias=1), dict(x=0, w_codes=16, w_scales=3, out=3, bias=0),
           dict(x=32, w_codes=48, w_scales=2, out=0, bias=3), dict(x=48, w_codes=32, w_scales=7, out=5, bias=2)]

# the bf16 composed route (dequantise + dense GEMM): the smallest call that takes it
COMPOSED_SHAPE = (ROWS + 1, 9, 128)
