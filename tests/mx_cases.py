"""The case tables and input builders that tests/test_mx_host.py and tests/test_gpu_mx.py share (the format: tests/mx_emul.py)."""
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
