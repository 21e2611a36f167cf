"""The case tables of the MXFP4 expert linears (k_mx_experts), shared by tests/test_moe_host.py (which closes them on
the CPU) and tests/test_gpu_moe.py.  The format and the generators: tests/mx_emul.py.  The yardstick of every exact case is float64
over emul.decode_f64 per expert, `+ bias`, rounded once with mx_cases.to_dtype.

The constants the edges follow (csrc/moe_kernels.hip): a workgroup owns TILE = 16 weight rows of one expert; it scans the ids 64 per
wave-step (SCAN), lists the pairs routed to its expert and runs the decode loop once per ROWS = 16 listed pairs; its 8 waves take
k-steps of STEP = 128 k in turn and request two rounds (ROUND = 1024 k) at a time; one launch takes MAX_PAIRS pairs."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _moe_native as moen
from tests import mx_cases, mx_decode_cases, mx_emul as emul

TILE, ROWS, SCAN, STEP, ROUND = moen.TILE_N, moen.ROWS, 64, 128, 1024
MAX_PAIRS = moen.MAX_PAIRS
X16 = (torch.bfloat16, torch.float16)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
to_dtype = mx_cases.to_dtype
EDGE_COUNTS = (0, 1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1)          # pairs of one expert: the edges of the 16-row passes


def launch_text(x_dtype, per_slot, E, P):
    return f"mx_experts {'bf16' if x_dtype == torch.bfloat16 else 'f16'} {'slot' if per_slot else 'shared'} E{E} P{P}"


def ids_from_counts(counts, T, A, seed):
    """int32 [T, A]: expert e on exactly counts[e] pairs, at seeded random places"""
    flat = np.repeat(np.arange(len(counts)), counts)
    assert flat.size == T * A, (counts, T, A)
    return np.random.default_rng(seed).permutation(flat).astype(np.int32).reshape(T, A)


# ---------------------------------------------------------------- exact cases
# (E, N, K, T, A, pairs per expert, x dtype, out dtype, bias, per-slot input).  E of 1, 2, 5, 9; N on both sides of the tile;
# K of one block, two, a k-step minus / exactly / plus one block, a round plus a block, two rounds plus a block; single experts with
# 0, 1, 15, 16, 17 and 33 pairs inside one call; P of 1, 63, 64, 65, 70 (the scan's wave-step) and MAX_PAIRS.
EXACT_CASES = [
    (9, 17, 160, 41, 2, (33, 0, 1, 15, 16, 17, 0, 0, 0), torch.bfloat16, torch.bfloat16, True, False),
    (9, 33, 96, 41, 2, (0, 17, 16, 0, 15, 1, 0, 33, 0), torch.float16, torch.float32, False, True),
    (1, 1, 32, 1, 1, (1,), torch.bfloat16, torch.float16, True, False),
    (2, 15, 64, 63, 1, (31, 32), torch.float16, torch.bfloat16, False, True),
    (5, 16, 128, 16, 4, (17, 15, 16, 0, 16), torch.bfloat16, torch.float32, True, False),
    (5, 17, 1056, 13, 5, (1, 33, 15, 16, 0), torch.float16, torch.float16, True, True),
    (2, 33, 2080, 35, 2, (37, 33), torch.bfloat16, torch.bfloat16, False, False),
    (2, 5, 32, MAX_PAIRS // 4, 4, (MAX_PAIRS - 24, 24), torch.float16, torch.float32, True, False),
    (9, 16, 64, 3, 3, (1,) * 9, torch.bfloat16, torch.float16, False, True),          # every pair on a different expert
    (5, 1, 2080, 4, 2, (0, 0, 0, 8, 0), torch.float16, torch.bfloat16, True, False),  # all pairs on one expert
    (1, 15, 1056, 5, 4, (20,), torch.bfloat16, torch.float32, False, True),           # the same expert on every slot of a token
    (5, 33, 160, 1, 4, (1, 1, 0, 1, 1), torch.float16, torch.float16, True, False),   # one token
]


def exact_operands(case, index):
    """(x float64 [T, K] or [T, A, K], w float64 [E, N, K], bias float64 [E, N] or None, ids int32 [T, A]): lossless rows, a bias of
    small integers per expert"""
    E, N, K, T, A, counts, _, _, has_bias, per_slot = case
    x = emul.lossless(T * A if per_slot else T, K, seed=21000 + 2 * index)
    x = x.reshape(T, A, K) if per_slot else x
    w = emul.lossless(E * N, K, seed=21001 + 2 * index).reshape(E, N, K)
    bias = np.random.default_rng(23000 + index).integers(-8, 9, size=(E, N)).astype(np.float64) if has_bias else None
    return x, w, bias, ids_from_counts(counts, T, A, seed=24000 + index)


def quantize_experts(w):
    """w float64 [E, N, K] -> (codes uint8 [E, N, K / 2], scale bytes uint8 [E, N, K / 32])"""
    E, N, K = w.shape
    codes, scales = emul.quantize(w.reshape(E * N, K), "fp4")
    return codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32)


def decode_experts(codes, scales):
    E, N, _ = codes.shape
    return emul.decode_f64(codes.reshape(E * N, -1), scales.reshape(E * N, -1), "fp4").reshape(E, N, -1)


def pair_rows(x, A):
    """x [T, K] or [T, A, K] -> the row of every pair, [T * A, K]"""
    return x.reshape(-1, x.shape[-1]) if x.ndim == 3 else np.repeat(x, A, axis=0)


def reference_f64(x, wdec, bias, ids):
    """The normative rule in float64 -> [T * A, N]: pair p against expert ids[p], + bias; a pair whose id is outside [0, E): +0.0"""
    E, N, _ = wdec.shape
    T, A = ids.shape
    rows, flat = pair_rows(x, A), ids.reshape(-1).astype(np.int64)
    out = np.zeros((T * A, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for e in np.unique(flat[(flat >= 0) & (flat < E)]):
            sel = flat == e
            r = (rows[sel][:, None, :] * wdec[e][None, :, :]).sum(axis=2) if not np.isfinite(rows[sel]).all() else rows[sel] @ wdec[e].T
            out[sel] = r if bias is None else r + bias[e][None, :]
    return out


# ---------------------------------------------------------------- ids outside [0, E)
IDS_SHAPE = (3, 17, 64, 6, 3)                       # E, N, K, T, A
OUT_OF_RANGE = (-1, IDS_SHAPE[0], 2 ** 31 - 1, -2 ** 31)
OUT_OF_RANGE_PLACES = ((0, 0), (2, 1), (3, 2), (5, 0))


def ids_operands():
    E, N, K, T, A = IDS_SHAPE
    x = emul.lossless(T, K, seed=25001)
    w = emul.lossless(E * N, K, seed=25002).reshape(E, N, K)
    bias = np.random.default_rng(25003).integers(1, 9, size=(E, N)).astype(np.float64)       # never zero: a bias that leaked shows
    ids = np.random.default_rng(25004).integers(0, E, size=(T, A)).astype(np.int32)
    return x, w, bias, ids


# ---------------------------------------------------------------- the bit rule on random data: (T, A, E, N, K)
RANDOM_SHAPES = ((5, 3, 4, 33, 1056), (16, 4, 9, 17, 2080))
RANDOM_CASES = [(shape, xd, od) for shape in RANDOM_SHAPES for xd, od in zip(X16, (torch.bfloat16, torch.float32))]


def random_operands(shape, x_dtype, per_slot=False):
    """x ~ N(0, 1) in x_dtype, w ~ N(0, 0.02^2) in f32 (to be quantised), bias ~ N(0, 1) in f32, ids uniform with distinct experts
    per token where E allows"""
    T, A, E, N, K = shape
    g = torch.Generator().manual_seed(26000 + T)
    x = torch.randn((T, A, K) if per_slot else (T, K), generator=g).to(x_dtype)
    w = torch.randn(E, N, K, generator=g) * 0.02
    bias = torch.randn(E, N, generator=g)
    rng = np.random.default_rng(26100 + T)
    ids = np.stack([rng.permutation(E)[:A] for _ in range(T)]).astype(np.int32)
    return x, w, bias, ids


# ---------------------------------------------------------------- NaN scale bytes and non-finite activations
NAN_SHAPE = (3, 9, 160, 5, 2)                       # E, N, K, T, A: 5 blocks
NAN_EXPERT, NAN_COLUMN = 1, 5
NAN_BLOCKS = (0, 2, 4)                              # the first, a middle and the last block
X_BAD_TOKEN = 2
X_BAD_KS = (0, 31, 32, NAN_SHAPE[2] - 1)
X_BAD_VALUES = mx_decode_cases.X_BAD_VALUES


def nan_operands():
    E, N, K, T, A = NAN_SHAPE
    x = emul.lossless(T, K, seed=27001)
    w = emul.lossless(E * N, K, seed=27002).reshape(E, N, K)
    ids = np.array([[0, 1], [1, 2], [2, 0], [1, 1], [0, 2]], dtype=np.int32)
    return x, w, ids


# ---------------------------------------------------------------- scale bytes from one end of E8M0 to the other
# emul.wide (tests/mx_decode_cases.py WIDE_T: "low" puts the weight on bytes 0 .. 4, "high" on bytes 250 .. 254) on expert 1 of
# three; expert 0 holds the same rows rolled by one, expert 2 the same rows negated, so every pair stays exact in f32 in any order.
WIDE_SHAPE = (3, 9, 2080, 5, 3)                     # E, N, K, T, A: 65 blocks, the period of t is 8, so t[0] lies on blocks 0, 32 and 64
WIDE_CASES = [(which, od) for which in ("low", "high") for od in (torch.float32, torch.bfloat16)]


def wide_operands(which):
    """(x float64 [T, K], w float64 [E, N, K], codes, scale bytes, ids, a_i, c_j)"""
    E, N, K, T, A = WIDE_SHAPE
    t, a0, c0 = mx_decode_cases.WIDE_T[which]
    x, w1, a, c = emul.wide(T, N, K, t, a0, c0, seed=28000 + len(which))
    w = np.stack([np.roll(w1, 1, axis=0), w1, -w1])
    codes, scales = mx_cases.lossless_codes_checked(w.reshape(E * N, K))
    ids = np.stack([np.random.default_rng(28100 + i).permutation(E) for i in range(T)]).astype(np.int32)
    return x, w, codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32), ids, a, c


# bytes off a 16-byte boundary for x and the codes (16-byte steps), bytes for the scales, elements for ids, out and bias
OFFSETS = [dict(x=0, w_codes=0, w_scales=0, ids=0, out=0, bias=0), dict(x=16, w_codes=32, w_scales=1, ids=1, out=1, bias=1),
           dict(x=48, w_codes=16, w_scales=3, ids=3, out=3, bias=2), dict(x=32, w_codes=48, w_scales=2, ids=2, out=5, bias=3)]

# the Python surface: more pairs than one launch
CUT_SHAPE = (300, 4, 3, 5, 32)                      # T, A, E, N, K


# ---------------------------------------------------------------- the K walk of the decode tile
# K has KB = K / 32 blocks and s = ceil(KB / 4) k-steps; step c runs on wave c % 8 in that wave's pass c // 8 (tile_walk requests two
# passes per outer iteration).  The last step, c = s - 1, holds KB - 4 (s - 1) blocks: the others of its four are read from the
# clamped address and zeroed in registers.
WALK_KS = (
    352,                     # s = 3,  last step 3 blocks, wave 2, pass 0
    448,                     # s = 4,  last step 2 blocks, wave 3, pass 0
    992,                     # s = 8,  last step 3 blocks, wave 7, pass 0
    1024,                    # s = 8,  last step whole,    wave 7, pass 0: one whole round
    1216,                    # s = 10, last step 2 blocks, wave 1, pass 1
    2016,                    # s = 16, last step 3 blocks, wave 7, pass 1
    2048,                    # s = 16, last step whole,    wave 7, pass 1: two whole rounds
    2880,                    # s = 23, last step 2 blocks, wave 6, pass 2: the model's size (gpt-oss, H = I = 2880)
    3104,                    # s = 25, last step 1 block,  wave 0, pass 3: tile_walk's second outer iteration with a live u = 1 step
)
WALK_NONFINITE_KS = (992, 2880)                     # the tail off wave 0: where the 0xFF bytes, Inf and NaN are planted on it


def walk_of(K):
    """K -> dict(steps, tail: the blocks of the last step, first: the first block of the last step, wave, passes: the pass of the last step)"""
    KB = K // 32
    steps = -(-KB // 4)
    return dict(steps=steps, tail=KB - 4 * (steps - 1), first=4 * (steps - 1), wave=(steps - 1) % 8, passes=(steps - 1) // 8)


# k_mx_experts at every K of the walk: (E, N, K, T, A, pairs per expert, x dtype, out dtype, bias, per-slot input), the layout of
# EXACT_CASES.  N = 17 is two 16-row tiles, the second with one live column; 33 pairs are three passes of the pair list.
WALK_SEED = 100                                     # exact_operands(case, WALK_SEED + i): seeds no other table uses
WALK_CASES = [(3, 17, K, 11, 3, (17, 0, 16), X16[i % 2], DTYPES[i % 3], (i // 2) % 2 == 0, (i // 3) % 2 == 1) for i, K in enumerate(WALK_KS)]


def walk_nan_blocks(K):
    """the blocks that get a 0xFF byte: the first block of the last step and block KB - 1"""
    return tuple(sorted({walk_of(K)["first"], K // 32 - 1}))


def walk_bad_ks(K):
    """the k that get an Inf or a NaN activation: the first k of the last step and K - 1"""
    return (32 * walk_of(K)["first"], K - 1)


def walk_nan_operands(K):
    """(x float64 [T, K], w float64 [E, N, K], ids) of NAN_SHAPE's E, N, T, A at a K of the walk"""
    E, N, _, T, A = NAN_SHAPE
    return emul.lossless(T, K, seed=27100 + K), emul.lossless(E * N, K, seed=27101 + K).reshape(E, N, K), nan_operands()[2]
