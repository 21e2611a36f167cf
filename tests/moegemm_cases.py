"""The case tables and the numpy plan of the grouped GEMM over MXFP4 experts (k_plan_count, k_plan_fill, k_mx_experts_grouped;
DESIGN.md §32), shared by tests/test_moegemm_host.py (which closes them on the CPU) and tests/test_gpu_moegemm.py.  The generators and
the exact-case machinery are tests/moe_cases.py's and tests/mx_emul.py's, by import.

The constants the edges follow (csrc/moegemm_kernels.hip): a workgroup takes R = ROW_TILE listed pairs of one expert against
C = TILE_N weight rows; its 8 waves take k-steps of 128 k in turn; the plan kernels scan the ids 256 per step (count) and 1024 per
step (fill)."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _moegemm_native as gn
from tests import moe_cases

R, C = gn.ROW_TILE, gn.TILE_N
X16, DTYPES = moe_cases.X16, moe_cases.DTYPES
to_dtype = moe_cases.to_dtype
EDGE_COUNTS = (0, 1, R - 1, R, R + 1, 2 * R + 1)


def name16(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f16"


def plan_text(E, P):
    return f"mx_plan E{E} P{P} R{R}"


def experts_text(x_dtype, per_slot, E, P):
    return f"mx_grouped {name16(x_dtype)} {'slot' if per_slot else 'shared'} E{E} P{P} R{R}"


def glu_text(x_dtype, E, P):
    return f"mx_grouped_glu {name16(x_dtype)} E{E} P{P} R{R}"


def down_text(h_dtype, E, P, A):
    return f"mx_grouped_down_sum {name16(h_dtype)} E{E} P{P} R{R} A{A}"


# ---------------------------------------------------------------- the plan
def max_tiles(P, E, r=R):
    return min(E, P) + P // r


def plan_words(P, E, r=R):
    return E + 2 + 3 * max_tiles(P, E, r) + P


def plan_bytes(P, E, r=R):
    return -(-4 * plan_words(P, E, r) // 256) * 256


def plan_reference(ids, E, r=R):
    """ids: any integer array, read flat as int32 -> dict(counts [E], n_tiles, n_listed, tiles [n_tiles, 3], sorted [P]), the
    plan of include/mbnb_moegemm.h integer for integer: a function of the ids alone"""
    flat = np.asarray(ids).reshape(-1).astype(np.int64)
    inside = (flat >= 0) & (flat < E)
    counts = np.bincount(flat[inside], minlength=E).astype(np.int64)
    order = [np.nonzero(flat == e)[0] for e in range(E)] + [np.nonzero(~inside)[0]]      # np.nonzero ascends
    tiles, first = [], 0
    for e in range(E):
        for t in range(-(-int(counts[e]) // r)):
            tiles.append((e, first + t * r, min(r, int(counts[e]) - t * r)))
        first += int(counts[e])
    return dict(counts=counts.astype(np.int32), n_tiles=len(tiles), n_listed=int(inside.sum()),
                tiles=np.array(tiles, dtype=np.int32).reshape(-1, 3), sorted=np.concatenate(order).astype(np.int32))


def plan_from_words(words, P, E, r=R):
    """The int32 words a launch wrote -> the dict of plan_reference (the tile entries past n_tiles are not part of it)"""
    words = np.asarray(words).reshape(-1)
    n_tiles, n_listed = int(words[E]), int(words[E + 1])
    tiles = words[E + 2:E + 2 + 3 * max_tiles(P, E, r)].reshape(-1, 3)
    start = E + 2 + 3 * max_tiles(P, E, r)
    return dict(counts=words[:E].copy(), n_tiles=n_tiles, n_listed=n_listed, tiles=tiles[:max(0, n_tiles)].copy(), sorted=words[start:start + P].copy())


def same_plan(a, b):
    return (a["n_tiles"] == b["n_tiles"] and a["n_listed"] == b["n_listed"]
            and all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)) for k in ("counts", "tiles", "sorted")))


def _i32(v):
    return int(np.int64(v).astype(np.int32))


def _from_counts(counts, outside, seed):
    """ids with expert e on counts[e] pairs and the `outside` values once each, at seeded random places"""
    flat = np.concatenate([np.repeat(np.arange(len(counts)), counts), np.array([_i32(v) for v in outside], dtype=np.int64)])
    return np.random.default_rng(seed).permutation(flat).astype(np.int32)


def _sparse(E, **at):
    counts = [0] * E
    for k, v in at.items():
        counts[int(k[1:])] = v
    return tuple(counts)


# (E, ids): P of 1, 63, 64, 65, 1024, 1025, 2049; E of 1, 2, 5, 9, 128, 1024; counts of 0, 1, R - 1, R, R + 1, 2 R + 1 in one call;
# all pairs on one expert; every id outside [0, E); the ids -1, E, 2^31 - 1 and -2^31
def plan_cases():
    out = [
        (1, np.zeros(1, dtype=np.int32)),
        (2, _from_counts((31, 32), (), 1)),
        (5, _from_counts((0, 64, 0, 0, 0), (), 2)),                                    # all pairs on one expert, P = R
        (9, _from_counts((0, 1, R - 1, R, R + 1, 2 * R + 1, 0, 3, 0), (), 3)),
        (9, _from_counts((0, 1, R - 1, R, R + 1, 2 * R + 1, 0, 3, 0), (-1, 9, 2 ** 31 - 1, -2 ** 31), 4)),
        (2, _from_counts((65, 0), (), 5)),
        (128, _from_counts(_sparse(128, e0=1, e63=R, e64=R + 1, e127=1024 - 2 * R - 2), (), 6)),         # P = 1024
        (128, np.random.default_rng(7).integers(0, 128, size=1025).astype(np.int32)),
        (1024, _from_counts(_sparse(1024, e0=3, e1=1, e511=R, e1022=2 * R + 1, e1023=1025 - 3 * R - 5), (), 8)),
        (1024, np.random.default_rng(9).integers(-3, 1027, size=2049).astype(np.int32)),
        (5, np.random.default_rng(10).integers(0, 5, size=2049).astype(np.int32)),
        (5, np.full(2049, 3, dtype=np.int32)),                                         # all pairs on one expert, 33 tiles
        (1, np.zeros(63, dtype=np.int32)),
    ]
    for v in (-1, None, 2 ** 31 - 1, -2 ** 31):                                        # every id outside: None stands for E
        out.append((9, np.full(70, _i32(9 if v is None else v), dtype=np.int32)))
    return out


# ---------------------------------------------------------------- exact cases
# (E, N, K, T, A, pairs per expert, x dtype, out dtype, bias, per-slot input), as tests/moe_cases.py's.  N of 1, 15, 16, 17, C - 1,
# C, C + 1, 2 C + 1; K of one block, two, a k-step minus / exactly / plus one block, a round plus a block, two rounds plus a block;
# both row dtypes into all three output dtypes; counts on the edges of the row tile.
EXACT_CASES = [
    (5, 1, 32, 35, 4, (0, 1, R - 1, R, 12), torch.bfloat16, torch.float32, True, False),
    (2, 15, 64, 65, 2, (R + 1, R + 1), torch.float16, torch.bfloat16, False, True),
    (3, 16, 96, 66, 3, (2 * R + 1, R, 5), torch.bfloat16, torch.float16, True, True),
    (9, 17, 128, 41, 2, (33, 0, 1, 15, 16, 17, 0, 0, 0), torch.float16, torch.float32, False, False),
    (2, C - 1, 160, 35, 2, (37, 33), torch.bfloat16, torch.bfloat16, True, False),
    (1, C, 1056, 5, 4, (20,), torch.float16, torch.float16, False, True),
    (2, C + 1, 2080, 35, 2, (R + 5, 1), torch.bfloat16, torch.float32, True, False),
    (3, 2 * C + 1, 64, 22, 3, (R + 2, 0, 0), torch.float16, torch.bfloat16, False, False),       # all pairs on one expert
]
exact_operands = moe_cases.exact_operands
quantize_experts = moe_cases.quantize_experts

# ---------------------------------------------------------------- the bit rule on random data
# (N, K) of the weights, E = 9; P = T x A of 70, 1200 and 2049; a uniform routing and one skewed towards expert 0
RANDOM_WEIGHTS = ((17, 2080), (33, 1056))
RANDOM_E = 9
RANDOM_PAIRS = ((35, 2), (300, 4), (683, 3))
RANDOM_ROUTINGS = ("uniform", "skewed")
RANDOM_CASES = [(nk, ta, routing) for nk in RANDOM_WEIGHTS for ta in RANDOM_PAIRS for routing in RANDOM_ROUTINGS]
YARDSTICK_MAX_PAIRS = moe_cases.MAX_PAIRS


def random_weights(nk):
    """w ~ N(0, 0.02^2) in f32 [E, N, K] (to be quantised), bias ~ N(0, 1) [E, N]"""
    N, K = nk
    g = torch.Generator().manual_seed(41000 + N)
    return torch.randn(RANDOM_E, N, K, generator=g) * 0.02, torch.randn(RANDOM_E, N, generator=g)


def random_rows(nk, ta, x_dtype, per_slot):
    (N, K), (T, A) = nk, ta
    g = torch.Generator().manual_seed(41100 + N + T + int(per_slot))
    return torch.randn((T, A, K) if per_slot else (T, K), generator=g).to(x_dtype)


def random_routing(ta, routing):
    """int32 [T, A] with a few ids outside [0, E); `skewed`: three quarters of the pairs on expert 0"""
    T, A = ta
    rng = np.random.default_rng(41200 + T + len(routing))
    ids = rng.integers(0, RANDOM_E, size=(T, A))
    if routing == "skewed":
        ids = np.where(rng.random((T, A)) < 0.75, 0, ids)
    ids[rng.random((T, A)) < 0.02] = -1
    ids[0, 0], ids[T - 1, A - 1] = RANDOM_E, 1
    return ids.astype(np.int32)


# bytes off a 16-byte boundary for x, the codes, the plan and the workspace (16-byte steps), bytes for the scales, elements for ids,
# out, bias and rw
OFFSETS = [dict(x=0, w_codes=0, w_scales=0, ids=0, out=0, bias=0, rw=0, ws=0, plan=0), dict(x=16, w_codes=32, w_scales=1, ids=1, out=1, bias=1, rw=1, ws=16, plan=48),
           dict(x=48, w_codes=16, w_scales=3, ids=3, out=3, bias=2, rw=3, ws=32, plan=16), dict(x=32, w_codes=48, w_scales=2, ids=2, out=5, bias=3, rw=2, ws=48, plan=32)]

# the Python surface: more pairs than one call of the grouped route, on a tiny N and K: T, A, E, N, K
CUT_A = 4
CUT_SHAPE_TAIL = (3, 6, 32)                                    # E, N (2 I for the gate / up form), K
# the automatic route: a pair count at a threshold the tests set (the shipped value is a measurement)
ROUTE_SHAPE = (520, 4, 5, 64, 32)                              # T, A, E, H, I: 2080 pairs
