"""The case tables and the numpy plan of the grouped GEMM over MXFP4 experts (k_plan_count, k_plan_fill, k_mx_experts_grouped;
DESIGN.md §32), shared by tests/test_moegemm_host.py (which closes them on the CPU) and tests/test_gpu_moegemm.py.  The generators and
the exact-case machinery are tests/moe_cases.py's and tests/mx_emul.py's, by import.

The constants the edges follow (csrc/moegemm_kernels.hip): a workgroup takes R = ROW_TILE listed pairs of one expert against
C = TILE_N weight rows; its 8 waves take k-steps of 128 k in turn; the plan kernels scan the ids 256 per step (count) and 1024 per
step (fill)."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _moegemm_native as gn
from tests import moe_cases, moemlp_cases, mx_emul as emul

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

# ---------------------------------------------------------------- the K walk (tests/moe_cases.py WALK_KS), the three forms
# E = 3 with counts (R + 1, 0, 3): expert 0 has a full row tile and a one-row tile.  Plain: N = C + 1, the layout of EXACT_CASES.
# GLU: N = C + 2 (I = C / 2 + 1), the layout of moemlp_cases.GLU_CASES.  Down + sum: N = C + 1, the layout of moemlp_cases.SUM_CASES.
# Every one has a second column tile of one live column (plain, down) or one live (gate, up) pair (GLU).
WALK_KS, WALK_NONFINITE_KS, walk_of = moe_cases.WALK_KS, moe_cases.WALK_NONFINITE_KS, moe_cases.walk_of
WALK_SEED = 200                                                # the operands of case i: seeds WALK_SEED + i of the generators
_WALK_T, _WALK_A, _WALK_COUNTS = 17, 4, (R + 1, 0, 3)
WALK_CASES = [(3, C + 1, K, _WALK_T, _WALK_A, _WALK_COUNTS, X16[i % 2], DTYPES[i % 3], (i // 2) % 2 == 0, (i // 3) % 2 == 1) for i, K in enumerate(WALK_KS)]
WALK_GLU_CASES = [(3, C // 2 + 1, K, _WALK_T, _WALK_A, _WALK_COUNTS, X16[(i + 1) % 2], DTYPES[(i + 1) % 3], (i // 2) % 2 == 1, (moemlp_cases.LIMIT, moemlp_cases.INF)[(i // 3) % 2])
                  for i, K in enumerate(WALK_KS)]
WALK_SUM_CASES = [(3, C + 1, K, _WALK_T, _WALK_A, _WALK_COUNTS, X16[i % 2], DTYPES[(i + 2) % 3], (i // 2) % 2 == 0, DTYPES[(i + 1) % 3]) for i, K in enumerate(WALK_KS)]
glu_operands, sum_operands = moemlp_cases.glu_operands, moemlp_cases.sum_operands

# the bit rule at the model's K and at a tail on wave 7: (N, K) of the weights, E = RANDOM_E, P = 70, the uniform routing
WALK_RANDOM_WEIGHTS = ((17, 2880), (C + 1, 992))
WALK_RANDOM_PAIRS = RANDOM_PAIRS[0]

# ---------------------------------------------------------------- past one column tile in the GLU and down forms: K = 160
# (form, N): N on either side of the column tile and past two of them; for GLU that is I = 23, 24, 25, 49: both parities of I, and
# the tile edge on either side of a (gate, up) pair.  One routing: counts on the row-tile edges, a last expert that pads the call
# to T x A, and the four ids outside [0, E).
TILE_K = 160
TILE_CASES = [("glu", n) for n in (C - 2, C, C + 2, 2 * C + 2)] + [("down", n) for n in (C - 1, C, C + 1, 2 * C + 1)]
TILE_E, TILE_T, TILE_A = 6, 50, 4
TILE_COUNTS = (0, 1, R - 1, R, R + 1, 3)
TILE_ALL_OUTSIDE = (("glu", 2 * C + 2), ("plain", 2 * C + 1), ("down", 2 * C + 1))


def tile_ids():
    """int32 [TILE_T, TILE_A]: TILE_COUNTS and moe_cases.OUT_OF_RANGE's four ids (E standing for its E) at seeded places"""
    outside = tuple(TILE_E if v == moe_cases.IDS_SHAPE[0] else v for v in moe_cases.OUT_OF_RANGE)
    return _from_counts(TILE_COUNTS, outside, 44000).reshape(TILE_T, TILE_A)


def tile_operands(form, N):
    """(rows float64: x [T, K] for GLU, h [T, A, K] otherwise; w float64 [E, N, K]; bias float64 [E, N], never zero, four times as
    wide for GLU so that the pre-activations lie on both sides of the limit; ids; rw float64 [T, A])"""
    T, A, E, K = TILE_T, TILE_A, TILE_E, TILE_K
    rows = emul.lossless(T if form == "glu" else T * A, K, seed=44100 + N) * 0.125
    w = emul.lossless(E * N, K, seed=44200 + N).reshape(E, N, K)
    rng = np.random.default_rng(44300 + N)
    bias = rng.integers(1, 9, size=(E, N)).astype(np.float64) * rng.choice((-1.0, 1.0), size=(E, N))
    rw = np.random.default_rng(44400 + N).integers(1, 33, size=(T, A)) / 64.0
    return (rows if form == "glu" else rows.reshape(T, A, K)), w, bias * (4.0 if form == "glu" else 1.0), tile_ids(), rw


# ---------------------------------------------------------------- many experts, the three forms: (E, N, K, T, A, counts)
# moemlp_cases' MAX_EXPERTS row mirrored: sparse counts that include the lowest and the highest expert.  The GLU form needs an even
# N: it runs at N + 1 (E = 128: C + 2, past the column tile by one pair; MAX_EXPERTS: I = 1).
MANY_CASES = [
    (128, C + 1, 64, 40, 4, _sparse(128, e0=3, e1=1, e63=R + 1, e64=R, e126=2, e127=160 - 2 * R - 7)),
    (gn.MAX_EXPERTS, 1, 32, 8, 4, _sparse(gn.MAX_EXPERTS, e0=3, e63=1, e64=17, e65=2, e511=1, e960=7, e1023=1)),
]


def many_operands(case, index, form):
    """(rows, w [E, N or N + 1, K], bias, ids, rw): lossless, the layout of tile_operands"""
    E, N, K, T, A, counts = case
    n = N + 1 if form == "glu" else N
    rows = emul.lossless(T if form == "glu" else T * A, K, seed=45000 + 8 * index) * 0.125
    w = emul.lossless(E * n, K, seed=45001 + 8 * index + len(form)).reshape(E, n, K)
    bias = np.random.default_rng(45002 + 8 * index).integers(1, 9, size=(E, n)).astype(np.float64)
    rw = np.random.default_rng(45003 + 8 * index).integers(1, 33, size=(T, A)) / 64.0
    return (rows if form == "glu" else rows.reshape(T, A, K)), w, bias, moe_cases.ids_from_counts(counts, T, A, seed=45004 + index), rw


# ---------------------------------------------------------------- the references of the three forms, and the kernel restated
def same_values(a, b):
    """NaN in the same places, the same values elsewhere"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((np.isnan(a) == np.isnan(b)).all()) and bool((a[~np.isnan(a)] == b[~np.isnan(b)]).all())


def reference(form, x, codes, scales, ids, bias, alpha=0.0, limit=moemlp_cases.INF, rw=None):
    """float64 over moe_cases.decode_experts, then the form's own chain in f32: `plain` float64 [P, N]; `glu` f32 [P, N / 2]
    (moemlp_cases.glu_f32 over the pre-activations rounded once to f32; the rows of the pairs outside [0, E): +0.0); `down` f32
    [T, N] (moemlp_cases.routed_sum_f32 over the same)"""
    E = codes.shape[0]
    pre = moe_cases.reference_f64(x, moe_cases.decode_experts(codes, scales), bias, ids)
    if form == "plain":
        return pre
    with np.errstate(over="ignore", invalid="ignore"):
        pre32 = pre.astype(np.float32)
    if form == "down":
        return moemlp_cases.routed_sum_f32(pre32, rw, ids, E)
    flat = ids.reshape(-1)
    h = moemlp_cases.glu_f32(*moemlp_cases.split(pre32), alpha, limit)
    h[(flat < 0) | (flat >= E)] = 0.0
    return h


MUTANTS = ("steps_floor", "tail_keeps_x_and_scale", "tail_keeps_w", "tail_only_wave_idle", "glu_column_forgets_n0", "zeros_on_column_tile_0",
           "workspace_stride_of_a_tile", "tail_past_wave_1", "three_passes")
ZERO_THREADS = 512                                             # of the workgroup: ZERO_THREADS // columns rows of +0.0 per pass


def grouped_as_kernel(x, codes, scales, ids, bias, form, mutate=None, alpha=0.0, limit=moemlp_cases.INF, rw=None):
    """reference() restated along k_mx_experts_grouped's structure (csrc/moegemm_kernels.hip): the plan's tiles of R listed pairs
    against column tiles of C weight rows; per workgroup the k-steps of four blocks dealt to eight waves, the blocks of the last
    step that lie past K read from the clamped block and zeroed (activation, weight) or set to 2^0 (scale); the eight partial sums
    added from +0.0 in wave order; the three epilogues with their column arithmetic, and the rows of +0.0.  An output element no
    workgroup wrote is NaN here.  Unmutated it equals reference() on every exact table (tests/test_moegemm_host.py).  `mutate`:
      "steps_floor"                 steps = KB // 4: the ragged last step is dropped
      "tail_keeps_x_and_scale"      the blocks past K keep the clamped block's activation and scale byte
      "tail_keeps_w"                the weight dwords of the lane groups with 4 c + g >= KB are not zeroed
      "tail_only_wave_idle"         a wave whose only step is the ragged last step does nothing
      "glu_column_forgets_n0"       the GLU store column is (16 j + fr) / 2, without n0 / 2
      "zeros_on_column_tile_0"      the rows of +0.0 are written by the workgroups of column tile 0 only
      "workspace_stride_of_a_tile"  the workspace row stride is the width of column tile 0, min(N, C), in place of N
      "tail_past_wave_1"            the ragged last step is dropped when it falls on a wave past wave 1
      "three_passes"                a wave takes at most three steps"""
    assert mutate is None or mutate in MUTANTS, mutate
    T, A = ids.shape
    P, (E, N, _), K = T * A, codes.shape, x.shape[-1]
    KB, glu = K // 32, form == "glu"
    rows = moe_cases.pair_rows(np.asarray(x, dtype=np.float64), A)
    c4 = emul.unpack(codes.reshape(E * N, -1), "fp4").astype(np.int64)
    wval = np.where(c4 & 8, -emul.FP4_GRID[c4 & 7], emul.FP4_GRID[c4 & 7]).reshape(E, N, K)
    sbytes = np.asarray(scales, dtype=np.int64)
    plan = plan_reference(ids, E)
    tiles, order, n_tiles, n_listed, mt = plan["tiles"], plan["sorted"], plan["n_tiles"], plan["n_listed"], max_tiles(P, E)
    width = N // 2 if glu else N
    stride = min(N, C) if mutate == "workspace_stride_of_a_tile" else N
    out = np.full(P * max(width, C), np.nan)                   # flat; the first P * width elements are the output (or the workspace)
    whole = -(-KB // 4)
    steps = KB // 4 if mutate == "steps_floor" else whole
    ragged = whole - 1 if KB % 4 else -1                       # the index of the ragged last step
    with np.errstate(invalid="ignore", over="ignore"):
        for tile in range(mt):
            for n0 in range(0, N, C):
                if form != "down" and not (mutate == "zeros_on_column_tile_0" and n0):
                    zcols = C // 2 if glu else C
                    zrows = ZERO_THREADS // zcols
                    cols = (n0 // 2 if glu else n0) + np.arange(zcols)
                    cols = cols[cols < width]
                    for r in range(zrows):
                        for i in range(n_listed + tile * zrows + r, P, mt * zrows):
                            out[order[i] * width + cols] = 0.0
                if tile >= n_tiles:
                    continue
                e, first, count = (int(v) for v in tiles[tile])
                pairs = order[first:first + count].astype(np.int64)
                ncols = min(C, N - n0)
                xr, wv, sv = rows[pairs], wval[e, n0:n0 + ncols], sbytes[e, n0:n0 + ncols]
                acc, ff = np.zeros((8, count, ncols)), np.zeros(ncols, dtype=bool)
                for c in range(steps):
                    wave = c % 8
                    if c == ragged and ((mutate == "tail_only_wave_idle" and c < 8) or (mutate == "tail_past_wave_1" and wave > 1)):
                        continue
                    if mutate == "three_passes" and c // 8 >= 3:
                        continue
                    for q in range(4):
                        inside = 4 * c + q < KB
                        b = 4 * c + q if inside else KB - 1
                        xq, wq, byte = xr[:, 32 * b:32 * b + 32], wv[:, 32 * b:32 * b + 32], sv[:, b]
                        if not inside:
                            if mutate != "tail_keeps_x_and_scale":
                                xq, byte = np.zeros_like(xq), np.full_like(byte, 127)
                            if mutate != "tail_keeps_w":
                                wq = np.zeros_like(wq)
                        ff |= byte == 255
                        d = xq @ wq.T if np.isfinite(xq).all() else (xq[:, None, :] * wq[None, :, :]).sum(axis=2)
                        acc[wave] += d * np.ldexp(1.0, np.where(byte == 255, 127, byte) - 127)[None, :]       # one FMA by the scale per block
                total = np.zeros((count, ncols))
                for wave in range(8):
                    total = total + acc[wave]
                pre = total if bias is None else total + np.asarray(bias, dtype=np.float64)[e, n0:n0 + ncols][None, :]
                pre = np.where(ff[None, :], np.nan, pre)
                if glu:                                            # ncols is even: (gate, up) pairs never straddle a column tile
                    pre32 = pre.astype(np.float32)
                    h = moemlp_cases.glu_f32(pre32[:, 0::2], pre32[:, 1::2], alpha, limit)
                    col = (0 if mutate == "glu_column_forgets_n0" else n0 // 2) + np.arange(ncols // 2)
                    out[pairs[:, None] * width + col[None, :]] = h
                else:
                    out[pairs[:, None] * (stride if form == "down" else width) + (n0 + np.arange(ncols))[None, :]] = pre
    res = out[:P * width].reshape(P, width)
    if form == "plain":
        return res
    if glu:
        return res.astype(np.float32)
    return moemlp_cases.routed_sum_f32(res.astype(np.float32), rw, ids, E)


# the Python surface: more pairs than one call of the grouped route, on a tiny N and K: T, A, E, N, K
CUT_A = 4
CUT_SHAPE_TAIL = (3, 6, 32)                                    # E, N (2 I for the gate / up form), K
# the automatic route: a pair count at a threshold the tests set (the shipped value is a measurement)
ROUTE_SHAPE = (520, 4, 5, 64, 32)                              # T, A, E, H, I: 2080 pairs
