"""The case tables and the numpy restatements of the MXFP4 mixture-of-experts MLP (k_mx_experts_rt, k_routed_sum),
shared by tests/test_moemlp_host.py (which closes them on the CPU) and tests/test_gpu_moemlp.py.  The yardstick of every GPU case is
the f32 output of mbnb_moe_mxfp4_experts (k_mx_experts), a kernel older than these, put through the chains below.

The constants the edges follow (csrc/moemlp_kernels.hip): a workgroup owns TILE = 16 weight rows of one expert, 8 (gate, up) pairs
of the gate / up launch; it scans the ids 64 per wave-step (SCAN) and walks the presence bytes 64 experts per step; it runs the
decode loop once per ROWS = 16 listed pairs; the grid has R = min(E, P) rows."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _moemlp_native as mlpn
from tests import moe_cases, mx_emul as emul, optim_emul

TILE, ROWS, SCAN = mlpn.TILE_N, mlpn.ROWS, 64
MAX_PAIRS, MAX_EXPERTS = mlpn.MAX_PAIRS, mlpn.MAX_EXPERTS
X16 = moe_cases.X16
DTYPES = moe_cases.DTYPES
to_dtype = moe_cases.to_dtype
F32 = np.float32
INF = float("inf")
ALPHA, LIMIT = 1.702, 7.0
EDGE_COUNTS = moe_cases.EDGE_COUNTS                           # pairs of one expert: 0, 1, 15, 16, 17, 33
_ERR = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def glu_text(x_dtype, E, P):
    return f"mx_glu {'bf16' if x_dtype == torch.bfloat16 else 'f16'} E{E} P{P} R{min(E, P)}"


def down_text(h_dtype, E, P, A):
    return f"mx_down_sum {'bf16' if h_dtype == torch.bfloat16 else 'f16'} E{E} P{P} R{min(E, P)} A{A}"


# ---------------------------------------------------------------- the chains
def split(pre):
    """pre [P, 2I] -> (gate [P, I], up [P, I]): row 2j of the weight is gate j, row 2j + 1 is up j"""
    return pre[:, 0::2], pre[:, 1::2]


def glu_f32(g, u, alpha, limit):
    """The kernel's chain in numpy f32, every operation rounded on its own.  With alpha = 0 every step is a correctly rounded IEEE
    operation (exp(+-0) is exactly 1), so the result is the kernel's bit for bit; otherwise numpy's expf stands in for OCML's."""
    g, u, alpha, limit = np.asarray(g, dtype=F32), np.asarray(u, dtype=F32), F32(alpha), F32(limit)
    with np.errstate(**_ERR):
        g = np.where(g > limit, limit, g)
        u = np.where(u > limit, limit, np.where(u < -limit, -limit, u))
        t = (alpha * g).astype(F32)
        den = (F32(1) + np.exp(-t).astype(F32)).astype(F32)
        sig = (F32(1) / den).astype(F32)
        gs = (g * sig).astype(F32)
        up = (u + F32(1)).astype(F32)
        return (up * gs).astype(F32)


def glu_f64(g, u, alpha, limit):
    """The same chain in float64 over f32 inputs; alpha is the f32 argument the kernel receives"""
    g, u, alpha = np.asarray(g, dtype=np.float64), np.asarray(u, dtype=np.float64), float(F32(alpha))
    with np.errstate(**_ERR):
        g = np.where(g > limit, limit, g)
        u = np.where(u > limit, limit, np.where(u < -limit, -limit, u))
        return (u + 1.0) * (g * (1.0 / (1.0 + np.exp(-(alpha * g)))))


def glu_f64_rounded_per_operation(g, u, limit):
    """alpha = 0 in float64 with a rounding to f32 after every operation: what the f32 chain must equal"""
    r = lambda v: np.asarray(v, dtype=np.float64).astype(F32).astype(np.float64)
    g, u = r(g), r(u)
    with np.errstate(**_ERR):
        g = np.where(g > limit, limit, g)
        u = np.where(u > limit, limit, np.where(u < -limit, -limit, u))
        t = r(0.0 * g)
        den = r(1.0 + r(np.exp(-t)))
        return r(r(u + 1.0) * r(g * r(1.0 / den))).astype(F32)


def glu_tol(r):
    """2^-16 |r| + 2^-118.  Derived, not measured: the rounding of alpha * g enters exp scaled by |alpha * g| <= 88.73, below
    2^-17.5 relative; seven further roundings of at most 2^-23 each leave the total under 2^-17, doubled as the margin.  Where expf
    leaves the f32 range the kernel gives 0 and the true value is at most (88.73 / alpha) * 2^-128 * (limit + 1) < 2^-118."""
    return 2.0 ** -16 * np.abs(r) + 2.0 ** -118


def round_direct(v, dtype):
    """float64 -> the value of `dtype` nearest to it (ties to even), as float64: ONE rounding, no detour through f32"""
    v = np.asarray(v, dtype=np.float64)
    if dtype == torch.float32:
        with np.errstate(**_ERR):
            return v.astype(F32).astype(np.float64)
    p, emin, top = (8, -126, (2.0 - 2.0 ** -7) * 2.0 ** 127) if dtype == torch.bfloat16 else (11, -14, 65504.0)
    with np.errstate(**_ERR):
        _, e = np.frexp(v)                                     # |v| in [2^(e - 1), 2^e)
        q = np.ldexp(1.0, np.maximum(e, emin + 1) - p)         # the spacing of dtype at v
        out = np.rint(v / q) * q
        return np.where(np.abs(out) > top, np.sign(v) * np.inf, out)


def within_glu_bound(y, r, dtype):
    """(ok, lo, hi): round(r - tol) <= y <= round(r + tol) elementwise; y float64 values of `dtype`, r the float64 chain"""
    tol = glu_tol(r)
    lo, hi = round_direct(r - tol, dtype), round_direct(r + tol, dtype)
    return (y >= lo) & (y <= hi), lo, hi


def routed_sum_f32(y, rw, ids, E):
    """y f32 [T * A, N], rw f32 [T, A], ids [T, A] -> f32 [T, N]: acc = fmaf(rw[t, a], y[t * A + a], acc) from +0.0 in slot order,
    the slots whose id is outside [0, E) skipped (optim_emul.fma: one rounding)"""
    T, A = ids.shape
    y = np.asarray(y, dtype=F32).reshape(T, A, -1)
    acc = np.zeros((T, y.shape[2]), dtype=F32)
    for a in range(A):
        live = (ids[:, a] >= 0) & (ids[:, a] < E)
        if live.any():
            acc[live] = optim_emul.fma(np.asarray(rw, dtype=F32)[live, a][:, None], y[live, a], acc[live])
    return acc


# ---------------------------------------------------------------- routings
def _sparse(E, **at):
    counts = [0] * E
    for e, c in at.items():
        counts[int(e[1:])] = c
    return tuple(counts)


ids_from_counts = moe_cases.ids_from_counts
quantize_experts = moe_cases.quantize_experts

# (E, I, K, T, A, pairs per expert, x dtype, out dtype, bias, limit).  E of 1, 2, 5, 9; I on both sides of the 8-output tile; K of
# one block, two, a k-step plus a block, a round plus a block, two rounds plus a block; single experts with 0, 1, 15, 16, 17 and 33
# pairs inside one call; P of 1, 63, 64, 65 and MAX_PAIRS; one distinct expert, distinct = min(E, P) with E < P and with E > P, the
# highest and the lowest expert only; MAX_EXPERTS experts at I = 1, K = 32.
GLU_CASES = [
    (9, 17, 160, 41, 2, (33, 0, 1, 15, 16, 17, 0, 0, 0), torch.bfloat16, torch.bfloat16, True, LIMIT),
    (9, 9, 64, 41, 2, (0, 17, 16, 0, 15, 1, 0, 33, 0), torch.float16, torch.float32, False, INF),
    (1, 1, 32, 1, 1, (1,), torch.bfloat16, torch.float16, True, LIMIT),
    (2, 7, 64, 63, 1, (31, 32), torch.float16, torch.bfloat16, False, LIMIT),                 # distinct = E < P
    (5, 8, 1056, 16, 4, (17, 15, 16, 0, 16), torch.bfloat16, torch.float32, True, INF),
    (5, 17, 2080, 13, 5, (1, 33, 15, 16, 0), torch.float16, torch.float16, True, LIMIT),
    (2, 1, 32, MAX_PAIRS // 4, 4, (MAX_PAIRS - 24, 24), torch.bfloat16, torch.bfloat16, False, INF),
    (9, 8, 32, 3, 3, (1,) * 9, torch.bfloat16, torch.float16, False, LIMIT),                  # every pair on a different expert
    (9, 7, 160, 2, 2, (1, 0, 1, 0, 0, 1, 0, 0, 1), torch.float16, torch.float32, True, LIMIT),  # distinct = P < E
    (5, 9, 64, 4, 2, (0, 0, 0, 0, 8), torch.float16, torch.bfloat16, True, INF),              # the highest expert only
    (5, 8, 160, 4, 2, (8, 0, 0, 0, 0), torch.bfloat16, torch.float32, False, LIMIT),          # the lowest expert only
    (MAX_EXPERTS, 1, 32, 8, 4, _sparse(MAX_EXPERTS, e0=3, e63=1, e64=17, e65=2, e511=1, e960=7, e1023=1), torch.float16, torch.float16, True, LIMIT),
]


def glu_operands(case, index):
    """(x float64 [T, K], w float64 [E, 2I, K], bias float64 [E, 2I] or None, ids int32 [T, A]): lossless rows scaled by 2^-3 (still
    exact in both 16-bit types) so that the pre-activations fall on both sides of +-limit; a bias of small integers"""
    E, I, K, T, A, counts, _, _, has_bias, _ = case
    x = emul.lossless(T, K, seed=31000 + 2 * index) * 0.125
    w = emul.lossless(E * 2 * I, K, seed=31001 + 2 * index).reshape(E, 2 * I, K)
    bias = np.random.default_rng(33000 + index).integers(-8, 9, size=(E, 2 * I)).astype(np.float64) if has_bias else None
    return x, w, bias, ids_from_counts(counts, T, A, seed=34000 + index)


# (E, N, K, T, A, pairs per expert, h dtype, out dtype, bias, rw dtype).  A of 1, 2, 4, 8; N on both sides of the tile; the E, K and
# pair-count edges of GLU_CASES.
SUM_CASES = [
    (9, 17, 160, 41, 2, (33, 0, 1, 15, 16, 17, 0, 0, 0), torch.bfloat16, torch.bfloat16, True, torch.float32),
    (9, 33, 64, 82, 1, (0, 17, 16, 0, 15, 1, 0, 33, 0), torch.float16, torch.float32, False, torch.bfloat16),
    (1, 1, 32, 1, 1, (1,), torch.bfloat16, torch.float16, True, torch.float16),
    (2, 15, 64, 63, 1, (31, 32), torch.float16, torch.bfloat16, False, torch.float32),
    (5, 16, 1056, 16, 4, (17, 15, 16, 0, 16), torch.bfloat16, torch.float32, True, torch.bfloat16),
    (5, 17, 2080, 13, 5, (1, 33, 15, 16, 0), torch.float16, torch.float16, True, torch.float16),
    (2, 5, 32, MAX_PAIRS // 8, 8, (MAX_PAIRS - 24, 24), torch.bfloat16, torch.bfloat16, False, torch.float32),
    (9, 16, 32, 3, 3, (1,) * 9, torch.bfloat16, torch.float16, False, torch.bfloat16),
    (9, 15, 160, 2, 2, (1, 0, 1, 0, 0, 1, 0, 0, 1), torch.float16, torch.float32, True, torch.float16),
    (5, 33, 64, 1, 8, (0, 0, 0, 0, 8), torch.float16, torch.bfloat16, True, torch.float32),   # all slots of the token on one expert
    (5, 1, 160, 4, 2, (8, 0, 0, 0, 0), torch.bfloat16, torch.float32, False, torch.bfloat16),
    (MAX_EXPERTS, 1, 32, 8, 4, _sparse(MAX_EXPERTS, e0=3, e63=1, e64=17, e65=2, e511=1, e960=7, e1023=1), torch.float16, torch.float16, True, torch.float16),
]
RW_SPECIALS = (0.0, -1.5, INF, -INF)                          # planted at the first pairs of a case that has room for them


def sum_operands(case, index):
    """(h float64 [T, A, K], w float64 [E, N, K], bias or None, ids, rw float64 [T, A] exact in every rw dtype)"""
    E, N, K, T, A, counts, _, _, has_bias, _ = case
    h = (emul.lossless(T * A, K, seed=35000 + 2 * index) * 0.125).reshape(T, A, K)
    w = emul.lossless(E * N, K, seed=35001 + 2 * index).reshape(E, N, K)
    bias = np.random.default_rng(36000 + index).integers(-8, 9, size=(E, N)).astype(np.float64) if has_bias else None
    rw = np.random.default_rng(37000 + index).integers(-32, 33, size=(T, A)) / 64.0           # multiples of 2^-6 in [-0.5, 0.5]
    flat = rw.reshape(-1)
    if flat.size >= 2 * len(RW_SPECIALS):
        flat[1:1 + len(RW_SPECIALS)] = RW_SPECIALS
    return h, w, bias, ids_from_counts(counts, T, A, seed=38000 + index), rw


# ---------------------------------------------------------------- the bound against float64: planted pre-activations
# Zero weight codes make pre = bias exactly, so an f32 bias plants any (g, u): g at, just under and over the limit, near the
# argument -52.13 = -88.73 / alpha where expf(-(alpha g)) overflows, and a sweep of [-60, 8]; u at +-limit, their neighbours, and
# ordinary values.
PLANT_SHAPE = (4, 64, 32, 6, 2)                                # E, I, K, T, A


def planted_bias():
    E, I, K, T, A = PLANT_SHAPE
    lim = F32(LIMIT)
    edge = -88.72284 / ALPHA
    g_special = np.array([lim, np.nextafter(lim, F32(0)), np.nextafter(lim, F32(9)), 7.5, 100.0, 0.0, 1e-30, -1e-30,
                          edge, edge - 1e-3, edge + 1e-3, edge - 0.5, edge + 0.5, -52.13, -60.0, -87.0 / ALPHA, -103.0 / ALPHA], dtype=F32)
    u_special = np.array([lim, -lim, np.nextafter(lim, F32(0)), np.nextafter(lim, F32(9)), np.nextafter(-lim, F32(0)),
                          np.nextafter(-lim, F32(-9)), -1.0, np.nextafter(F32(-1), F32(0)), 0.0, 3.25, -100.0, 100.0], dtype=F32)
    rng = np.random.default_rng(39001)
    g = np.concatenate([g_special, np.linspace(-60.0, 8.0, E * I - g_special.size).astype(F32)])
    u = np.concatenate([u_special, rng.uniform(-9.0, 9.0, E * I - u_special.size).astype(F32)])
    u = u[rng.permutation(E * I)]
    bias = np.empty((E, 2 * I), dtype=F32)
    bias[:, 0::2], bias[:, 1::2] = g.reshape(E, I), u.reshape(E, I)
    return bias


def planted_ids():
    E, I, K, T, A = PLANT_SHAPE
    return (np.arange(T * A, dtype=np.int32) % E).reshape(T, A)          # every expert, so every planted (g, u), on three pairs


# ---------------------------------------------------------------- independence on random data: (T, A, E, 2I, K)
RANDOM_GLU_SHAPES = ((5, 3, 4, 34, 1056), (5, 3, 4, 18, 1056))
RANDOM_SUM_SHAPE = (16, 4, 9, 17, 2080)                        # T, A, E, N, K
random_operands = moe_cases.random_operands

# ---------------------------------------------------------------- ids outside [0, E), NaN scale bytes, non-finite activations
OUT_OF_RANGE = (-1, None, 2 ** 31 - 1, -2 ** 31)               # None stands for E
EDGE_SHAPE = (3, 9, 160, 5, 2)                                 # E, I (or N), K, T, A: 5 blocks
OUT_OF_RANGE_PLACES = ((0, 0), (2, 1), (3, 0), (4, 1))
NAN_EXPERT, NAN_OUTPUT = 1, 5
NAN_BLOCKS = (0, 2, 4)                                         # the first, a middle and the last block
X_BAD_TOKEN = 2
X_BAD_VALUES = (INF, -INF, float("nan"))
EDGE_IDS = np.array([[0, 1], [1, 2], [2, 0], [1, 1], [0, 2]], dtype=np.int32)

# bytes off a 16-byte boundary for x / h, the codes and the workspace (16-byte steps), bytes for the scales, elements for the others
OFFSETS = [dict(x=0, w_codes=0, w_scales=0, ids=0, out=0, bias=0, rw=0, ws=0), dict(x=16, w_codes=32, w_scales=1, ids=1, out=1, bias=1, rw=1, ws=16),
           dict(x=48, w_codes=16, w_scales=3, ids=3, out=3, bias=2, rw=3, ws=48), dict(x=32, w_codes=48, w_scales=2, ids=2, out=5, bias=3, rw=2, ws=32)]

CUT_SHAPE = (300, 4, 3, 32, 32)                                # the Python surface, more pairs than one call: T, A, E, I, H

# ---------------------------------------------------------------- the K walk (tests/moe_cases.py WALK_KS), both epilogues
# The routing of moe_cases.WALK_CASES: 33 pairs, counts (17, 0, 16).  GLU: I = 9 (two 8-output tiles, the second with one live
# output), the layout of GLU_CASES.  Down + sum: N = 17, the layout of SUM_CASES.
WALK_KS, WALK_NONFINITE_KS, walk_of = moe_cases.WALK_KS, moe_cases.WALK_NONFINITE_KS, moe_cases.walk_of
WALK_SEED = 100                                                # glu_operands / sum_operands(case, WALK_SEED + i)
WALK_GLU_CASES = [(3, 9, K, 11, 3, (17, 0, 16), X16[i % 2], DTYPES[i % 3], (i // 2) % 2 == 0, (LIMIT, INF)[(i // 3) % 2]) for i, K in enumerate(WALK_KS)]
WALK_SUM_CASES = [(3, 17, K, 11, 3, (17, 0, 16), X16[(i + 1) % 2], DTYPES[(i + 1) % 3], (i // 2) % 2 == 1, DTYPES[(i + 2) % 3]) for i, K in enumerate(WALK_KS)]
