"""The case tables and the numpy restatement of the mixture-of-experts router (k_router), shared by
tests/test_router_host.py (which closes them on the CPU) and tests/test_gpu_router.py.

The constants the edges follow (csrc/router_kernels.hip): a lane walks the row in 16-byte chunks of 8 elements, 64 chunks (512
elements) per pass; 16 waves take the experts w, w + 16, ..., four at a time, so 64 experts per round of the workgroup; the
selecting wave holds candidate lane + 64 j on a lane."""
import numpy as np
import torch

from mps_bitsandbytes_amd import _router_native as rn

F32 = np.float32
INF = float("inf")
MAX_EXPERTS, MAX_TOPK, MAX_K = rn.MAX_EXPERTS, rn.MAX_TOPK, rn.MAX_K
X16 = (torch.float16, torch.bfloat16)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ERR = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def launch_text(dtype, E, K, A, T):
    return f"router {'bf16' if dtype == torch.bfloat16 else 'f16'} E{E} K{K} A{A} T{T}"


def to_dtype(a64, dtype):
    """float64 numpy -> a torch tensor of `dtype`; the callers pass values that are exact in it"""
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float64)).to(dtype)


# ---------------------------------------------------------------- the restatement
def rank_key(logits):
    """f32 -> uint32, order-preserving: a NaN of either sign the maximum, -0 on +0's key"""
    u = np.ascontiguousarray(logits, dtype=F32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    k = np.where(u & 0x80000000 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0xFFFFFFFF
    return k


def select(logits, A):
    """ids int32 [T, A]: descending key, the lower index first among equal keys (np.lexsort: the last key is the primary one)"""
    logits = np.asarray(logits, dtype=F32)
    T, E = logits.shape
    falling = (np.int64(0xFFFFFFFF) - rank_key(logits).astype(np.int64))
    index = np.broadcast_to(np.arange(E, dtype=np.int64), (T, E))
    return np.lexsort((index, falling), axis=-1)[:, :A].astype(np.int32)


def _chain(v, exp):
    """the softmax chain over the selected logits v f32 [T, A]; `exp` maps the f32 differences to e"""
    with np.errstate(**_ERR):
        d = (v - v[:, :1]).astype(F32)
        e = exp(d)
        s = e[:, 0].copy()
        for a in range(1, v.shape[1]):
            s = (s + e[:, a]).astype(e.dtype)
        return (e / s[:, None]).astype(e.dtype)


def emulate(logits, A):
    """(ids int32 [T, A], rw f32 [T, A]): the kernel's chain in numpy f32, every operation rounded on its own; numpy's expf stands
    in for OCML's, so rw is the kernel's bit for bit only where every exp is exact (differences of 0, or below -104: 1 and 0)."""
    logits = np.asarray(logits, dtype=F32)
    ids = select(logits, A)
    v = np.take_along_axis(logits, ids.astype(np.int64), axis=1)
    return ids, _chain(v, lambda d: np.exp(d).astype(F32))


def emulate64(logits, A):
    """(ids, rw float64): the same selection and the same f32 differences, exp, the sum and the division in float64"""
    logits = np.asarray(logits, dtype=F32)
    ids = select(logits, A)
    v = np.take_along_axis(logits, ids.astype(np.int64), axis=1)
    return ids, _chain(v, lambda d: np.exp(d.astype(np.float64)))


def weight_tol(r, A):
    """The bound on |w - r| for a weight w of the f32 chain against the float64 chain r = emulate64's.

    The differences d[a] are the same f32 values in both chains.  expf is taken at 1 ulp, the accuracy tests/moemlp_cases.py
    already rests on: e[a] carries 2^-23 relative.  s is a sum of A non-negative terms: the terms' 2^-23, plus A - 1 additions of
    2^-24 each: 2^-23 + (A - 1) 2^-24.  The division adds 2^-24.  Together 2^-23 + 2^-23 + (A - 1) 2^-24 + 2^-24 = (A + 4) 2^-24
    relative, doubled as the margin (as moemlp_cases.glu_tol is), plus an absolute floor of 2^-149 where e[a] is denormal and its
    ulp is no longer relative."""
    return 2.0 * (A + 4) * 2.0 ** -24 * np.abs(r) + 2.0 ** -149


def within_weight_bound(w, r, A):
    """elementwise: NaN exactly where r is NaN, else |w - r| <= weight_tol"""
    w, r = np.asarray(w, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(**_ERR):
        return np.where(np.isnan(r), np.isnan(w), np.abs(w - r) <= weight_tol(r, A))


def logits_f64(x, W, bias):
    """float64 [T, E] over the stored 16-bit operands (numpy float64 arrays) and the bias (or None)"""
    l = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    return l if bias is None else l + np.asarray(bias, dtype=np.float64)[None, :]


def logit_tol(x, W, bias):
    """The any-order bound of an f32 dot product of K exact products plus one add: (K + 2) 2^-24 (sum_k |x_k W_ek| + |b_e|)"""
    K = np.asarray(x).shape[1]
    mag = np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(W, dtype=np.float64)).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return (K + 2) * 2.0 ** -24 * mag


# ---------------------------------------------------------------- lossless operands
def lossless(rows, K, seed):
    """[rows, K] float64: integers in [-8, 8] times 2^-2, exact in f16 and bf16.  A product of two of them is a multiple of 2^-4 of
    magnitude at most 4, so every partial sum of up to MAX_K of them is a multiple of 2^-4 below 2^16 = 2^-4 * 2^20 < 2^-4 * 2^24:
    exact in f32 in any order."""
    return np.random.default_rng(seed).integers(-8, 9, size=(rows, K)).astype(np.float64) * 0.25


def lossless_bias(E, seed):
    """[E] float64: integers in [-32, 32] times 2^-2: exact in f16 and bf16 (at most 6 significant bits), on the products' grid"""
    return np.random.default_rng(seed).integers(-32, 33, size=E).astype(np.float64) * 0.25


# (E, K, T, A, dtype of x and W, bias dtype or None).  E on both sides of the 64 candidates of a lane pass and of the 64 experts of
# a workgroup round, and the limit; K of one chunk, two, one pass of a wave (512) minus, exactly and plus a chunk, and the user's;
# T of 1, 2, 3 and 17; A of 1, 2, 4, 8, 32 and E itself.
LOGIT_CASES = [
    (1, 8, 1, 1, torch.bfloat16, None),
    (2, 16, 2, 2, torch.float16, torch.float16),
    (63, 504, 3, 32, torch.bfloat16, torch.bfloat16),
    (64, 512, 17, 8, torch.float16, torch.float32),
    (65, 520, 2, 4, torch.bfloat16, torch.float32),
    (128, 2880, 17, 4, torch.bfloat16, torch.bfloat16),
    (1000, 16, 3, 32, torch.float16, None),
    (1024, 520, 2, 8, torch.bfloat16, torch.float16),
    (32, 2880, 1, 32, torch.float16, torch.bfloat16),
    (2, 8, 17, 1, torch.bfloat16, None),
    (17, 512, 3, 17, torch.float16, torch.float16),
]


def logit_operands(case, index):
    """(x float64 [T, K], W float64 [E, K], bias float64 [E] or None)"""
    E, K, T, A, _, bias_dtype = case
    return lossless(T, K, 41000 + 2 * index), lossless(E, K, 41001 + 2 * index), None if bias_dtype is None else lossless_bias(E, 42000 + index)


# ---------------------------------------------------------------- planted logits: a zero weight makes the logit the f32 bias, bit for bit
# (the accumulator is +0 and +0 + b = b for every b but -0, which gives +0: a -0 logit cannot leave the kernel, so the -0 == +0 rule
# is held on the restatement, and the device is shown a -0 bias beside a +0 one)
def planted(name, E=128):
    """f32 [E] biases -> (bias, A, exact): `exact` where the restatement's weights are the kernel's bit for bit"""
    b = np.zeros(E, dtype=F32)
    if name == "all-equal":
        b[:] = F32(-3.25)
        return b, 4, True
    if name == "pairs-64":                                   # e and e + 64: the same lane of the selecting wave, the next candidate
        b[:] = -np.arange(E, dtype=F32) * F32(128) - F32(1024)
        b[70], b[6] = 512, 512
        b[5], b[69] = 0, 0
        return b, 4, True
    if name == "pairs-4-and-16":                             # e + 4 and e + 16: across the wave strides of the logit phase
        b[:] = -np.arange(E, dtype=F32) * F32(128) - F32(1024)
        b[33], b[37] = 512, 512
        b[100], b[116] = 0, 0
        return b, 4, True
    if name == "zeros":                                      # +0 against -0, every other logit below
        b[:] = F32(-200)
        b[[90, 27, 91]] = F32(-0.0)
        b[[3, 64]] = F32(0.0)
        return b, 8, True
    if name == "boundary":                                   # more candidates tied at rank A - 1 than fit: the lowest indices get in
        b[:] = F32(-500)
        b[77] = F32(1.0)
        b[[120, 9, 73, 10, 64, 8]] = F32(0.5)
        return b, 4, False
    if name == "half-half":                                  # {c, c, c - 110, c - 110}
        b[:] = F32(-1000)
        b[[101, 40]] = F32(7.5)
        b[[41, 2]] = F32(7.5 - 110)
        return b, 4, True
    raise KeyError(name)


PLANTED = ("all-equal", "pairs-64", "pairs-4-and-16", "zeros", "boundary", "half-half")

# a sweep of gaps for the weight bound: slot 0 at c, the others c + g for g in [-100, 0]
SWEEP_A = 4


def gap_sweep(n=4096, seed=43000):
    """f32 [n, SWEEP_A] selected logits in descending order: v[0] = c, then gaps drawn over [-100, 0], dense near 0 and near the
    underflow of expf (-87.3 .. -103.9)"""
    rng = np.random.default_rng(seed)
    g = np.concatenate([rng.uniform(-100, 0, size=(n // 2, SWEEP_A - 1)), rng.uniform(-2, 0, size=(n // 4, SWEEP_A - 1)),
                        rng.uniform(-100, -87, size=(n - n // 2 - n // 4, SWEEP_A - 1))])
    g = -np.sort(-g, axis=1)
    c = rng.uniform(-30, 30, size=(g.shape[0], 1))
    return np.concatenate([c, c + g], axis=1).astype(F32)


# ---------------------------------------------------------------- random data at the user's shape
RANDOM_SHAPES = ((17, 2880, 32, 4), (17, 2880, 128, 4))      # T, K, E, A


def random_operands(shape, dtype, seed=44000):
    T, K, E, A = shape
    g = torch.Generator().manual_seed(seed + E)
    x = torch.randn(T, K, generator=g).to(dtype)
    W = (torch.randn(E, K, generator=g) * 0.05).to(dtype)
    bias = torch.randn(E, generator=g).to(dtype)
    return x, W, bias


# ---------------------------------------------------------------- the gap fixture: float64's top-k is the only admissible answer
GAP_SHAPE = (64, 64, 128, 4)                                 # T, K, E, A: a small K, so the logit bound is tiny
GAP_SEEDS = (45001, 45002)


def gap_operands(seed):
    T, K, E, A = GAP_SHAPE
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    W = torch.randn(E, K, generator=g).to(torch.bfloat16)
    bias = torch.randn(E, generator=g).to(torch.bfloat16)
    return x, W, bias


def gap_margins(x, W, bias, A):
    """(ids of float64's top-A [T, A], ok [T]): ok where every gap between the ranks 0 .. A of the float64 logits (the boundary
    rank A included) exceeds twice the larger logit bound of the two neighbours, so no f32 summation order can swap them"""
    xd, Wd, bd = x.double().numpy(), W.double().numpy(), bias.double().numpy()
    l, tol = logits_f64(xd, Wd, bd), logit_tol(xd, Wd, bd)
    full = np.argsort(-l, axis=1, kind="stable")
    order = full[:, :A + 1]
    top, top_tol = np.take_along_axis(l, order, axis=1), np.take_along_axis(tol, order, axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    need = 2.0 * np.maximum(top_tol[:, :-1], top_tol[:, 1:])
    # and no expert past rank A - 1, whatever its own bound, reaches rank A - 1
    rest = np.take_along_axis(l + tol, full[:, A:], axis=1).max(axis=1)
    return order[:, :A].astype(np.int32), (gaps > need).all(axis=1) & (top[:, A - 1] - top_tol[:, A - 1] > rest)


# ---------------------------------------------------------------- non-finite values
BAD_SHAPE = (5, 520, 16, 4)                                  # T, K, E, A
BAD_TOKEN = 2
BAD_K = (0, 260, 519)                                        # the first, a middle and the last k
BAD_VALUES = (float("nan"), INF, -INF)
BAD_EXPERT = 11

# bytes off a 16-byte boundary for x and w (16-byte steps), elements for the others
OFFSETS = [dict(x=0, w=0, bias=0, ids=0, rw=0, logits=0), dict(x=16, w=32, bias=1, ids=1, rw=1, logits=1),
           dict(x=48, w=16, bias=3, ids=3, rw=3, logits=2), dict(x=32, w=48, bias=2, ids=2, rw=5, logits=3)]

BLOCK_SHAPES = tuple((8, 64, 64, A, T) for A in (2, 4) for T in (1, 5))        # E, H, I, A, T
