"""
Boundary inputs of the quantisers, and plain numpy f32 restatements of their arithmetic.  Data only, importable without a GPU.

Every quantiser is equal to the reference only if the last bit of a quotient (4-bit, FP8) or of a product (int8) is right, and a wrong
last bit shows only when the value lies within one ulp of a decision boundary.  The builders below put values there, at every scale:

  scales      512 f32 mantissas in [1, 2) (1.0, the next f32 above 1, the next below 2, seeded random ones) at the exponents a dtype can
              hold (f32 / bf16: 0, -30, +40; f16: 0, -6, +8), plus the edges of the kernels' fast-path ranges and of the clamps
  4-bit       for each scale a and each midpoint t between neighbouring codes, the values of the input dtype within +-3 steps of t * a,
              in blocks that hold one element equal to a (the block's own absmax); and, for a supplied absmax, x fixed in the input
              dtype with the f32 absmax within +-3 ulps of x / t, one block per absmax
  int8        for each scale and each half-integer h = 0.5 ... 126.5 (both signs), the values within +-2 steps of h / rscale127(a);
              laid out as rows, as blocks, as the rows or the columns of a matrix, and as the absmax values of 4-bit blocks
  FP8         for each scale s (row maximum 448 s) and each boundary b of the encoder -- mantissa midpoints, powers of two with the 8
              values below them, 448 and 256 -- the values within +-3 steps of b * s

The restatements use np.float32 operations only (numpy's +, -, *, / on float32 are correctly rounded) and no shortcut: a literal argmin
whose first minimum wins, (1 / am) * 127, rint, the reference's FP8 formula with the oracle's bump table.  tests/test_rounding_host.py
holds them against the oracle on all of this data, counts the elements whose output changes when the quotient or product moves to a
neighbouring f32 (the data is sharp), and applies MUTANTS -- the ways a kernel could be subtly wrong -- to show that each changes
expected outputs here.  tests/test_gpu_rounding.py runs every kernel form on the data.
"""
import numpy as np
import torch

F32 = np.float32
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
EXPS = {"f32": (0, -30, 40), "bf16": (0, -30, 40), "f16": (0, -6, 8)}
# a block's or row's own absmax is clamped at 1e-8 (about 2^-26.6): at exponent -30 every scale becomes the clamp itself, so the builders
# of an own absmax sweep one more exponent, -20, to have small scales that are not clamped
EXPS_OWN = {"f32": (0, -30, 40, -20), "bf16": (0, -30, 40, -20), "f16": (0, -6, 8)}
CLAMP = F32(1e-8)
N_MANT = 512

NF4 = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=F32)
FP4_POS = np.array([0.0, 0.0625, 0.125, 0.25, 0.375, 0.5, 0.75, 1.0], dtype=F32)
FP4 = np.concatenate([FP4_POS, -FP4_POS]).astype(F32)
TABLE = {"nf4": NF4, "fp4": FP4}


# ----------------------------------------------------------------------------------------------- f32 as ordered integers
def up(x, n=1):
    """The f32 n steps above x (below for n < 0); x finite, no step crosses zero."""
    x = np.asarray(x, dtype=F32)
    u = x.view(np.int32).astype(np.int64)
    u = np.where(u < 0, u - n, u + n)
    return u.astype(np.int32).view(F32)


def bits(x):
    return int(np.asarray(x, dtype=F32).reshape(-1)[0].view(np.uint32))


def neighbours(centre, dt, k):
    """[..., 2k + 1] f32: the values of dtype `dt` within +-k steps of |centre| (rounded to dt), signed like centre.  centre in float64."""
    c = np.asarray(centre, dtype=np.float64)
    t = torch.as_tensor(np.abs(c)).to(DT[dt])
    iv = t.view(torch.int32 if dt == "f32" else torch.int16).to(torch.int64)
    nb = iv[..., None] + torch.arange(-k, k + 1, dtype=torch.int64)
    assert int(nb.min()) > 0
    v = nb.to(torch.int32 if dt == "f32" else torch.int16).view(DT[dt]).float().numpy()
    return (v * np.sign(c)[..., None]).astype(F32)


def in_dtype(x, dt):
    """x (f32 / f64) rounded to dtype dt, as f32."""
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(DT[dt]).float().numpy()


# ----------------------------------------------------------------------------------------------- scales
def mantissas(n=N_MANT, seed=20261020):
    rng = np.random.default_rng(seed)
    m = (rng.integers(1, (1 << 23) - 1, size=n - 3, dtype=np.int64) | 0x3F800000).astype(np.uint32).view(F32)
    return np.concatenate([F32([1.0]), up(F32([1.0])), up(F32([2.0]), -1), m]).astype(F32)


def scales(dt="f32", exps=None, n=N_MANT):
    """(scale f32 [n * len(exps)], exponent [same]); for a 16-bit dtype the mantissas are rounded to it (a block's own absmax is an
    element of the block) and repeated values are kept: the layout stays the same for every dtype."""
    exps = EXPS[dt] if exps is None else exps
    m = mantissas(n)
    if dt != "f32":
        m = in_dtype(m, dt)
        m = np.where(m >= 2, neighbours(2.0, dt, 1)[0], m).astype(F32)             # stays in [1, 2)
    s = np.concatenate([np.ldexp(m, e).astype(F32) for e in exps])
    return s, np.repeat(np.asarray(exps), n)


def shared_div_ok(am):
    """quant_kernels.hip shared_div_ok for one lane: the absmax lies in the range where v_div_scale is the identity."""
    am = F32(am)
    return bool(am >= F32(2.0 ** -60) and am <= F32(2.0 ** 60))


def fp8_shared(s, v):
    """k_quantize_fp8's test for the shared division of element v by the row scale s."""
    s, v = F32(s), F32(v)
    return bool(s >= F32(2.0 ** -20) and s <= F32(2.0 ** 60) and (abs(v) >= F32(2.0 ** -90) or v == 0))


# absmax edges of the 4-bit kernels: the fast path's range [2^-60, 2^60] with the neighbours outside, and the clamp 1e-8 with both
# neighbours.  A block's own absmax cannot go below the clamp, so the lower range edge is reached with a supplied absmax only, where
# the kernel keeps the plain division anyway.
def q4_edges(dt, given):
    """[below, at, above] in dtype dt of 2^60 and of 1e-8, and for a supplied absmax of 2^-60 (f16 holds none of them)."""
    if dt == "f16":
        return np.zeros(0, dtype=F32)
    return np.concatenate([neighbours(float(F32(v)), "f32" if given else dt, 1) for v in ((2.0 ** 60, 1e-8, 2.0 ** -60) if given else (2.0 ** 60, 1e-8))])


FP8_EDGE_SCALES = [F32(2.0 ** -20), up(F32(2.0 ** -20)), up(F32(2.0 ** -20), -1), F32(2.0 ** 60), up(F32(2.0 ** 60)), up(F32(2.0 ** 60), -1),
                   F32(1e-12), up(F32(1e-12)), up(F32(1e-12), -1)]


# ----------------------------------------------------------------------------------------------- 4-bit: restatements
def midpoints(qt):
    """The boundaries between neighbouring codes, float64, ascending: 15 for NF4, 7 per sign for FP4."""
    if qt == "nf4":
        t = NF4.astype(np.float64)
        return (t[:-1] + t[1:]) / 2
    p = FP4_POS.astype(np.float64)
    m = (p[:-1] + p[1:]) / 2
    return np.concatenate([-m[::-1], m])


def neighbour_codes(qt):
    """[(code below, code above)] per midpoint of midpoints(qt), as indices into the code table."""
    if qt == "nf4":
        return [(i, i + 1) for i in range(15)]
    pos = [(i, i + 1) for i in range(7)]
    neg = [(8 + i + 1 if i + 1 else 0, 8 + i if i else 0) for i in range(7)]        # -0.0 (index 8) is never produced
    return neg[::-1] + pos


def argmin_codes(q, qt, chunk=1 << 18):
    """The reference's argmin over the f32 distances to the 16 codes, the first minimum wins (NaN distances: index 0)."""
    q = np.asarray(q, dtype=F32).reshape(-1)
    out = np.empty(q.size, dtype=np.uint8)
    tab = TABLE[qt]
    with np.errstate(all="ignore"):
        for i in range(0, q.size, chunk):
            d = np.abs(q[i:i + chunk, None] - tab[None, :])
            d = np.where(np.isnan(d), F32(np.inf), d)
            out[i:i + chunk] = np.argmin(d, axis=1)
    return out


def quotient(x, am, mutant=None):
    with np.errstate(all="ignore"):
        if mutant == "recip":
            return (np.asarray(x, F32) * (F32(1.0) / np.asarray(am, F32))).astype(F32)
        return (np.asarray(x, F32) / np.asarray(am, F32)).astype(F32)


def q4_literal(x, am, qt, mutant=None):
    """Codes [nblk, bs] of blocks x [nblk, bs] with absmax am [nblk]: x / am, literal argmin."""
    return argmin_codes(quotient(x, am[:, None], mutant), qt).reshape(x.shape)


def _threshold_between(a, b, table, qt):
    """The largest f32 that still selects the code below the midpoint of neighbouring values a < b, found with the literal argmin."""
    c = F32((np.float64(a) + np.float64(b)) / 2)
    cand = up(np.full(65, c, dtype=F32), np.arange(-32, 33))
    idx = argmin_codes(cand, qt)
    vals = table[idx]
    low = np.nonzero(vals == a)[0]
    assert low.size and (vals[low[-1] + 1:] == b).all() and low[-1] + 1 < cand.size
    return cand[low[-1]]


def thresholds(qt):
    """The f32 thresholds of the counting form: argmin == #{i : xn > thr[i]} (NF4), the same over |xn| among the non-negative codes (FP4)."""
    tab = NF4 if qt == "nf4" else FP4_POS
    return np.array([_threshold_between(tab[i], tab[i + 1], TABLE[qt], qt) for i in range(len(tab) - 1)], dtype=F32)


def code_bins(qt, thr=None):
    """The 256-bin first guess of nearest_code_lut: the thresholds safely below each bin (tools/gen_code_thresholds.py bin_table)."""
    thr = (thresholds(qt) if thr is None else thr).astype(np.float64)
    lo, scale = (-1.0, 128.0) if qt == "nf4" else (0.0, 256.0)
    return np.array([int((thr < lo + b / scale - 2.0 ** -23).sum()) for b in range(256)], dtype=np.int64)


def q4_counting(q, qt, thr=None, ge=False, bins=None, bin_shift=0):
    """The kernels' form on quotients q with |q| < 2^22: a count of thresholds, optionally from the 256-bin first guess (one exact compare
    finishes it).  thr / ge / bin_shift are the mutants' handles."""
    q = np.asarray(q, dtype=F32).reshape(-1)
    thr = thresholds(qt) if thr is None else thr
    a = q if qt == "nf4" else np.abs(q)
    gt = (lambda v, t: v >= t) if ge else (lambda v, t: v > t)
    with np.errstate(all="ignore"):
        if bins is None:
            j = gt(a[:, None], thr[None, :]).sum(axis=1)
        else:
            y = (a.astype(np.float64) * 128.0 + 128.0).astype(F32) if qt == "nf4" else (a * F32(256.0)).astype(F32)
            b = np.clip(np.trunc(np.where(np.isnan(y), 0, y)).astype(np.int64), 0, 255)
            b = np.clip(b + bin_shift, 0, 255)
            low = bins[b]
            pad = np.concatenate([thr, F32([np.inf])]).astype(F32)
            j = low + gt(a, pad[low])
    if qt == "fp4":
        j = np.where((q < 0) & (j > 0), 8 + j, j)
    return j.astype(np.uint8)


def unpack(packed, shape):
    """Codes [nblk, bs] from the packed bytes of a flat layout (low nibble = even index)."""
    p = np.asarray(packed, dtype=np.uint8).reshape(-1)
    return np.stack([p & 0xF, p >> 4], axis=1).reshape(shape)


# ----------------------------------------------------------------------------------------------- 4-bit: builders
def _pack_blocks(cand, lead, tid, bs):
    """cand [S, n] -> blocks [S * nb, bs]: `lead` [S] first in each block, then bs - 1 candidates, zeros after the last.  tid [n] -> [.., bs]
    (-1: not a boundary element)."""
    S, n = cand.shape
    per = bs - 1
    nb = -(-n // per)
    x = np.zeros((S, nb * per), dtype=F32)
    x[:, :n] = cand
    t = np.full((nb * per,), -1, dtype=np.int16)
    t[:n] = tid
    x = np.concatenate([np.broadcast_to(lead[:, None, None], (S, nb, 1)), x.reshape(S, nb, per)], axis=2)
    t = np.concatenate([np.full((nb, 1), -1, dtype=np.int16), t.reshape(nb, per)], axis=1)
    return x.reshape(S * nb, bs), np.broadcast_to(t[None], (S, nb, bs)).reshape(S * nb, bs), nb


def _scatter_edges(x, tid, am, exp, edge_x, edge_tid, edge_am):
    """Put the edge blocks alone among the others, one every len // n_edges blocks (an out-of-range absmax moves its whole wave onto the plain
    division), keeping the order of the rest."""
    n, ne = x.shape[0], edge_x.shape[0]
    pos = (np.arange(ne) * max(1, n // ne) + 37 + np.arange(ne)).astype(np.int64)
    order = np.full(n + ne, -1, dtype=np.int64)
    order[pos] = n + np.arange(ne)
    order[order < 0] = np.arange(n)
    cat = lambda a, b: np.concatenate([a, b])[order]
    return cat(x, edge_x), cat(tid, edge_tid), cat(am, edge_am), cat(exp, np.full(ne, 999)), pos


def q4_own(qt, dt="f32", bs=128, exps=None, steps=3, edges=True):
    """Blocks whose own absmax is the scale.  dict: x [nblk, bs] f32 values of dtype dt, am [nblk] the absmax the block has, tid [nblk, bs]
    the midpoint an element sits at (-1: none), exp [nblk] the scale's exponent (999: an edge block), edge_pos."""
    s, e = scales(dt, EXPS_OWN[dt] if exps is None else exps)
    eff = np.maximum(s, CLAMP)                                                             # the absmax the block has
    mid = midpoints(qt)
    cand = neighbours(mid[None, :] * eff.astype(np.float64)[:, None], dt, steps)          # [S, T, 2k + 1]
    S, T, W = cand.shape
    keep = np.abs(cand) <= eff[:, None, None]                                              # never above the block's absmax
    cand = np.where(keep, cand, F32(0)).reshape(S, T * W)
    tid = np.repeat(np.arange(T, dtype=np.int16), W)
    x, t, nb = _pack_blocks(cand, s, tid, bs)
    am, ex = np.repeat(eff, nb), np.repeat(e, nb)
    d = dict(edge_pos=np.zeros(0, dtype=np.int64))
    if edges and dt != "f16":
        es = q4_edges(dt, False)
        ee = np.maximum(es, CLAMP)
        ec = neighbours(mid[None, :] * ee.astype(np.float64)[:, None], dt, steps)
        ec = np.where(np.abs(ec) <= ee[:, None, None], ec, F32(0)).reshape(len(es), T * W)
        ex_x, ex_t, enb = _pack_blocks(ec, es, tid, bs)
        x, t, am, ex, pos = _scatter_edges(x, t, am, ex, ex_x, ex_t, np.maximum(np.repeat(es, enb), F32(1e-8)))
        d["edge_pos"] = pos
    d.update(x=np.ascontiguousarray(x), am=am.astype(F32), tid=np.ascontiguousarray(t), exp=ex, qt=qt, dt=dt, bs=bs)
    return d


def q4_given(qt, dt="f32", bs=8, exps=None, steps=3, edges=True, n=N_MANT):
    """A supplied absmax: x fixed in dtype dt near t * a, one block per f32 absmax within +-steps ulps of x / t (for 16-bit inputs this is how a
    quotient reaches a boundary).  The block holds x, -x and x for the neighbouring midpoints; only element 0 is counted (tid)."""
    s, e = scales("f32", EXPS[dt] if exps is None else exps, n)
    if edges and dt != "f16":
        es = q4_edges(dt, True)
        s, e = np.concatenate([s, es]), np.concatenate([e, np.full(len(es), 999)])
    mid = midpoints(qt)
    xs = in_dtype(mid[None, :] * s.astype(np.float64)[:, None], dt)                          # [S, T]
    am = neighbours(np.abs(xs.astype(np.float64) / mid[None, :]), "f32", steps)                # [S, T, W] f32
    S, T, W = am.shape
    x = np.zeros((S, T, W, bs), dtype=F32)
    for j in range(bs):
        x[..., j] = np.roll(xs, j // 2, axis=1)[:, :, None] * (F32(-1.0) if j & 1 else F32(1.0))
    tid = np.full((S, T, W, bs), -1, dtype=np.int16)
    tid[..., 0] = np.arange(T, dtype=np.int16)[None, :, None]
    return dict(x=x.reshape(-1, bs), am=am.reshape(-1).astype(F32), tid=tid.reshape(-1, bs), exp=np.repeat(e, T * W), qt=qt, dt=dt, bs=bs,
                edge_pos=np.nonzero(np.repeat(e, T * W) == 999)[0])


def fp4_ties_16bit(dt):
    """FP4's dyadic midpoints as exact ties in a 16-bit dtype: absmax values of one, two and three significant bits times each midpoint are
    representable, so x / absmax is the midpoint itself.  Blocks of 16: [a, +-t a for the 7 midpoints, 0]."""
    a = np.array([1.0, 2.0 ** -4, 1.5, 3.0 * 2.0 ** 5, 1.25, 1.75, 7.0 * 2.0 ** -3], dtype=F32)
    mid = midpoints("fp4")
    x = np.zeros((len(a), 16), dtype=F32)
    x[:, 0] = a
    x[:, 1:15] = (mid[None, :] * a.astype(np.float64)[:, None]).astype(F32)
    assert (in_dtype(x, dt) == x).all()
    tid = np.full(x.shape, -1, dtype=np.int16)
    tid[:, 1:15] = np.arange(14)
    return dict(x=x, am=a, tid=tid, exp=np.zeros(len(a), dtype=np.int64), qt="fp4", dt=dt, bs=16, edge_pos=np.zeros(0, dtype=np.int64))


def q4_sensitive(d):
    """[nblk, bs] bool: the element's code changes when its quotient moves to either f32 neighbour."""
    q = quotient(d["x"], d["am"][:, None]).reshape(-1)
    c = argmin_codes(q, d["qt"])
    with np.errstate(all="ignore"):
        return ((c != argmin_codes(up(q, 1), d["qt"])) | (c != argmin_codes(up(q, -1), d["qt"]))).reshape(d["x"].shape)


# ----------------------------------------------------------------------------------------------- int8: restatement
def rscale127(am):
    am = np.asarray(am, dtype=F32)
    with np.errstate(all="ignore"):
        return ((F32(1.0) / am) * F32(127.0)).astype(F32)


def int8_product(x, am, mutant=None):
    x, am = np.asarray(x, dtype=F32), np.asarray(am, dtype=F32)
    with np.errstate(all="ignore"):
        if mutant == "div127":
            return (x * (F32(127.0) / am)).astype(F32)          # 127 / am in one rounding
        if mutant == "xdivam":
            return ((x / am) * F32(127.0)).astype(F32)
        return (x * rscale127(am)).astype(F32)


def int8_round(p, mutant=None):
    with np.errstate(all="ignore"):
        if mutant == "away":
            r = np.trunc(p + np.copysign(F32(0.5), p)).astype(F32)
            r = np.where(np.abs(p) >= F32(2.0 ** 23), p, r)        # already an integer
        elif mutant == "trunc":
            r = np.trunc(p)
        else:
            r = np.rint(p)
        return np.clip(r, -127.0, 127.0).astype(np.int8)


def int8_codes(x, am, mutant=None):
    """clamp(rint(x * ((1 / am) * 127)), -127, 127); am broadcasts against x."""
    return int8_round(int8_product(x, am, mutant if mutant in ("div127", "xdivam") else None), mutant if mutant in ("away", "trunc") else None)


def int8_sensitive(x, am):
    p = int8_product(x, am)
    c = int8_round(p)
    return ((c != int8_round(up(p, 1))) | (c != int8_round(up(p, -1)))) & (p != 0)


# ----------------------------------------------------------------------------------------------- int8: builders
HALVES = np.arange(127, dtype=np.float64) + 0.5          # 0.5 ... 126.5


def int8_candidates(s, dt="f32", steps=2, clamp=False, positive=False):
    """[S, n] values of dtype dt within +-steps of (+-h) / rscale127(s) for every half-integer h; clamp: also 127.5, 128.5 and 200 (above
    the scale: for a supplied absmax only); positive: the positive half only (absmax values)."""
    h = np.concatenate([HALVES, [127.5, 128.5, 200.0]]) if clamp else HALVES
    s = s if clamp else np.maximum(s, CLAMP)                                                 # an own absmax is clamped
    c = neighbours(h[None, :] / rscale127(s).astype(np.float64)[:, None], dt, steps)         # [S, H, W]
    if not clamp:
        c = np.where(c <= s[:, None, None], c, F32(0))
    c = c.reshape(len(s), -1)
    return c if positive else np.concatenate([c, -c], axis=1)


def int8_rows(dt="f32", exps=None, width=None, n=N_MANT, edges=True):
    """Rows whose own absmax is the scale (column 0): x [S, width] (zeros after the candidates), am [S], exp [S]."""
    s, e = scales(dt, EXPS_OWN[dt] if exps is None else exps, n)
    if edges:
        es = neighbours(float(F32(1e-8)), dt, 1) if dt != "f16" else np.zeros(0, dtype=F32)      # 1e-8 is below f16's smallest value
        s, e = np.concatenate([s, es]), np.concatenate([e, np.full(len(es), 999)])
    c = int8_candidates(s, dt)
    w = c.shape[1] + 1 if width is None else width
    x = np.zeros((len(s), w), dtype=F32)
    x[:, 0] = s
    x[:, 1:1 + c.shape[1]] = c
    return dict(x=x, am=np.maximum(s, F32(1e-8)), exp=e, dt=dt)


def int8_blocks(dt="f32", bs=32, exps=None, given=False, n=N_MANT):
    """The same candidates cut into blocks of bs: own absmax (the scale leads each block) or supplied (no lead, the clamp's values included)."""
    s, e = scales(dt if not given else "f32", (EXPS if given else EXPS_OWN)[dt] if exps is None else exps, n)
    c = int8_candidates(s, dt, clamp=given)
    if given:
        nb = -(-c.shape[1] // bs)
        x = np.zeros((len(s), nb * bs), dtype=F32)
        x[:, :c.shape[1]] = c
        x = x.reshape(-1, bs)
    else:
        x, _, nb = _pack_blocks(c, s, np.zeros(c.shape[1], dtype=np.int16), bs)
    return dict(x=np.ascontiguousarray(x), am=np.repeat(s if given else np.maximum(s, CLAMP), nb), exp=np.repeat(e, nb), dt=dt, bs=bs)


def int8_absmax_blocks(dt="f32", bs=8, exps=(0,), n=N_MANT):
    """4-bit blocks [v, 0, ...] whose absmax values v meet the ties of the nested int8 quantisation (blocksize 256) of
    quantize_4bit(compress_statistics=True): each group of 256 blocks starts with the scale, the candidates follow."""
    s, e = scales(dt, exps, n)
    c = int8_candidates(s, dt, positive=True)
    v, _, ng = _pack_blocks(c, s, np.zeros(c.shape[1], dtype=np.int16), 256)                    # [S * ng, 256] absmax values
    x = np.zeros((v.size, bs), dtype=F32)
    x[:, 0] = v.reshape(-1)
    x[1::2, 0] *= F32(-1.0)                                                                   # the absmax is of |x|
    return dict(x=x, absmax=np.maximum(v.reshape(-1), F32(1e-8)), am2=np.repeat(s, ng), dt=dt, bs=bs)


def colrow_matrix(dt="f32", n=96, steps=2):
    """quantize_colrow: s[i, j] = sqrt(rm[i] * cm[j]).  Row 0 holds the column maxima C[j] in [2, 4), column 0 the row maxima a[i] in
    [1, 2); element [i, j] sits within +-steps of a half-integer over rscale127(s[i, j]), the half-integers cycling along the row."""
    a = scales(dt, (0,), n)[0]
    W = 2 * steps + 1
    ncol = 1 + 63 * W
    C = in_dtype(np.ldexp(mantissas(ncol, seed=7), 1), dt)
    C[0] = in_dtype(F32(3.9990234375), dt)
    rm = np.concatenate([[C.max()], a]).astype(F32)
    with np.errstate(all="ignore"):
        sc = np.sqrt((rm[:, None] * C[None, :]).astype(F32).astype(np.float64)).astype(F32)
    j = np.arange(ncol - 1)
    h = HALVES[j // W]                                                                          # h <= 62.5: h s / 127 stays below a[i]
    nb = neighbours(h[None, :] / rscale127(sc[1:, 1:]).astype(np.float64), dt, steps)           # [n, ncol - 1, W]
    x = np.zeros((n + 1, ncol), dtype=F32)
    x[0] = C
    x[1:, 0] = a
    x[1:, 1:] = nb[:, j, j % W]
    x[1:, 1::2] *= F32(-1.0)
    assert (np.abs(x[1:, 1:]) <= a[:, None]).all() and (np.abs(x[1:]) <= C[None, :]).all()
    return x


def coo_values(dt="f32", n=N_MANT, steps=2):
    """quantize_sparse_coo, q = rint(v / (max / 127)): one scale per call, so a list of value vectors [max, candidates] (one per mantissa
    would be n launches; the test takes a sample)."""
    s = scales(dt, (0, -30 if dt != "f16" else -6), n)[0]
    with np.errstate(all="ignore"):
        sc = (s / F32(127.0)).astype(F32)
    c = neighbours(HALVES[None, :] * sc.astype(np.float64)[:, None], dt, steps)
    c = np.where(c <= s[:, None, None], c, F32(0)).reshape(len(s), -1)
    return np.concatenate([s[:, None], c, -c], axis=1)


# ----------------------------------------------------------------------------------------------- FP8: restatement
def fp8_bump_table(k):
    """oracle.c fp8_round_up_ulps: how many f32 values below 2^k already report exponent k."""
    k = np.asarray(k)
    return np.select([k >= 9, k >= 5, k >= 3, k >= -1, k >= -3, k >= -7, k >= -15], [5, 2, 1, 0, 1, 2, 5], 11)


def fp8_quotient(x, s, mutant=None):
    x, s = np.asarray(x, dtype=F32), np.asarray(s, dtype=F32)
    with np.errstate(all="ignore"):
        n = (x * (F32(1.0) / s)).astype(F32) if mutant == "recip" else (x / s).astype(F32)
    return n


def fp8_encode(n, mutant=None):
    """The reference's encoder on the quotient n (before the clamp), the oracle's formula; mutant: None | "rne" | "nobump" | "bump+1" | "bump-1"
    | "subnormals"."""
    n = np.clip(np.asarray(n, dtype=F32), F32(-448.0), F32(448.0))
    sign = np.where(n < 0, 0x80, 0).astype(np.int64)
    a = np.abs(n)
    u = a.view(np.uint32).astype(np.int64)
    e = ((u >> 23) & 0xFF) - 127
    mant = u & 0x7FFFFF
    sub = ((u >> 23) & 0xFF) == 0
    nb = fp8_bump_table(e + 1)
    if mutant == "nobump":
        nb = np.zeros_like(nb)
    elif mutant == "bump+1":
        nb = nb + 1
    elif mutant == "bump-1":
        nb = np.maximum(nb - 1, 0)
    if mutant != "rne":
        e = e + ((0x7FFFFF - mant) < nb)
    e = np.where(sub, -127, e)
    with np.errstate(all="ignore"):
        m = (a / np.ldexp(F32(1.0), e.astype(np.int32)).astype(F32)).astype(F32) - F32(1.0)
        if mutant == "rne":
            mb = np.rint((m * F32(8.0)).astype(F32))                    # the OCP conversion: nearest even, the carry goes into the exponent
            e = np.where(mb >= 8, e + 1, e)
            mb = np.where(mb >= 8, 0, mb)
        else:
            mb = np.trunc(np.clip((m * F32(8.0)).astype(F32) + F32(0.5), F32(0.0), F32(7.0)))
    biased = e + 7
    code = sign | (np.clip(biased, 0, 15) << 3) | np.where(np.isnan(mb), 0, mb).astype(np.int64)
    code = np.where(biased >= 15, sign | 0x77, code)
    flushed = sign
    if mutant == "subnormals":
        with np.errstate(all="ignore"):
            flushed = sign | np.clip(np.rint((a * F32(512.0)).astype(F32)), 0, 7).astype(np.int64)
    code = np.where(biased <= 0, flushed, code)
    code = np.where(a == 0, sign, code)
    code = np.where(np.isnan(n), 0x7F, code)
    return code.astype(np.uint8)


def fp8_codes(x, s, mutant=None):
    return fp8_encode(fp8_quotient(x, s, "recip" if mutant == "recip" else None), None if mutant == "recip" else mutant)


def fp8_sensitive(x, s):
    n = fp8_quotient(x, s)
    c = fp8_encode(n)
    return ((c != fp8_encode(up(n, 1))) | (c != fp8_encode(up(n, -1)))) & (n != 0)


# ----------------------------------------------------------------------------------------------- FP8: builder
def fp8_boundaries():
    """(b float64, steps below, steps above, kind): mantissa midpoints (1 + (m + 0.5) / 8) 2^k for k in -6 ... 8, 2^k with the 8 f32 values
    below it for k in -9 ... 9, 448 and 256.  kind "dead": no decision boundary of the reference's encoder (its mantissa never carries, it
    flushes below 2^-6 and every |v| >= 256 becomes 0x77) -- the mutants' boundaries."""
    out = []
    for k in range(-6, 9):
        out += [((1 + (m + 0.5) / 8) * 2.0 ** k, 3, 3, "mid" if m < 7 and k < 8 else "dead") for m in range(8)]

    out += [(2.0 ** k, 8, 3, "pow2" if -6 <= k < 8 else "dead") for k in range(-9, 10)]
    out += [(448.0, 3, 3, "dead"), (256.0, 3, 3, "dead")]
    return out


def fp8_rows(dt="f32", exps=None, n=N_MANT, edges=True, width=None):
    """Rows of maximum 448 s (column 0).  x [S, width], s [S] the scale the row has (max / 448 in f32, clamped), bid [width] the boundary an
    element sits at (-1: none), exp [S]."""
    exps = {"f32": (0, -30, 40), "bf16": (0, -30, 40), "f16": (0, -6, 4)}[dt] if exps is None else exps
    s0, e = scales("f32", exps, n)
    if edges and dt != "f16":
        es = np.array(FP8_EDGE_SCALES, dtype=F32)
        s0, e = np.concatenate([s0, es]), np.concatenate([e, np.full(len(es), 999)])
    top = in_dtype(s0.astype(np.float64) * 448.0, dt)
    with np.errstate(all="ignore"):
        s = np.maximum((top / F32(448.0)).astype(F32), F32(1e-12))
    cols, bid = [], []
    for i, (b, lo, hi, _) in enumerate(fp8_boundaries()):
        k = max(lo, hi)
        c = neighbours(b * s.astype(np.float64), dt, k)[:, k - lo:k + hi + 1]
        cols += [c, -c]
        bid += [i] * (2 * c.shape[1])
    c = np.concatenate(cols, axis=1)
    c = np.where(np.abs(c) <= top[:, None], c, F32(0))
    w = c.shape[1] + 2 if width is None else width
    assert w >= c.shape[1] + 2
    x = np.zeros((len(s), w), dtype=F32)
    x[:, 0] = top
    x[:, 1:1 + c.shape[1]] = c
    if edges and dt != "f16":
        x[::5, w - 1] = in_dtype(F32(2.0 ** -90), dt)                 # numerators at the edge of the shared division's range
        x[1::5, w - 1] = -in_dtype(up(F32(2.0 ** -90), -1 if dt == "f32" else -(1 << 16)), dt)
    b = np.full(w, -1, dtype=np.int16)
    b[1:1 + c.shape[1]] = bid
    return dict(x=x, s=s, bid=b, exp=e, dt=dt)


# ----------------------------------------------------------------------------------------------- the mutants
Q4_MUTANTS = ["recip", "ge", "bin+1"]                     # plus ("thr", i, +-1) for every threshold of both tables: 44
INT8_MUTANTS = ["div127", "xdivam", "away", "trunc"]
FP8_MUTANTS = ["recip", "rne", "nobump", "bump+1", "bump-1", "subnormals"]


def q4_mutant_codes(d, mutant):
    """The codes of dataset d under a mutant of the 4-bit chain."""
    qt = d["qt"]
    if mutant == "recip":
        return q4_literal(d["x"], d["am"], qt, "recip")
    q = quotient(d["x"], d["am"][:, None]).reshape(-1)
    thr = thresholds(qt)
    if mutant == "ge":
        return q4_counting(q, qt, thr, ge=True).reshape(d["x"].shape)
    if mutant == "bin+1":
        return q4_counting(q, qt, thr, bins=code_bins(qt, thr), bin_shift=1).reshape(d["x"].shape)
    _, i, step = mutant
    t = thr.copy()
    t[i] = up(t[i], step)
    return q4_counting(q, qt, t).reshape(d["x"].shape)
