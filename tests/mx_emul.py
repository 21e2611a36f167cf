"""
A numpy restatement of the OCP MX format of DESIGN.md §25 (include/mbnb_mx.h): quantise, decode, and the linear in float64
over the decoded operands; plus the generator of LOSSLESS rows that the exact GEMM tests run on, its wide-scale and one-signed
variants, and the same linear walked the way k_gemm_mx walks it, with the mutants that show the forms tables bite.

An MX tensor is [rows, K], K % 32 == 0: codes plus `scales` uint8 [rows, K / 32] (E8M0: byte b = 2^(b - 127), 0xFF = NaN block).
"fp4": E2M1, two codes per byte, the even k in the low nibble.  "fp8": OCP E4M3, one byte per element.

Everything here works on float64 copies of f32 values: a power-of-two scaling of an f32 value and the comparisons against the
element grid are exact in float64, so no rounding happens outside the one this file states.
"""
import numpy as np

BLOCK = 32
EMAX = {"fp4": 2, "fp8": 8}
FP4_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _e4m3_grid():
    g = np.empty(127)
    for c in range(127):                       # 0x00 .. 0x7E; 0x7F is NaN
        e, m = c >> 3, c & 7
        g[c] = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return g


FP8_GRID = _e4m3_grid()
GRID = {"fp4": FP4_GRID, "fp8": FP8_GRID}


def _nearest_even_code(a, grid):
    """|value| (float64, exact) -> the index of the nearest grid value, ties to the even index, saturating at the last one."""
    hi = np.searchsorted(grid, a, side="left").clip(1, len(grid) - 1)        # grid[hi - 1] < a <= grid[hi] inside the grid
    lo = hi - 1
    dl, dh = a - grid[lo], grid[hi] - a
    pick_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    return np.where(pick_hi, hi, lo).astype(np.uint8)


def quantize(x, elem="fp4"):
    """x: [rows, K] array of f32 (or anything that converts to f32 exactly) -> (codes uint8, scales uint8 [rows, K / 32])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, K = x.shape
    assert K % BLOCK == 0
    v = x.reshape(rows, K // BLOCK, BLOCK)
    bits = v.view(np.uint32)
    amax_bits = (bits & np.uint32(0x7FFFFFFF)).max(axis=2)
    E = (amax_bits >> np.uint32(23)).astype(np.int64)
    bad = E == 255                                                           # a NaN or an Inf in the block
    byte = np.where(bad, 255, np.maximum(E - EMAX[elem], 0)).astype(np.int64)
    scaled = np.ldexp(np.where(bad[..., None], 0.0, v.astype(np.float64)), (127 - np.where(bad, 127, byte))[..., None])
    sign = (bits >> np.uint32(31)).astype(np.uint8)
    mag = _nearest_even_code(np.abs(scaled), GRID[elem])
    code = mag | (sign << (3 if elem == "fp4" else 7))
    code = np.where(bad[..., None], 0, code).astype(np.uint8).reshape(rows, K)
    if elem == "fp4":
        code = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return code, byte.astype(np.uint8)


def unpack(codes, elem="fp4"):
    """codes as stored -> one code per element, [rows, K]"""
    if elem == "fp8":
        return codes
    out = np.empty((codes.shape[0], codes.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def decode_f64(codes, scales, elem="fp4"):
    """The exact value of every element, float64 [rows, K]: value(code) * 2^(byte - 127); NaN for a 0xFF byte or an fp8 NaN code."""
    c = unpack(np.asarray(codes, dtype=np.uint8), elem).astype(np.int64)
    if elem == "fp4":
        mag, neg, nan = FP4_GRID[c & 7], (c & 8) != 0, np.zeros(c.shape, bool)
    else:
        nan = (c & 0x7F) == 0x7F
        mag, neg = FP8_GRID[np.where(nan, 0, c & 0x7F)], (c & 0x80) != 0
    s = np.asarray(scales, dtype=np.int64)
    val = np.ldexp(np.where(neg, -mag, mag), np.repeat(s - 127, BLOCK, axis=1))
    return np.where(nan | np.repeat(s == 255, BLOCK, axis=1), np.nan, val)


def linear_f64(x_codes, x_scales, x_elem, w_codes, w_scales, bias=None):
    """decode(x) . decode(w)^T + bias in float64 (the weight is fp4)"""
    r = decode_f64(x_codes, x_scales, x_elem) @ decode_f64(w_codes, w_scales, "fp4").T
    return r if bias is None else r + np.asarray(bias, dtype=np.float64)[None, :]


def lossless(rows, K, seed):
    """[rows, K] float64 values +-grid * 2^e, e in {-1, 0, 1} per block, every block with one magnitude 4 or 6 at a random place:
    exactly representable in bf16 and f16, and quantised to exactly these codes by both formats (the block's amax is in [4, 8) * 2^e,
    so its scale is 2^e (fp4) or 2^(e - 6) (fp8, every scaled element a multiple of 32 up to 384)."""
    rng = np.random.default_rng(seed)
    nb = K // BLOCK
    mag = rng.integers(0, 8, size=(rows, nb, BLOCK))
    sign = rng.integers(0, 2, size=(rows, nb, BLOCK))
    top = rng.integers(0, BLOCK, size=(rows, nb))
    r, b = np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij")
    mag[r, b, top] = rng.integers(6, 8, size=(rows, nb))
    e = rng.integers(-1, 2, size=(rows, nb))
    val = np.ldexp(np.where(sign == 1, -FP4_GRID[mag], FP4_GRID[mag]), e[..., None])
    return val.reshape(rows, K)


def lossless_codes(x):
    """The fp4 codes and scales a lossless tensor must quantise to, built from its values directly (not through quantize())."""
    rows, K = x.shape
    v = x.reshape(rows, K // BLOCK, BLOCK)
    amax = np.abs(v).max(axis=2)
    e = np.floor(np.log2(amax)).astype(np.int64) - 2
    s = np.ldexp(np.abs(v), -e[..., None])
    mag = np.searchsorted(FP4_GRID, s)
    assert (FP4_GRID[mag] == s).all()
    code = (mag | ((np.signbit(v)).astype(np.int64) << 3)).astype(np.uint8).reshape(rows, K)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8), (e + 127).astype(np.uint8)


# ---------------------------------------------------------------- operands for the forms tables (tests/mx_cases.py)
def _lossless_parts(rows, K, seed, e_lo=-1, e_hi=1):
    """(signed grid values [rows, K / 32, 32], block exponents e [rows, K / 32]) of lossless(): the value is grid * 2^e"""
    rng = np.random.default_rng(seed)
    nb = K // BLOCK
    mag = rng.integers(0, 8, size=(rows, nb, BLOCK))
    sign = rng.integers(0, 2, size=(rows, nb, BLOCK))
    top = rng.integers(0, BLOCK, size=(rows, nb))
    r, b = np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij")
    mag[r, b, top] = rng.integers(6, 8, size=(rows, nb))
    e = rng.integers(e_lo, e_hi + 1, size=(rows, nb))
    return np.where(sign == 1, -FP4_GRID[mag], FP4_GRID[mag]), e


def wide(M, N, K, t, a0, c0, seed):
    """(x [M, K], w [N, K]) float64 whose block exponents span the format while x . w^T stays exact in f32 in any order:
    x[i, block b] = lossless * 2^(a_i + t_b), w[j, block b] = lossless * 2^(c_j - t_b) with a_i = a0 + i % 3, c_j = c0 + j % 3 and
    t_b = t[b % len(t)].  The per-block offset t_b cancels in every product, so output (i, j) is a sum of multiples of
    2^(a_i + c_j - 4); tests/test_mx_host.py asserts the sum of the magnitudes below 2^24 of that unit for every case."""
    gx, ex = _lossless_parts(M, K, seed)
    gw, ew = _lossless_parts(N, K, seed + 1)
    tb = np.array([t[b % len(t)] for b in range(K // BLOCK)], dtype=np.int64)
    a = a0 + np.arange(M) % 3
    c = c0 + np.arange(N) % 3
    x = np.ldexp(gx, (ex + a[:, None] + tb[None, :])[..., None]).reshape(M, K)
    w = np.ldexp(gw, (ew + c[:, None] - tb[None, :])[..., None]).reshape(N, K)
    return x, w, a, c


def one_signed(M, N, K, a, c, seed):
    """(x, w): |lossless| * 2^a_i with the sign of row i = (-1)^i, and |lossless| * 2^c: every product of a row has the row's sign, so
    a partial sum in any order lies between 0 and the whole sum and an overflow has one direction only."""
    gx, ex = _lossless_parts(M, K, seed)
    gw, ew = _lossless_parts(N, K, seed + 1)
    sgn = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
    x = np.ldexp(np.abs(gx) * sgn[:, None, None], (ex + np.asarray(a)[:, None])[..., None]).reshape(M, K)
    w = np.ldexp(np.abs(gw), (ew + np.asarray(c)[:, None])[..., None]).reshape(N, K)
    return x, w


# ---------------------------------------------------------------- the GEMM as k_gemm_mx walks it, and its mutants
MUTANTS = ("fp8_lane_map", "subnormal_bit", "nan_mask_fr", "tail_half")


def gemm_as_kernel(x_codes, x_scales, x_elem, w_codes, w_scales, bias=None, mutate=None, KS=128):
    """linear_f64 restated along k_gemm_mx's structure: K-steps of 128 whose k past K count as zeros, the fp8 bytes
    of a lane placed at the k the instruction reads them as, NaN rows and columns from the 0xFF scale bytes through 16-row
    fragment masks.  Unmutated it equals linear_f64 (asserted on every table in tests/test_mx_host.py).  `mutate` plants one of the
    mistakes the forms tables are there to catch:
      "fp8_lane_map"   the first build's map: a lane's 32 bytes are 32 consecutive k, which the instruction reads as the 16 k from
                       16 g and the 16 k from 64 + 16 g, each under the scale of the block it was placed in
      "subnormal_bit"  the lowest mantissa bit of a subnormal E4M3 code (exponent field 0) is dropped
      "nan_mask_fr"    the epilogue looks a row's NaN bit up by the lane's column index, fr, not by 4 g + r
      "tail_half"      the zeroing of the ragged last K-step starts one half (64 k) early"""
    assert mutate is None or mutate in MUTANTS
    xc = unpack(np.asarray(x_codes, dtype=np.uint8), x_elem).astype(np.int64)
    wc = unpack(np.asarray(w_codes, dtype=np.uint8), "fp4").astype(np.int64)
    M, K = xc.shape
    N = wc.shape[0]
    xs, ws = np.asarray(x_scales, dtype=np.int64), np.asarray(w_scales, dtype=np.int64)
    if x_elem == "fp4":
        xv = np.where(xc & 8, -FP4_GRID[xc & 7], FP4_GRID[xc & 7])
    else:
        c7 = xc & 0x7F
        if mutate == "subnormal_bit":
            c7 = np.where(c7 < 8, c7 & ~1, c7)
        xv = np.where(c7 == 0x7F, np.nan, FP8_GRID[np.minimum(c7, 0x7E)])
        xv = np.where(xc & 0x80, -xv, xv)
    wv = np.where(wc & 8, -FP4_GRID[wc & 7], FP4_GRID[wc & 7])
    Kp = (K + KS - 1) // KS * KS
    pad = lambda v, n, fill: np.concatenate([v, np.full((v.shape[0], n - v.shape[1]), fill, dtype=v.dtype)], axis=1)
    xv, wv = pad(xv, Kp, 0.0), pad(wv, Kp, 0.0)
    xsp, wsp = pad(xs, Kp // BLOCK, 127), pad(ws, Kp // BLOCK, 127)
    if mutate == "fp8_lane_map" and x_elem == "fp8":
        k = np.arange(Kp)
        step, g, r = k // KS, (k % KS) // 32, k % 32
        placed = step * KS + np.where(r < 16, 16 * g + r, 64 + 16 * g + (r - 16))
        moved = np.zeros_like(xv)
        moved[:, placed] = xv
        xv = moved
    cut = K - 64 if (mutate == "tail_half" and K % KS) else K
    xv[:, cut:] = 0.0
    wv[:, cut:] = 0.0
    xd = np.ldexp(xv, np.repeat(np.where(xsp == 255, 127, xsp) - 127, BLOCK, axis=1))
    wd = np.ldexp(wv, np.repeat(np.where(wsp == 255, 127, wsp) - 127, BLOCK, axis=1))
    r = xd @ wd.T
    if bias is not None:
        r = r + np.asarray(bias, dtype=np.float64)[None, :]
    a_nan, b_nan = (xs == 255).any(axis=1), (ws == 255).any(axis=1)
    rows, cols = np.arange(M)[:, None], np.arange(N)[None, :]
    if mutate == "nan_mask_fr":
        a_pad = np.concatenate([a_nan, np.zeros(16, bool)])
        row_nan = a_pad[(rows // 16) * 16 + cols % 16]
    else:
        row_nan = np.broadcast_to(a_nan[:, None], (M, N))
    return np.where(row_nan | b_nan[None, :], np.nan, r)
