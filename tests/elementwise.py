"""
Element-by-element checks of matmul-shaped outputs against a float64 reference of the same operands.

``assert_linear_elementwise`` checks y = X . Wd^T + b one element at a time, with the bound that the library's numerics
promise (operands in the weight dtype, f32 accumulation in any order, one rounding to the weight dtype, one cast to the
output dtype):

    |y - r| <= g*S + (u_T + u_out)*(|r| + g*S) + a,      r = X . Wd^T + b,   S = |X| . |Wd|^T + |b|   (both in float64)

- g = (K + 2) * 2^-23 for 16-bit operands: their products are exact in f32, and this allows f32 accumulation in any order,
  the split-K partial adds and the bias add, with a 2x margin over round-to-nearest.  g = (2K + 2) * 2^-23 for f32 operands
  (k_gemm_f32 and the f32 generic kernel), whose products are rounded as well.  K is the contraction length.
- u_T: unit roundoff of the weight dtype (the f32 result rounded to it); u_out: that of the cast to the output dtype, 0 where
  the cast is exact; a = 2^-24 where f16 is involved (its subnormal spacing).

A norm-wise gate (goldenio.rel_fro) lets dozens of wholly wrong elements through on a large output and hardly sees an error in
a row of small magnitude; this bound is per element, so one wrong element, one element never written or one NaN that leaks
out of its row fails.  A kernel that multiplied without rounding the decoded weight to the weight dtype would miss by up to
u_T * S, and fails too.

Non-finite outputs are predicted from the operands, not from the float64 product (BLAS libraries need not propagate NaN / Inf
consistently): a NaN anywhere in row i of X, row n of Wd or b[n] makes y[i, n] NaN; so do Inf * 0 and Infs of opposite sign in
one dot product; otherwise an Inf product (or bias) gives that Inf.  r is compared on the elements expected finite only.
"""
import torch

UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TILES = (256, 128, 64)


def _out_unit(w_dtype, out_dtype):
    if out_dtype == w_dtype or out_dtype == torch.float32:
        return 0.0          # no cast, or a value already rounded to 16 bits widened to f32: exact
    return UNIT[out_dtype]


def _any_mm(a, b):
    """[M, K] bool x [N, K] bool -> [M, N] bool: some k with a[i, k] and b[n, k] (counts stay exact in f32 below 2^24)."""
    return (a.float() @ b.float().t()) > 0


def expected_nonfinite(X, Wd, bias=None):
    """(nan, +inf, -inf) masks [M, N] of X . Wd^T + b by the operand rules of the module docstring."""
    M, N = X.shape[0], Wd.shape[0]
    nan = torch.isnan(X).any(1)[:, None] | torch.isnan(Wd).any(1)[None, :]
    pos = torch.zeros(M, N, dtype=torch.bool, device=X.device)
    neg = torch.zeros_like(pos)
    infX, infW = torch.isinf(X), torch.isinf(Wd)
    if bool(infX.any()) or bool(infW.any()):
        nan = nan | _any_mm(infX, Wd == 0) | _any_mm(X == 0, infW)
        pX, nX, pW, nW = X > 0, X < 0, Wd > 0, Wd < 0         # (the Infs included; NaN is neither)
        pos = _any_mm(infX & pX, pW) | _any_mm(infX & nX, nW) | _any_mm(pX, infW & pW) | _any_mm(nX, infW & nW)
        neg = _any_mm(infX & pX, nW) | _any_mm(infX & nX, pW) | _any_mm(pX, infW & nW) | _any_mm(nX, infW & pW)
    if bias is not None:
        nan = nan | torch.isnan(bias)[None, :]
        pos = pos | (bias == float("inf"))[None, :]
        neg = neg | (bias == float("-inf"))[None, :]
    nan = nan | (pos & neg)
    return nan, pos & ~nan, neg & ~nan


def _compare(y, r, bound, nan_e, pos_e, neg_e, kernel, what):
    """Raise with a report of the worst element unless every element of y is where it should be; return max err / bound."""
    yd = y.double()
    fin_e = ~(nan_e | pos_e | neg_e)
    err = (yd - r).abs()
    ok = torch.where(fin_e, err <= bound, torch.ones_like(fin_e))     # a NaN where a number is due: err is NaN, not <= bound
    ok &= ~nan_e | torch.isnan(yd)
    ok &= ~pos_e | (yd == float("inf"))
    ok &= ~neg_e | (yd == float("-inf"))
    ratio = torch.where(fin_e, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    bad = ~ok
    if bool(bad.any()):
        score = torch.where(bad, torch.where(fin_e, ratio, torch.full_like(ratio, float("inf"))), torch.full_like(ratio, -1.0))
        i, n = divmod(int(torch.argmax(score)), y.shape[1])
        want = float(r[i, n]) if bool(fin_e[i, n]) else ("nan" if bool(nan_e[i, n]) else ("+inf" if bool(pos_e[i, n]) else "-inf"))
        tiles = ", ".join(f"{t}: ({i // t}, {n // t})" for t in TILES)
        raise AssertionError(f"{what} [{kernel}]: {int(bad.sum())} of {y.numel()} elements out of bounds; worst at (row {i}, col {n}): "
                             f"value {float(yd[i, n]):.9g}, reference {want}, bound {float(bound[i, n]):.3g}; "
                             f"tile (row, col) at {tiles}")
    return float(ratio.max()) if ratio.numel() else 0.0


def linear_bound(X, Wd, bias, w_dtype, out_dtype):
    """(r, bound) in float64 for y = X . Wd^T + b; non-finite operands read as 0 (their elements are checked by the masks)."""
    Xf = torch.where(torch.isfinite(X), X, torch.zeros_like(X)).double()
    Wf = torch.where(torch.isfinite(Wd), Wd, torch.zeros_like(Wd)).double()
    r = Xf @ Wf.t()
    S = Xf.abs() @ Wf.abs().t()
    if bias is not None:
        bf = torch.where(torch.isfinite(bias), bias, torch.zeros_like(bias)).double()
        r += bf
        S += bf.abs()
    K = X.shape[1]
    g = ((2 * K + 2) if w_dtype == torch.float32 else (K + 2)) * 2.0 ** -23
    a = 2.0 ** -24 if torch.float16 in (w_dtype, out_dtype) else 0.0
    bound = g * S + (UNIT[w_dtype] + _out_unit(w_dtype, out_dtype)) * (r.abs() + g * S) + a
    return r, bound


def assert_linear_elementwise(y, X, Wd, bias, w_dtype, out_dtype, kernel=""):
    """Check y = X . Wd^T + bias element by element (module docstring); return the largest err / bound ratio.

    X: the activation exactly as the op feeds it (after ``.to(w_dtype)``), [..., K]; Wd: the decoded weight [N, K] from the CPU
    oracle, not from the library; bias: [N] in the weight dtype, or None; y: the op's output [..., N] in out_dtype."""
    y2 = y.reshape(-1, y.shape[-1])
    dev = y2.device
    X2 = X.reshape(-1, X.shape[-1]).to(dev)
    Wd = Wd.to(dev)
    b = None if bias is None else bias.to(dev)
    assert y2.shape == (X2.shape[0], Wd.shape[0]), (tuple(y.shape), tuple(X.shape), tuple(Wd.shape))
    assert y2.dtype == out_dtype, (y2.dtype, out_dtype)
    r, bound = linear_bound(X2, Wd, b, w_dtype, out_dtype)
    nan_e, pos_e, neg_e = expected_nonfinite(X2, Wd, b)
    return _compare(y2, r, bound, nan_e, pos_e, neg_e, kernel, "y = X . Wd^T + b")


def int8_reference(A, B, sa, sb, chunk=None):
    """(A . B) (sa / 127) (sb / 127) in float64 on A's device, the int32 contraction exact (|sum| < 2^53): the value matmul_int8
    rounds to f32.  With `chunk`, B is widened a column chunk at a time (no float64 copy of a large B)."""
    M, N = A.shape[0], B.shape[1]
    Ad = A.double()
    if chunk is None:
        exact = Ad @ B.double()
    else:
        exact = torch.empty(M, N, dtype=torch.float64, device=A.device)
        for c0 in range(0, N, chunk):
            exact[:, c0:c0 + chunk] = Ad @ B[:, c0:c0 + chunk].double()
    return exact * (sa.double() / 127.0)[:, None] * (sb.double() / 127.0)[None, :]


def assert_int8_elementwise(y, r, out_dtype, kernel=""):
    """matmul_int8 against r = int8_reference(...): the contraction is exact, so y may differ by a few f32 roundings (the
    int32 -> f32 conversion, the two scale quotients and the two products: 8 units of 2^-24 allowed) and the output cast.
    NaN exactly where r is NaN (a NaN scale).  Returns the largest err / bound ratio."""
    y2 = y.reshape(-1, y.shape[-1])
    r = r.to(y2.device)
    a = 2.0 ** -24 if out_dtype == torch.float16 else 0.0
    u_out = 0.0 if out_dtype == torch.float32 else UNIT[out_dtype]
    nan_e = torch.isnan(r)
    rf = torch.where(nan_e, torch.zeros_like(r), r)
    bound = (8 * 2.0 ** -24 + u_out) * rf.abs() + a
    none = torch.zeros_like(nan_e)
    return _compare(y2, rf, bound, nan_e, none, none, kernel, "y = (A . B) sa sb / 127^2")


def assert_bound_elementwise(y, ref, bound, kernel="", what="y"):
    """y against a float64 reference with a given per-element bound; NaN / +-Inf exactly where ref has them."""
    y2 = y.reshape(ref.shape)
    ref = ref.to(y2.device).double()
    nan_e = torch.isnan(ref)
    pos_e, neg_e = ref == float("inf"), ref == float("-inf")
    rf = torch.where(nan_e | pos_e | neg_e, torch.zeros_like(ref), ref)
    return _compare(y2, rf, bound.to(y2.device), nan_e, pos_e, neg_e, kernel, what)
