"""
Where non-finite values are planted on the GEMM-family kernels, as data: importable without a GPU.

A kernel treats the contraction axis specially at a few places -- its first and last element, the start of the ragged last
k-step, a split-K slice boundary, the padding K_weight > K -- and answers a chunk that lies past K from a clamped address.  An
Inf or a NaN that sits exactly there shows what the kernel does with such a chunk: an Inf that meets a zeroed weight becomes a
NaN (Inf * 0), a row tail read from the next row brings that row's NaN along.  tests/test_gpu_nonfinite.py plants at these places
on every case of tests/kernel_cases.py and tests/gemm_variant_cases.py with a floating activation; tests/test_nonfinite_host.py
holds the plan itself.

positions(L, slice_len)   the positions along a contraction of length L: 0, L - 1, L // 2; for each g of WIDTHS the start of the
                          last (perhaps ragged) g-wide step, g * ((L - 1) // g), and the element before it; with split-K slices of
                          slice_len, every slice boundary s * slice_len < L and the element before it.  WIDTHS are the chunk, k-step
                          and tile widths of the kernels: 32 the lane chunk of k_gemv4, 64 the k-tile of the MFMA kernels, 128
                          the skinny block, 256 the k-step of k_gemm_small / k_gemm_mid, 2048 one trip of 64 lanes x 32 k.
passes(rows, L, ...)      planting passes, each a list of (row, k, value).  A row holds at most one planted value per pass, so its
                          expectation is not diluted by a second plant; every position receives a +-Inf in some pass, the signs
                          alternating along the positions (Inf is the kind that shows a same-row Inf * 0).  From 3 rows on, every
                          pass also has one row with a NaN (its position walks through the plan) and one row left untouched: a
                          NaN or an Inf in the untouched row, or a NaN in an Inf row, is leakage between rows.  One row takes
                          len(positions) passes of one Inf each.  With exactly 2 rows a pass cannot hold an Inf row, a NaN row
                          and an untouched row: it holds one planted row and one untouched row, an Inf pass per position (the
                          rows taking turns) and a NaN pass at the first and at the last position.
slice_length(c)           the k per split-K slice of a table case (None: one slice), from the launchers as
                          tests/gemm_variant_cases.py restates them.
"""
from tests import gemm_variant_cases as gv

WIDTHS = (32, 64, 128, 256, 2048)
INF, NAN = float("inf"), float("nan")

# ops whose activation is floating point and goes to the kernel as it is.  outlier_linear and the embeddings are out: see
# tests/test_gpu_nonfinite.py
ACTIVATION_OPS = ("matmul_4bit", "linear_int8", "matmul_fp8", "gemm_dense", "linear_dense", "grad")
WEIGHT_OPS = ("matmul_4bit", "linear_int8", "matmul_fp8", "grad", "grad_t", "matmul_int8")


def positions(L, slice_len=None):
    assert L >= 1
    p = {0, L - 1, L // 2}
    for g in WIDTHS:
        s = g * ((L - 1) // g)
        p.add(s)
        if s - 1 >= 0:
            p.add(s - 1)
    if slice_len:
        for s in range(slice_len, L, slice_len):
            p.update((s, s - 1))
    return sorted(p)


def passes(rows, L, slice_len=None):
    P = positions(L, slice_len)
    sign = [INF if j % 2 == 0 else -INF for j in range(len(P))]
    if rows == 1:
        return [[(0, k, sign[j])] for j, k in enumerate(P)]
    if rows == 2:
        out = [[(j % 2, k, sign[j])] for j, k in enumerate(P)]
        return out + [[(0, P[0], NAN)], [(1, P[-1], NAN)]]
    out, j, p = [], 0, 0
    while j < len(P):
        nan_row, free_row = p % rows, (p + 1) % rows
        one = [(nan_row, P[p % len(P)], NAN)]
        for r in range(rows):
            if r not in (nan_row, free_row) and j < len(P):
                one.append((r, P[j], sign[j]))
                j += 1
        out.append(one)
        p += 1
    return out


def rows_of(c):
    d = gv.derived(c) if c["op"] not in ("grad", "grad_t") else c
    return d["M"]


def contraction(c):
    """The contraction length of the case's floating activation: K, or N for the input gradient (dX = dY . W)."""
    return c["N"] if c["op"] == "grad" else c["K"]


def slice_length(c):
    """k per split-K slice of the case's launch, None where it runs in one slice."""
    op, L = c["op"], contraction(c)
    if op == "grad":
        if c["kernel"] != "grad_t+dense_splitk":
            return None
        s = gv.gemm_dense_plan(c["M"], c["K"], c["N"])[1]          # the forward's dense GEMM with K and N exchanged
        return gv._cdiv(L // 64, s) * 64 if s > 1 else None
    if op not in ACTIVATION_OPS:
        return None
    name, variant = gv.model(c)
    if "splitk" not in name:
        return None
    d = gv.derived(c)
    M, N, K = d["M"], d["N"], d["K"]
    if variant.startswith("decode128"):
        kps = gv._cdiv(K // 64, gv.matmul4_splitk_slices(M, N, K)) * 64
    elif variant.startswith("small8"):
        kps = gv._cdiv(K // 256, gv.gemm_small_plan(M, N, K, 8)[1]) * 256
    elif variant.startswith("small"):
        kps = gv._cdiv(K // 256, gv.gemm_small_plan(M, N, K)[1]) * 256
    elif variant.startswith("mid"):
        kps = gv._cdiv(gv._cdiv(K, 256), gv.gemm_mid_slices(M, N, K)) * 256
    elif variant.startswith("dense"):
        s = c["slices"] if op == "gemm_dense" and c["slices"] else gv.gemm_dense_plan(M, N, K)[1]
        kps = gv._cdiv(K // 64, s) * 64
    elif variant.startswith("f32 64"):
        t64 = gv._cdiv(M, 64) * gv._cdiv(N, 64)
        s = max(min(gv._cdiv(1024, t64), K // 256, 16), 1)
        kps = gv._cdiv(gv._cdiv(K, s), 32) * 32
    else:
        raise KeyError(variant)
    used = int(variant.rsplit(" x", 1)[1])
    assert gv._cdiv(K, kps) == used, (variant, kps)
    return kps


def case_passes(c):
    return passes(rows_of(c), contraction(c), slice_length(c))


def classes(t):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf, elementwise (an integer tensor of t's shape)."""
    import torch
    return torch.isnan(t) * 1 + (t == INF) * 2 + (t == -INF) * 3


def ieee_linear(X, Wd, bias=None):
    """X . Wd^T + b as IEEE arithmetic gives it in float64: every product formed, the sums taken elementwise, no BLAS (whose
    propagation of NaN / Inf, and of Inf * 0, is its own business).  [M, K] x [N, K] -> [M, N]; for small operands."""
    y = (X.double()[:, None, :] * Wd.double()[None, :, :]).sum(-1)
    return y if bias is None else y + bias.double()[None, :]


def adapter_classes(X, Wd, bias=None, adapter=None):
    """The classes of x . Wd^T + b + s (B . (A . x)) by ieee_linear: the adapter (A [R, K], B [N, R], s) applied as the kernels apply
    it, the down-projection first.  Operands at unit scale: nothing overflows by itself, in f32 or in float64."""
    y = ieee_linear(X, Wd, bias)
    if adapter is not None:
        A, B, s = adapter
        y = y + float(s) * ieee_linear(ieee_linear(X, A), B)
    return classes(y)


def planted(X0, one):
    """A copy of the activation X0 [rows, L] with the pass's values planted."""
    X = X0.clone()
    for r, k, v in one:
        X[r, k] = v
    return X


def untouched_rows(rows, one):
    return [r for r in range(rows) if r not in {p[0] for p in one}]


NAMES = ("finite", "NaN", "+Inf", "-Inf")


def assert_classes(y, want, what):
    """Every element of y in the class `want` (classes()) gives it; the first departure is reported."""
    got = classes(y).reshape(want.shape).to(want.device)
    bad = (got != want).nonzero()
    if bad.numel():
        i, n = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} elements in another class than the IEEE evaluation; first at "
                             f"(row {i}, col {n}): value {NAMES[int(got[i, n])]}, reference {NAMES[int(want[i, n])]}")
