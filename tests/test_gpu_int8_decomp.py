"""
The col+row INT8 and COO sparse operations (libmbnb_sparse.so) on the GPU.  Every output and workspace the Python API allocates comes
back 0xFF-poisoned (tests/poison.py), so an element no kernel writes reads as NaN / -1.

1. exact against the emulation (tests/int8_decomp_emul.py: the rounding chains of include/mbnb_sparse.h, sqrt in float64 rounded to f32):
   statistics, codes and dequantize_colrow outputs, sparse_coo_from_dense (indices, values, order) and quantize_sparse_coo, bit for bit,
   on the goldens' inputs and on larger random ones (up to 4096 x 11008);
2. against the reference's goldens (tests/golden/g12_int8_decomp.npz): statistics, from_dense and quantize_sparse_coo bit-equal; every
   golden code and Wd element equals the chain with s[i, j] or with the next f32 below it (torch's CPU sqrt is 1 ulp low on ~0.6 % of
   inputs; no other difference passes and no share of elements is exempt); matmul_colrow and spmm within derived bounds;
3. every kernel route of tests/int8_decomp_cases.py element by element against float64;
4. determinism of spmm_coo, the sorted and the general path against each other;  5. out-of-range indices and guard bands;
6. the scenarios of the reference's tests/test_sparse.py, restated against 'cuda'.

spmm bound (the form of tests/elementwise.py with K replaced by the row's entry count n_i):
    |y - r| <= g S + u_T (|r| + g S) + a,   g = (n_i + 2) 2^-23 for 16-bit operands (exact products), (2 n_i + 2) 2^-23 for f32,
    r = sum val * dense and S = sum |val| |dense| in float64, a = 2^-24 for f16 (its subnormal spacing).
Against the reference's goldens the bound also covers the reference's own error: its f32 sum in another order for f32 (+ g S once more),
its rounding after every add for 16-bit dtypes (+ n_i u_T S): |y - golden| <= g S + u_T (|r| + g S) + a + that term, nothing more.
matmul_colrow against its golden allows twice the bound of tests/elementwise.py: ours and the reference's output are two independently
rounded T results within that bound of the same float64 product (one ulp = 2 u_T |r| apart at most from the roundings alone), and the
reference's Wd may sit 1 ulp off the emulation's where its sqrt is low.
Non-finite outputs are predicted from the operands: r is accumulated entry by entry in float64, where
NaN, Inf * 0 and Inf - Inf propagate as they do in f32, and only the entries of a row take part (a NaN row of `dense` that no entry points
at must not leak); NaN / +Inf / -Inf must then stand exactly where r has them.
"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _sparse_native, synthetic
from mps_bitsandbytes_amd import functional as F
from tests import forms, guard
from tests import int8_decomp_cases as cases_mod
from tests import int8_decomp_emul as emul
from tests.forms import memo as _memo
from tests.elementwise import UNIT, assert_bound_elementwise, assert_linear_elementwise, linear_bound
from tests.goldenio import DT, HERE, from_bits
from tests.guard import guarded_alloc  # noqa: F401  (the fixture, by name: it replaces poisoned_alloc's proxy in the tests that ask for it)
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name: every torch.empty of functional.py comes back 0xFF)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"
_bits = emul.bits


@pytest.fixture(scope="module")
def g12():
    import json
    import os
    with open(os.path.join(HERE, "manifest_int8_decomp.json")) as f:
        manifest = json.load(f)["g12"]
    return manifest, np.load(os.path.join(HERE, "g12_int8_decomp.npz"))


def _spread(R, C, T, seed):
    """A matrix whose rows and columns are scaled log-normally (several orders of magnitude), made on the device."""
    x = synthetic.normal_device((R, C), torch.float32, seed=seed, std=0.05, device=DEV)
    x = x * torch.exp(1.5 * synthetic.normal_device((R, 1), torch.float32, seed=seed + 1, device=DEV))
    x = x * torch.exp(1.5 * synthetic.normal_device((1, C), torch.float32, seed=seed + 2, device=DEV))
    return x.to(T)


def _expected_quantize(x):
    e_rm, e_cm = emul.colrow_stats(x)
    s = emul.colrow_scale(e_rm, e_cm)
    return e_rm, e_cm, s, emul.colrow_codes(x, s)


def _check_quantize(x_dev, kernel=None, run=None):
    """quantize_colrow of x against the emulation, bit for bit; returns (q, rm, cm, s, codes of the emulation), the first three on the device.
    `run`: the table's run (name, variant and guard bands are its business, the emulation is shared between its fills)."""
    q, rm, cm = bnb.quantize_colrow(x_dev)
    if kernel is not None:
        assert _sparse_native.last_kernel() == kernel
    if run is not None:
        run.end()
    R, C = x_dev.shape
    assert q.dtype == torch.int8 and q.shape == (R, C) and rm.dtype == cm.dtype == torch.float32 and rm.shape == (R,) and cm.shape == (C,)
    e_rm, e_cm, s, e_q = _memo(("quantize", run.id), lambda: _expected_quantize(x_dev.cpu())) if run is not None else _expected_quantize(x_dev.cpu())
    assert np.array_equal(rm.cpu().numpy().view(np.uint32), e_rm.view(np.uint32)), "row statistics differ from the emulation"
    assert np.array_equal(cm.cpu().numpy().view(np.uint32), e_cm.view(np.uint32)), "column statistics differ from the emulation"
    bad = int((q.cpu().numpy() != e_q).sum())
    assert bad == 0, f"{bad} of {q.numel()} codes differ from the emulation"
    return q, rm, cm, s, e_q


def _check_dequant(q, rm, cm, T, s=None, kernel=None, route=None, run=None):
    wd = F._colrow_dequant_pass(q, rm, cm, T) if route == "pass" else bnb.dequantize_colrow(q, rm, cm, T)
    if kernel is not None:
        assert _sparse_native.last_kernel() == kernel
    if run is not None:
        run.end()
    assert wd.dtype == T and wd.shape == q.shape

    def expected():
        return emul.colrow_wd(q.cpu().numpy(), emul.colrow_scale(rm.cpu().numpy(), cm.cpu().numpy()) if s is None else s, T)

    e_wd = _memo(("dequant", run.id), expected) if run is not None else expected()
    bad = int((_bits(wd) != _bits(e_wd)).sum())
    assert bad == 0, f"{bad} of {wd.numel()} dequantize_colrow elements differ from the emulation"
    return wd


# ----------------------------------------------------------------------------- COO helpers
def _lists(rows, cols, density, index, seed):
    """(row, col) on the device: a random pattern in row-major order, then permuted / narrowed to int32 / given duplicates."""
    u = synthetic.normal_device((rows, cols), torch.float32, seed=seed, device=DEV)
    # P(|N(0,1)| > t) = density
    t = float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - density / 2.0))) if 0 < density < 1 else (-1.0 if density >= 1 else 1e9)
    mask = u.abs() > t
    if rows > 2:
        mask[rows // 2, :] = False         # an empty row
    idx = mask.nonzero()
    r, c = idx[:, 0].contiguous(), idx[:, 1].contiguous()
    if index in ("permuted", "duplicates") and r.numel() > 0:
        if index == "duplicates":
            r, c = torch.cat([r, r[::3]]), torch.cat([c, c[::3]])
        perm = torch.argsort(synthetic.normal_device((r.numel(),), torch.float32, seed=seed + 1, device=DEV))
        r, c = r[perm].contiguous(), c[perm].contiguous()
    if index == "int32":
        r, c = r.to(torch.int32), c.to(torch.int32)
    return r, c


def _spmm_and_path(*args, **kw):
    """(out, path, workspace) of functional._spmm_coo: path is the first int32 of the workspace the call allocated, 0 where the device found
    `row_indices` non-decreasing and used the list in place, 1 where it built the CSR form.  The workspace (uint8, whole; its layout is
    _csr_arrays') is the call's last uint8 allocation; it is caught on its way through the `torch` proxy that functional.py sees under
    this module's fixtures."""
    proxy, seen = F.torch, []
    inner = proxy.empty

    def recording(*a, **k):
        t = inner(*a, **k)
        if k.get("dtype") == torch.uint8:
            seen.append(t)
        return t

    proxy.empty = recording
    try:
        out = F._spmm_coo(*args, **kw)
    finally:
        del proxy.empty
    return out, int(seen[-1][:4].view(torch.int32).item()), seen[-1]


def _csr_arrays(ws, nnz, rows):
    """(flag, row_ptr [rows + 1], cursor [rows], perm [nnz]) as int64 numpy arrays: the workspace's layout (sparse_kernels.hip; its sizes
    are asserted without a GPU by test_workspace_queries_are_host_arithmetic), each part rounded up to 256 bytes."""
    r256 = lambda b: (b + 255) // 256 * 256     # noqa: E731
    w = ws.cpu().numpy()
    assert w.size >= 256 + r256((rows + 1) * 4) + r256(rows * 4) + r256(nnz * 4)
    take = lambda at, n: w[at:at + 4 * n].view(np.int32).astype(np.int64)     # noqa: E731
    a_ptr, a_cur = 256, 256 + r256((rows + 1) * 4)
    return int(take(0, 1)[0]), take(a_ptr, rows + 1), take(a_cur, rows), take(a_cur + r256(rows * 4), nnz)


def _spmm_reference(r, c, val, dense, rows):
    """(ref, S, n_i) in float64 on the device: sum val * dense, sum |val| |dense| and the entry count per output row.  Entries outside
    the shape are dropped, as the kernel drops them."""
    cols = dense.shape[0]
    r, c = r.long(), c.long()
    ok = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
    r, c, v = r[ok], c[ok], val[ok].double()
    ref = torch.zeros(rows, dense.shape[1], dtype=torch.float64, device=dense.device)
    S = torch.zeros_like(ref)
    d = dense.double()
    step = max(1, (1 << 24) // max(1, dense.shape[1]))
    for i in range(0, r.numel(), step):
        term = v[i:i + step, None] * d[c[i:i + step]]
        ref.index_add_(0, r[i:i + step], term)
        S.index_add_(0, r[i:i + step], torch.where(torch.isfinite(term), term.abs(), torch.zeros_like(term)))
    n_i = torch.bincount(r, minlength=rows).double()
    return ref, S, n_i


def _spmm_bound(ref, S, n_i, T, golden=False):
    g = ((2 * n_i + 2) if T == torch.float32 else (n_i + 2)) * 2.0 ** -23
    gS = g[:, None] * S
    rf = torch.where(torch.isfinite(ref), ref.abs(), torch.zeros_like(ref))
    bound = gS + UNIT[T] * (rf + gS) + (2.0 ** -24 if T == torch.float16 else 0.0)
    if golden:
        bound = bound + (gS if T == torch.float32 else n_i[:, None] * UNIT[T] * S)
    return bound


def _check_spmm(y, r, c, val, dense, rows, T, kernel, golden_y=None):
    ref, S, n_i = _spmm_reference(r, c, val, dense, rows)
    assert y.dtype == T and y.shape == ref.shape
    ratio = assert_bound_elementwise(y, ref, _spmm_bound(ref, S, n_i, T), kernel, "out = sparse . dense")
    if golden_y is not None:
        fin = torch.isfinite(ref)
        gy = golden_y.to(y.device).double()
        ratio_g = assert_bound_elementwise(y, torch.where(fin, gy, ref), _spmm_bound(ref, S, n_i, T, golden=True), kernel,
                                           "out against the reference's golden")
        print(f"spmm {kernel}: err / bound {ratio:.3f} against float64, {ratio_g:.3f} against the golden")
    return ratio


# ----------------------------------------------------------------------------- 3 (and 1): every case of the table
_SENTINEL = {}


def _sentinel(case):
    """A call of another entry point whose launcher sets no variant: the case's own name and variant cannot be left over from before."""
    if not _SENTINEL:
        _SENTINEL["x"] = torch.ones(3, 5, device=DEV)
        _SENTINEL["q"] = torch.ones(3, 5, dtype=torch.int8, device=DEV)
    if case["op"] in ("count", "from_dense"):
        bnb.dequantize_colrow(_SENTINEL["q"], _SENTINEL["x"][:, 0], _SENTINEL["x"][0], torch.float32)
        name = "colrow_dequant1"
    else:
        F._coo_row_ptr(_SENTINEL["x"], 0.0)
        name = "coo_count"
    assert _sparse_native.last_kernel() == name
    assert _sparse_native.last_variant() == "", "a call whose launcher sets no variant reports the previous call's"


def _Run(case, proxy=None, fill=None):
    return forms.Run(cases_mod, _sparse_native, _sentinel, case, proxy, fill)


def _nonfinite_matrix(x):
    """A NaN in the first chunk and row block, a +Inf in the last of both, a -Inf behind the first chunk and row-block boundary."""
    R, C = x.shape
    x[3, 5], x[R - 1, C - 1], x[17, min(C - 1, 2050)] = float("nan"), float("inf"), float("-inf")
    return x


def _edge_matrix(x, thr):
    """from_dense's edges: +-threshold as the dtype rounds it (kept), the next value below it (dropped), -0.0 and 0.0 (dropped), NaN and
    +-Inf (kept, with and without a threshold)."""
    t = torch.tensor(0.3 if thr == 0 else thr, dtype=x.dtype)
    below = (t.view(torch.int16 if x.element_size() == 2 else torch.int32) - 1).view(x.dtype)
    x[0, 0], x[0, 1], x[1, 64], x[1, 65] = t, -t, below, -below
    x[2, 3], x[2, 65], x[3, 129], x[4, 0], x[5, 5], x[32, 128] = -0.0, float("nan"), float("inf"), float("-inf"), 0.0, float("nan")
    return x


def _run_case(case, proxy=None, fill=None):
    T = DT[case["dt"]]
    op, kernel = case["op"], case["kernel"]
    run = _Run(case, proxy, fill)
    seed = 2100 + sum(map(ord, cases_mod.case_id({k: v for k, v in case.items() if k not in ("off", "variant", "special")}))) % 997
    nonfinite = case.get("special") == "nonfinite"
    if op == "quantize":
        x0 = _spread(case["R"], case["C"], T, seed)
        if nonfinite:
            x0 = _nonfinite_matrix(x0)
        run.begin()
        q, rm, cm, _, _ = _check_quantize(run.put("x", x0), run=run)
        if nonfinite:
            R, C = x0.shape
            assert bool(torch.isnan(rm[3])) and bool(torch.isnan(cm[5])) and bool(torch.isinf(rm[R - 1])) and bool(torch.isinf(cm[C - 1])) and bool(torch.isinf(rm[17]))
            assert not bool(q[3].any()) and not bool(q[:, 5].any()) and not bool(q[R - 1].any()) and not bool(q[17].any())
        return
    if op == "dequant":
        R, C = case["R"], case["C"]
        q = synthetic.int8_tensor((R, C), seed=seed).to(DEV)
        rm = synthetic.normal_device((R,), torch.float32, seed=seed + 1, device=DEV).abs().clamp_min(1e-8)
        cm = synthetic.normal_device((C,), torch.float32, seed=seed + 2, device=DEV).abs().clamp_min(1e-8)
        if nonfinite:
            rm[3], rm[R - 1], cm[C - 1], cm[5] = float("nan"), float("inf"), float("inf"), float("nan")
            q[R - 1, 7] = 0          # 0 * Inf
        run.begin()
        wd = _check_dequant(run.put("q", q), run.put("rm", rm), run.put("cm", cm), T, route=case.get("route"), run=run)
        if nonfinite:
            assert bool(torch.isnan(wd[3]).all()) and bool(torch.isnan(wd[:, 5]).all()) and bool(torch.isnan(wd[R - 1, 7])) and bool(torch.isinf(wd[0, C - 1]) or q[0, C - 1] == 0)
        return
    if op == "matmul":
        N, K = case["N"], case["K"]
        lead = tuple(case["lead"]) if "lead" in case else (case["M"],)
        q, rm, cm = bnb.quantize_colrow(_spread(N, K, torch.float32, seed))
        x = synthetic.normal_device(lead + (K,), T, seed=seed + 3, device=DEV)
        b = synthetic.normal_device((N,), T, seed=seed + 4, device=DEV) if case.get("bias") else None
        flags = _sparse_native.FORCE_GENERIC if case.get("generic") else 0
        wd = _memo(("wd", N, K, seed, T), lambda: emul.colrow_wd(q.cpu().numpy(), emul.colrow_scale(rm.cpu().numpy(), cm.cpu().numpy()), T))
        run.begin()
        x, q, rm, cm, b = run.put("x", x), run.put("w", q), run.put("rm", rm), run.put("cm", cm), run.put("bias", b)
        y = F._matmul_colrow(x, q, rm, cm, b, T, flags)
        run.end()
        assert y.shape == lead + (N,) and y.dtype == T
        assert_linear_elementwise(y.reshape(-1, N), x.reshape(-1, K), wd, b, T, T, kernel)
        return
    if op in ("count", "from_dense"):
        R, C, thr = case["R"], case["C"], case.get("threshold", 0.0)
        x = synthetic.normal_device((R, C), T, seed=seed, device=DEV)
        if case["density"] < 1:
            keep = synthetic.normal_device((R, C), torch.float32, seed=seed + 1, device=DEV).abs() > float(
                torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - case["density"] / 2.0)))
            x = x * keep
        if case.get("special") == "edges":
            x = _edge_matrix(x, thr)
        er, ec, ev = _memo(("coo", run.id), lambda: emul.coo_from_dense(x.cpu(), thr))
        run.begin()
        x = run.put("x", x)
        if op == "count":
            _, _, row_ptr = F._coo_row_ptr(x, thr)
            run.end()
            want = torch.zeros(R + 1, dtype=torch.int64)
            want[1:] = torch.cumsum(torch.bincount(er, minlength=R), 0)
            assert torch.equal(row_ptr.cpu(), want)
            return
        r, c, v, rows, cols = bnb.sparse_coo_from_dense(x, thr)
        run.end()
        assert (rows, cols) == (R, C) and r.dtype == c.dtype == torch.int64 and v.dtype == T
        assert torch.equal(r.cpu(), er) and torch.equal(c.cpu(), ec) and torch.equal(_bits(v), _bits(ev))
        if case.get("special") == "edges":
            kept = set(zip(er.tolist(), ec.tolist()))
            assert {(2, 65), (3, 129), (4, 0), (32, 128)} <= kept and not {(2, 3), (5, 5)} & kept
            assert ({(0, 0), (0, 1)} <= kept and not {(1, 64), (1, 65)} & kept) if thr > 0 else {(0, 0), (0, 1), (1, 64), (1, 65)} <= kept
        return
    if op == "quantize_coo":
        n = case["n"]
        v = synthetic.normal_device((n,), T, seed=seed, std=0.37, device=DEV)
        if nonfinite:
            v[5], v[n - 1], v[7] = float("nan"), float("inf"), float("-inf")
        idx = torch.arange(n, device=DEV)
        eq, es = _memo(("cooq", run.id), lambda: emul.coo_quantize(v.cpu()))
        run.begin()
        v = run.put("values", v)
        r, c, q, scale = bnb.quantize_sparse_coo(idx, idx, v)
        run.end()
        assert r is idx and c is idx and q.dtype == torch.int8 and q.shape == (n,) and scale.dtype == torch.float32 and scale.shape == (1,)
        assert torch.equal(q.cpu(), eq) and torch.equal(_bits(scale), _bits(es))
        if nonfinite:
            assert bool(torch.isnan(scale).all()) and not bool(q.any())
        return
    assert op == "spmm"
    rows, cols, N = case["rows"], case["cols"], case["N"]
    r, c = _lists(rows, cols, case["density"], case["index"], seed)
    nnz = r.numel()
    vals = synthetic.normal_device((nnz,), T, seed=seed + 2, device=DEV)
    dense = synthetic.normal_device((cols, N), T, seed=seed + 3, device=DEV)
    flags = _sparse_native.FORCE_GENERIC if case.get("generic") else 0
    if case["values"] == "T":
        kind, scale, what, used = _sparse_native.COO_VALUES, None, "spmm_coo", vals
    else:
        vals = synthetic.int8_tensor((max(nnz, 1),), seed=seed + 4)[:nnz].to(DEV)
        scale = torch.tensor([0.0123], device=DEV) if case["values"] == "int8" else synthetic.normal_device((nnz,), torch.float32, seed=seed + 5, std=0.01, device=DEV)
        kind, what = (_sparse_native.COO_INT8_SCALAR if case["values"] == "int8" else _sparse_native.COO_INT8_ENTRY), "spmm_coo_int8"
        used = emul.coo_int8_values(vals.cpu(), scale.cpu(), T).to(DEV)
    run.begin()
    r, c, vals, dense, scale = run.put("row", r), run.put("col", c), run.put("values", vals), run.put("dense", dense), run.put("scale", scale)
    y, path, _ = _spmm_and_path(r, c, vals, kind, scale, dense, rows, cols, T, what, flags)
    run.end()
    assert path == (1 if case.get("generic") or case["index"] in ("permuted", "duplicates") else 0), "the device took the other path"
    if nnz == 0:
        assert not bool(_bits(y).any())
    _check_spmm(y, r, c, used, dense, rows, T, kernel)


@pytest.mark.parametrize("case", [c for c in cases_mod.CASES if not cases_mod.needs_plan(c)], ids=cases_mod.case_id)
def test_case(case):
    _run_case(case)


# every case that launches no GEMM again, inside guard bands and under two fills: an element the kernel never wrote holds the fill, and
# cannot equal the emulation under both (0xFF is the legal code -1); a store outside a buffer changes a band.  The cases that place one
# of functional.py's own allocations off its alignment run here only.
@pytest.mark.parametrize("fill", guard.FILLS, ids=lambda f: f"fill{f:02X}")
@pytest.mark.parametrize("case", [c for c in cases_mod.CASES if not cases_mod.launches_gemm(c)], ids=cases_mod.case_id)
def test_case_guarded(case, fill, guarded_alloc):
    _run_case(case, guarded_alloc, fill)
    assert guarded_alloc.allocs, "nothing went through the guarded proxy"


# ----------------------------------------------------------------------------- 1 + 2: the goldens
def test_goldens_colrow(g12):
    manifest, z = g12
    for case in (c for c in manifest if c["kind"] == "colrow"):
        i, T = case["id"], DT[case["dtype"]]
        x = from_bits(z[f"cr{i}_x"], T)
        q, rm, cm, s, e_q = _check_quantize(x.to(DEV))
        # statistics: bit-equal with the reference
        assert np.array_equal(rm.cpu().numpy().view(np.uint32), z[f"cr{i}_rm"]) and np.array_equal(cm.cpu().numpy().view(np.uint32), z[f"cr{i}_cm"]), case
        s_low = emul.colrow_scale(rm.cpu().numpy(), cm.cpu().numpy(), lower=True)
        gq = torch.from_numpy(z[f"cr{i}_q"])
        ok = emul.explained(gq, q.cpu(), torch.from_numpy(emul.colrow_codes(x, s_low)))
        assert bool(ok.all()), (case, int((~ok).sum()), "golden codes that neither s nor the next f32 below s explains")
        for t, To in DT.items():
            wd = _check_dequant(gq.to(DEV), rm, cm, To, s)
            ok = emul.explained(from_bits(z[f"cr{i}_wd_{t}"], To), wd.cpu(), emul.colrow_wd(gq.numpy(), s_low, To))
            assert bool(ok.all()), (case, t, int((~ok).sum()), "golden Wd elements that neither s nor the next f32 below s explains")


def test_goldens_matmul_colrow(g12):
    """Ours and the reference's output both lie within the bound of tests/elementwise.py around the float64 product of the same operands
    (Wd from the emulation), so they differ by at most twice that bound."""
    manifest, z = g12
    for case in (c for c in manifest if c["kind"] == "matmul_colrow"):
        i, T, N, K = case["id"], DT[case["dtype"]], case["N"], case["K"]
        q, rm, cm = torch.from_numpy(z[f"mm{i}_q"]), from_bits(z[f"mm{i}_rm"]), from_bits(z[f"mm{i}_cm"])
        x = from_bits(z[f"mm{i}_x"]).view(*case["lead"], K)
        b = from_bits(z[f"mm{i}_b"]) if case["bias"] else None
        y = bnb.matmul_colrow(x.to(DEV), q.to(DEV), rm.to(DEV), cm.to(DEV), None if b is None else b.to(DEV), dtype=T)
        assert y.shape == tuple(case["lead"]) + (N,) and y.dtype == T
        wd = emul.colrow_wd(q.numpy(), emul.colrow_scale(rm.numpy(), cm.numpy()), T)
        xt, bt = x.to(T).reshape(-1, K), None if b is None else b.to(T)
        assert_linear_elementwise(y.reshape(-1, N), xt, wd, bt, T, T, "matmul_colrow")
        _, bound = linear_bound(xt.to(DEV), wd.to(DEV), None if bt is None else bt.to(DEV), T, T)
        assert_bound_elementwise(y.reshape(-1, N), from_bits(z[f"mm{i}_y"], T).reshape(-1, N).double(), 2 * bound, "matmul_colrow", "y against the golden")


def test_goldens_from_dense_and_quantize_coo(g12):
    manifest, z = g12
    for case in (c for c in manifest if c["kind"] == "from_dense"):
        i, T = case["id"], DT[case["dtype"]]
        x = from_bits(z[f"fd{i}_x"], T).view(case["rows"], case["cols"])
        r, c, v, rows, cols = bnb.sparse_coo_from_dense(x.to(DEV), case["threshold"])
        assert (rows, cols) == (case["rows"], case["cols"]) and v.numel() == case["nnz"], case
        assert np.array_equal(r.cpu().numpy(), z[f"fd{i}_row"]) and np.array_equal(c.cpu().numpy(), z[f"fd{i}_col"]), case
        assert torch.equal(_bits(v), _bits(from_bits(z[f"fd{i}_val"], T))), case
    for case in (c for c in manifest if c["kind"] == "quantize_sparse_coo"):
        i, T = case["id"], DT[case["dtype"]]
        v = from_bits(z[f"qs{i}_v"], T).to(DEV)
        _, _, q, scale = bnb.quantize_sparse_coo(None, None, v)
        assert np.array_equal(q.cpu().numpy(), z[f"qs{i}_q"]) and np.array_equal(scale.cpu().numpy().view(np.uint32), z[f"qs{i}_scale"]), case


def test_goldens_spmm(g12):
    manifest, z = g12
    for case in (c for c in manifest if c["kind"] == "spmm"):
        i, T, rows, cols = case["id"], DT[case["dtype"]], case["rows"], case["cols"]
        r, c = torch.from_numpy(z[f"sp{i}_row"]).to(DEV), torch.from_numpy(z[f"sp{i}_col"]).to(DEV)
        v, d = from_bits(z[f"sp{i}_val"], T).to(DEV), from_bits(z[f"sp{i}_dense"], T).view(cols, case["N"]).to(DEV)
        y = bnb.spmm_coo(r, c, v, d, rows, cols)
        _check_spmm(y, r, c, v, d, rows, T, "spmm_coo", from_bits(z[f"sp{i}_y"], T).view(rows, -1))
        q, scale, per = torch.from_numpy(z[f"sp{i}_q"]).to(DEV), from_bits(z[f"sp{i}_scale"]).to(DEV), from_bits(z[f"sp{i}_per"]).to(DEV)
        _, _, q2, scale2 = bnb.quantize_sparse_coo(r, c, v)
        assert torch.equal(q2, q) and torch.equal(_bits(scale2), _bits(scale))
        y8 = bnb.spmm_coo_int8(r, c, q, scale, d, rows, cols, dtype=T)
        _check_spmm(y8, r, c, emul.coo_int8_values(q.cpu(), scale.cpu(), T).to(DEV), d, rows, T, "spmm_coo_int8", from_bits(z[f"sp{i}_y8"], T).view(rows, -1))
        y8e = bnb.spmm_coo_int8(r, c, q, per, d, rows, cols, dtype=T)
        _check_spmm(y8e, r, c, emul.coo_int8_values(q.cpu(), per.cpu(), T).to(DEV), d, rows, T, "spmm_coo_int8", from_bits(z[f"sp{i}_y8e"], T).view(rows, -1))


def test_colrow_nan_and_inf():
    x = _spread(64, 128, torch.float16, 77)
    x[3, 5], x[10, 20] = float("nan"), float("inf")
    q, rm, cm, _, _ = _check_quantize(x)
    assert bool(torch.isnan(rm[3])) and bool(torch.isnan(cm[5])) and bool(torch.isinf(rm[10])) and bool(torch.isinf(cm[20]))
    assert not bool(q[3].any()) and not bool(q[:, 5].any()) and not bool(q[10].any()) and not bool(q[:, 20].any())
    wd = _check_dequant(q, rm, cm, torch.float32)
    assert bool(torch.isnan(wd[3]).all()) and bool(torch.isnan(wd[:, 20]).all())


def test_spmm_nonfinite_values_follow_the_operands():
    T, rows, cols, N = torch.float32, 6, 10, 16
    r = torch.tensor([0, 0, 1, 2, 2, 4, 5], device=DEV)
    c = torch.tensor([1, 3, 0, 2, 9, 4, 5], device=DEV)
    v = torch.tensor([1.0, float("nan"), float("inf"), 2.0, -1.0, 0.0, 3.0], device=DEV)
    d = synthetic.normal_device((cols, N), T, seed=5, device=DEV)
    d[4, 3] = float("inf")       # times the explicit zero of row 4: NaN
    d[5, 7] = float("-inf")
    d[7, :] = float("nan")       # a row no entry points at: must not leak anywhere
    y = bnb.spmm_coo(r, c, v, d, rows, cols)
    _check_spmm(y, r, c, v, d, rows, T, "spmm_coo")
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isinf(y[1]).all()) and bool(torch.isnan(y[4, 3])) and bool(y[5, 7] == float("-inf"))
    assert not bool(y[3].any()) and bool(torch.isfinite(y[2]).all())


# ----------------------------------------------------------------------------- 4: determinism, the two paths
def test_spmm_is_deterministic_and_the_paths_agree():
    T, rows, cols, N = torch.float16, 1000, 2000, 256
    r, c = _lists(rows, cols, 0.05, "duplicates", 31)
    v = synthetic.normal_device((r.numel(),), T, seed=32, device=DEV)
    d = synthetic.normal_device((cols, N), T, seed=33, device=DEV)
    runs = [bnb.spmm_coo(r, c, v, d, rows, cols) for _ in range(3)]
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[0]), _bits(runs[2]))
    _check_spmm(runs[0], r, c, v, d, rows, T, "spmm_coo")
    # the same entries sorted by row (stable): the fast path uses them in place; the general path on the sorted list must give the same bits
    order = torch.argsort(r, stable=True)
    rs, cs, vs = r[order].contiguous(), c[order].contiguous(), v[order].contiguous()
    y_fast, path, _ = _spmm_and_path(rs, cs, vs, _sparse_native.COO_VALUES, None, d, rows, cols, T, "spmm_coo")
    assert _sparse_native.last_kernel() == "spmm_coo8" and path == 0
    y_gen, path, _ = _spmm_and_path(rs, cs, vs, _sparse_native.COO_VALUES, None, d, rows, cols, T, "spmm_coo", _sparse_native.FORCE_GENERIC)
    assert _sparse_native.last_kernel() == "spmm_coo8_general" and path == 1
    assert torch.equal(_bits(y_fast), _bits(y_gen)), "both paths sum a row's entries in entry order"
    # sorted by row, the order within a row is the permuted list's order too (stable sort), so all three agree bit for bit
    assert torch.equal(_bits(y_fast), _bits(runs[0]))
    _check_spmm(y_fast, rs, cs, vs, d, rows, T, "spmm_coo8")


# ----------------------------------------------------------------------------- 4b: the CSR build, held exactly
def _planned_list(lengths, cols, seed, extra_rows=0):
    """(row, col) int64 on the CPU, permuted: row i has lengths[i] entries, `extra_rows` further rows get random counts; a tenth of the
    entries more lie outside the shape, by row (below 0, at and past `rows`) or by column."""
    g = np.random.default_rng(seed)
    rows = len(lengths) + extra_rows
    r = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    if extra_rows:
        r = np.concatenate([r, g.integers(len(lengths), rows, size=4 * extra_rows)])
    c = g.integers(0, cols, size=r.size)
    n_bad = r.size // 10
    bad_r = g.choice(np.array([-1, -7, rows, rows + 1, 2 ** 31 - 1, -(2 ** 31)], dtype=np.int64), size=n_bad)
    bad_c = g.choice(np.array([-1, cols, cols + 5, 2 ** 31 - 1], dtype=np.int64), size=n_bad)
    half = n_bad // 2
    r = np.concatenate([r, bad_r[:half], g.integers(0, rows, size=n_bad - half)])
    c = np.concatenate([c, g.integers(0, cols, size=half), bad_c[half:]])
    order = g.permutation(r.size)
    return torch.from_numpy(r[order]), torch.from_numpy(c[order]), rows


def _check_csr(r, c, rows, cols, index_dtype, forced=False):
    """One spmm call on the list; its workspace against the build restated in numpy, integer for integer."""
    T, N = torch.float32, 8
    nnz = r.numel()
    rd, cd = r.to(index_dtype).to(DEV), c.to(index_dtype).to(DEV)
    v = synthetic.normal_device((nnz,), T, seed=71, device=DEV)
    d = synthetic.normal_device((cols, N), T, seed=72, device=DEV)
    y, path, ws = _spmm_and_path(rd, cd, v, _sparse_native.COO_VALUES, None, d, rows, cols, T, "spmm_coo", _sparse_native.FORCE_GENERIC if forced else 0)
    flag, row_ptr, cursor, perm = _csr_arrays(ws, nnz, rows)
    rn = r.numpy()
    sorted_list = bool((rn[1:] >= rn[:-1]).all())
    assert flag == path == (0 if sorted_list and not forced else 1)
    if flag == 0:
        # the list in place: row_ptr[i] = the first entry whose row is >= i; entries of negative rows lie before row_ptr[0]
        assert np.array_equal(row_ptr, np.searchsorted(rn, np.arange(rows + 1), side="left"))
        assert row_ptr[0] == int((rn < 0).sum())
        assert bool((perm == -1).all()) and not cursor.any(), "the sorted path writes neither perm (still the 0xFF fill) nor cursor (zeroed)"
    else:
        ok = (rn >= 0) & (rn < rows)         # by row: an entry whose column is outside the shape keeps its slot, k_spmm_csr skips it
        counts = np.bincount(rn[ok], minlength=rows)
        want_ptr = np.concatenate([[0], np.cumsum(counts)])
        assert np.array_equal(row_ptr, want_ptr), "row_ptr[i] = the number of in-range entries with row < i"
        assert np.array_equal(cursor, counts), "cursor[i] = the row's count"
        idx = np.nonzero(ok)[0]
        want_perm = idx[np.argsort(rn[ok], kind="stable")]          # row by row, the original indices ascending
        n_ok = int(ok.sum())
        bad = np.nonzero(perm[:n_ok] != want_perm)[0]
        assert bad.size == 0, (f"{bad.size} of {n_ok} slots of perm differ; the first in row {int(np.searchsorted(want_ptr, bad[0], side='right')) - 1} "
                               f"of {counts[int(np.searchsorted(want_ptr, bad[0], side='right')) - 1]} entries")
        assert bool((perm[n_ok:] == -1).all()), "no slot past the in-range entries is written"
    _check_spmm(y, rd, cd, v, d, rows, T, "spmm_coo")
    return row_ptr


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_csr_build_is_exact(index_dtype):
    """flag, row_ptr, cursor and perm of both paths, integer for integer: rows of 0, 1, 2, 3 and 5 entries (the sort's early return and the
    comparators its network skips), of 255 | 256 | 257 (one pass of the 256 threads), of 4095 | 4096 | 4097 (COO_SORT_LDS: LDS | global
    memory) and of 9000; a tenth of the entries outside the shape."""
    lengths = list(cases_mod.CSR_ROW_LENGTHS)
    r, c, rows = _planned_list(lengths, 300, 81)
    assert rows == 12
    row_ptr = _check_csr(r, c, rows, 300, index_dtype)
    assert (np.diff(row_ptr) >= np.array(lengths)).all()          # the planned entries, and the row's share of those with a bad column
    # the same entries stably sorted by row: the list in place, and the forced build on it (every segment arrives sorted or not: atomics)
    order = torch.argsort(r, stable=True)
    _check_csr(r[order].contiguous(), c[order].contiguous(), rows, 300, index_dtype)
    _check_csr(r[order].contiguous(), c[order].contiguous(), rows, 300, index_dtype, forced=True)


@pytest.mark.parametrize("rows", cases_mod.CSR_ROW_COUNTS)
def test_csr_scan_share(rows):
    """k_scan_counts<int> with 1, 2 and 5 rows per thread (1024 | 1025 | 5000 rows)."""
    r, c, n = _planned_list([3, 0, 70], 100, 90 + rows, extra_rows=rows - 3)
    assert n == rows
    _check_csr(r, c, rows, 100, torch.int64)
    order = torch.argsort(r, stable=True)
    _check_csr(r[order].contiguous(), c[order].contiguous(), rows, 100, torch.int32)


# ----------------------------------------------------------------------------- 4c: the summation order, bit for bit
def _lognormal(shape, T, seed):
    """Values over many binades, exp(3 N(0, 1)) with a random sign, representable in bf16 (and in T): the product of two of them is exact in
    f32, so fmaf(v, d, acc) is acc + v d rounded once, and a numpy loop of f32 adds is the kernel's arithmetic.  For f16 the values are
    scaled by 2^-10 and held within +-16 (0.06 % of them), so that no sum of 128 products leaves f16's range."""
    g = np.random.default_rng(seed)
    x = torch.from_numpy((np.exp(3.0 * g.standard_normal(shape)) * g.choice([-1.0, 1.0], size=shape)).astype(np.float32)).to(torch.bfloat16).float()
    if T == torch.float16:
        x = (x * 2.0 ** -10).clamp(-16.0, 16.0)
    return x.to(T)


def _ordered_sum(r, c, v, d, rows, T, reverse=False):
    """out[i] = the f32 sum of row i's products, added one by one in entry order (ascending list index), then rounded once to T."""
    rn = r.numpy()
    vf, df = v.float().numpy(), d.float().numpy()
    acc = np.zeros((rows, df.shape[1]), dtype=np.float32)
    for i in range(rows):
        es = np.nonzero(rn == i)[0]
        for e in (es[::-1] if reverse else es):
            acc[i] = acc[i] + vf[e] * df[c[e]]          # the product is exact; one f32 rounding per add
    return acc, torch.from_numpy(acc).to(T)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_spmm_adds_in_entry_order_bit_for_bit(dt):
    """Both paths add a row's products in entry order, so the output is a function of the inputs alone.  64 rows of 128 entries, N = 16,
    magnitudes exp(3 N(0, 1)): the permuted list, the stably sorted list (in place), the forced build on it, and a list with duplicates
    equal the ordered f32 sum bit for bit, every element.  The check has teeth: the same sum in reversed order differs in more than half
    of the f32 elements (asserted below), one swapped pair of neighbours in about 1 %."""
    T, rows, per, cols, N = DT[dt], 64, 128, 300, 16
    g = np.random.default_rng(7)
    r0 = torch.from_numpy(np.repeat(np.arange(rows, dtype=np.int64), per))
    c0 = torch.from_numpy(g.integers(0, cols, size=rows * per))
    order = torch.from_numpy(g.permutation(rows * per))
    r, c = r0[order].contiguous(), c0[order].contiguous()
    v, d = _lognormal((rows * per,), T, 8), _lognormal((cols, N), T, 9)
    assert bool(torch.isfinite(v.float()).all()) and bool(torch.isfinite(d.float()).all())
    acc, want = _ordered_sum(r, c, v, d, rows, T)
    acc_rev, _ = _ordered_sum(r, c, v, d, rows, T, reverse=True)
    moved = float((acc.view(np.uint32) != acc_rev.view(np.uint32)).mean())
    print(f"\nspmm order {dt}: the reversed sum differs in {moved:.2f} of the f32 elements")
    assert moved >= 0.5, "the inputs must make the order visible"
    assert np.isfinite(acc).all() and bool(torch.isfinite(want.float()).all())
    dd = d.to(DEV)

    def run(rr, cc, vv, flags=0, kind=_sparse_native.COO_VALUES, scale=None):
        y, path, _ = _spmm_and_path(rr.to(DEV), cc.to(DEV), vv.to(DEV), kind, None if scale is None else scale.to(DEV), dd, rows, cols, T,
                                    "spmm_coo" if scale is None else "spmm_coo_int8", flags)
        return y, path

    def same(y, e, what):
        bad = int((_bits(y) != _bits(e)).sum())
        assert bad == 0, f"{what}: {bad} of {e.numel()} elements differ from the sum in entry order"

    y, path = run(r, c, v)
    assert path == 1 and _sparse_native.last_kernel() == "spmm_coo8"
    same(y, want, "permuted list")
    s = torch.argsort(r, stable=True)           # within a row still ascending list index: the same sums
    y, path = run(r[s].contiguous(), c[s].contiguous(), v[s].contiguous())
    assert path == 0
    same(y, want, "stably sorted list, in place")
    y, path = run(r[s].contiguous(), c[s].contiguous(), v[s].contiguous(), _sparse_native.FORCE_GENERIC)
    assert path == 1 and _sparse_native.last_kernel() == "spmm_coo8_general"
    same(y, want, "stably sorted list, forced build")
    r2, c2, v2 = torch.cat([r, r[::3]]), torch.cat([c, c[::3]]), torch.cat([v, v[::3]])
    o2 = torch.from_numpy(g.permutation(r2.numel()))
    r2, c2, v2 = r2[o2].contiguous(), c2[o2].contiguous(), v2[o2].contiguous()
    y, path = run(r2, c2, v2)
    assert path == 1
    same(y, _ordered_sum(r2, c2, v2, d, rows, T)[1], "list with duplicates")
    if T != torch.float32:
        # int8 codes with a scale per entry that T does not hold: the value is round_T(q * round_T(scale)), a T value whose product with
        # `dense` is exact again, so both roundings show bit for bit (in f32 the value has 24 bits and the product is not exact)
        q = torch.from_numpy(g.integers(-127, 128, size=rows * per).astype(np.int8))
        scale = torch.from_numpy((1e-3 * np.exp(g.standard_normal(rows * per))).astype(np.float32))
        assert float((scale.to(T).float() != scale).float().mean()) > 0.9
        v8 = emul.coo_int8_values(q, scale, T)
        y, path = run(r, c, q, kind=_sparse_native.COO_INT8_ENTRY, scale=scale)
        assert path == 1
        same(y, _ordered_sum(r, c, v8, d, rows, T)[1], "int8 codes with a scale per entry")
        y, path = run(r, c, q, kind=_sparse_native.COO_INT8_SCALAR, scale=scale[:1])
        same(y, _ordered_sum(r, c, emul.coo_int8_values(q, scale[:1], T), d, rows, T)[1], "int8 codes with one scale")


# ----------------------------------------------------------------------------- 5: memory safety
class _GuardedTorch:
    """`torch` as functional.py sees it here: every torch.empty is carved out of a larger 0xFF-filled buffer, 4 KiB of guard on each side."""
    GUARD = 4096

    def __init__(self):
        self.buffers = []

    def empty(self, *shape, dtype=torch.float32, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = int(np.prod(shape)) if len(shape) else 1
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((nbytes + 2 * self.GUARD,), 0xFF, dtype=torch.uint8, device=device)
        self.buffers.append((buf, nbytes))
        return buf[self.GUARD:self.GUARD + nbytes].view(dtype).view(shape)

    def __getattr__(self, name):
        return getattr(torch, name)

    def assert_guards_intact(self):
        assert self.buffers
        for buf, nbytes in self.buffers:
            assert bool((buf[:self.GUARD] == 0xFF).all()) and bool((buf[self.GUARD + nbytes:] == 0xFF).all()), "a guard band was written"


def _guarded_copy(proxy, t):
    out = proxy.empty(tuple(t.shape), dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


@pytest.mark.parametrize("index", ["sorted", "permuted"])
def test_out_of_range_indices_are_skipped_and_nothing_else_is_touched(monkeypatch, index):
    """Bad data for a bounds check, no fault: entries outside the sparse shape leave the output equal to the result without them, and the
    guard bands around every buffer (inputs, output, workspace) keep their fill."""
    T, rows, cols, N = torch.bfloat16, 200, 300, 64
    proxy = _GuardedTorch()
    monkeypatch.setattr(F, "torch", proxy)
    r, c = _lists(rows, cols, 0.1, index, 51)
    nnz = r.numel()
    v = synthetic.normal_device((nnz,), T, seed=52, device=DEV)
    d = synthetic.normal_device((cols, N), T, seed=53, device=DEV)
    bad = torch.arange(0, nnz, 7, device=DEV)
    r_bad, c_bad = r.clone(), c.clone()
    if index == "sorted":        # keep the list non-decreasing: rows below 0 in front, rows past the end behind
        r_bad[:5] = torch.tensor([-(2 ** 40), -7, -1, -1, -1], device=DEV)
        r_bad[-4:] = torch.tensor([rows, rows + 1, 2 ** 31, 2 ** 62], device=DEV)
    else:
        r_bad[bad[::2]] = torch.tensor([-1, rows, 2 ** 33, -(2 ** 50)], device=DEV).repeat(nnz)[:bad[::2].numel()]
    c_bad[bad[1::2]] = torch.tensor([cols, -1, 2 ** 31 + 5, -(2 ** 45), cols + 100000], device=DEV).repeat(nnz)[:bad[1::2].numel()]
    good = (r_bad >= 0) & (r_bad < rows) & (c_bad >= 0) & (c_bad < cols)
    assert int((~good).sum()) > 10
    y, path, _ = _spmm_and_path(_guarded_copy(proxy, r_bad), _guarded_copy(proxy, c_bad), _guarded_copy(proxy, v), _sparse_native.COO_VALUES, None,
                        _guarded_copy(proxy, d), rows, cols, T, "spmm_coo")
    assert path == (0 if index == "sorted" else 1)
    torch.cuda.synchronize()
    proxy.assert_guards_intact()
    y_good = bnb.spmm_coo(r_bad[good].contiguous(), c_bad[good].contiguous(), v[good].contiguous(), d, rows, cols)
    assert torch.equal(_bits(y), _bits(y_good)), "skipping the bad entries must give the bits of the list without them"
    _check_spmm(y, r_bad, c_bad, v, d, rows, T, "spmm_coo")
    proxy.assert_guards_intact()


def test_argument_errors_on_device_tensors():
    z = torch.zeros(3, dtype=torch.long, device=DEV)
    v, d = torch.zeros(3, device=DEV), torch.zeros(5, 2, device=DEV)
    with pytest.raises(ValueError, match="rows"):
        bnb.spmm_coo(z, z, v, d, 4, 4)
    with pytest.raises(ValueError, match="length"):
        bnb.spmm_coo(z[:2], z, v, d, 4, 5)
    with pytest.raises(ValueError, match="expected 1 or 3"):
        bnb.spmm_coo_int8(z, z, v.to(torch.int8), torch.ones(2, device=DEV), d, 4, 5, dtype=torch.float32)
    with pytest.raises(ValueError, match="Input must be 2D"):
        bnb.quantize_colrow(torch.zeros(2, 3, 4, device=DEV))
    with pytest.raises((RuntimeError, ValueError), match="nnz == 0"):
        bnb.quantize_sparse_coo(z[:0], z[:0], v[:0])
    assert bnb.spmm_coo(z, z, v, d, 4, 5).shape == (4, 2)       # and the same arguments with matching shapes pass


# ----------------------------------------------------------------------------- 6: the reference's tests/test_sparse.py scenarios
def _masked(M, K, sparsity, T, seed):
    x = synthetic.normal_device((M, K), T, seed=seed, device=DEV)
    u = synthetic.normal_device((M, K), torch.float32, seed=seed + 1, device=DEV)
    t = float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(0.5 + sparsity / 2.0)))
    return x * (u.abs() > t)


def test_scenario_small_known_products():
    for sparse, dense in [
        ([[1.0, 0.0, 2.0, 0.0], [0.0, 3.0, 0.0, 0.0], [0.0, 0.0, 0.0, 4.0]], [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]),
        ([[1.0, 0.0, 2.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]], [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]),      # an empty row
    ]:
        a, d = torch.tensor(sparse, device=DEV), torch.tensor(dense, device=DEV)
        r, c, v, M, K = bnb.sparse_coo_from_dense(a)
        y = bnb.spmm_coo(r, c, v, d, M, K)
        assert y.shape == (len(sparse), 2) and torch.allclose(y.cpu(), torch.tensor(sparse) @ torch.tensor(dense), atol=1e-3)
    assert not bool(y[1].any())
    one = torch.zeros(4, 4, device=DEV)
    one[2, 1] = 5.0
    d = synthetic.normal_device((4, 3), torch.float32, seed=3, device=DEV)
    r, c, v, M, K = bnb.sparse_coo_from_dense(one)
    assert v.numel() == 1 and torch.allclose(bnb.spmm_coo(r, c, v, d, M, K).cpu(), one.cpu() @ d.cpu(), atol=1e-3)


@pytest.mark.parametrize("M,K,N,sparsity,dt,atol", [(64, 128, 32, 0.9, "f32", 1e-3), (32, 64, 16, 0.8, "f16", 0.1), (64, 128, 32, 0.85, "f32", 1e-3),
                                                     (1000, 2000, 256, 0.95, "f32", 1e-3)])
def test_scenario_random_against_the_dense_product(M, K, N, sparsity, dt, atol):
    T = DT[dt]
    a = _masked(M, K, sparsity, T, 11)
    d = synthetic.normal_device((K, N), T, seed=13, device=DEV)
    r, c, v, rows, cols = bnb.sparse_coo_from_dense(a)
    y = bnb.spmm_coo(r, c, v, d, rows, cols)
    assert y.shape == (M, N) and not bool(torch.isnan(y).any())
    assert torch.allclose(y.double(), a.double() @ d.double(), atol=atol)


def test_scenario_int8_values():
    M, K, N = 32, 64, 16
    a = _masked(M, K, 0.8, torch.float32, 21)
    d = synthetic.normal_device((K, N), torch.float16, seed=23, device=DEV)
    r, c, v, rows, cols = bnb.sparse_coo_from_dense(a)
    ref = bnb.spmm_coo(r, c, v, d.float(), rows, cols)
    r8, c8, q, scale = bnb.quantize_sparse_coo(r, c, v)
    y8 = bnb.spmm_coo_int8(r8, c8, q, scale, d, rows, cols)
    assert y8.dtype == torch.float16 and y8.shape == (M, N) and bool(torch.isfinite(y8).all())
    assert float((ref.half() - y8).abs().float().mean() / ref.abs().mean()) < 0.15
    manual = bnb.spmm_coo(r8, c8, q.float() * scale.float(), d.float(), rows, cols)
    assert torch.allclose(y8.float(), manual, atol=1e-2)


def test_scenario_from_dense_and_quantize():
    a = torch.tensor([[1.0, 0.0, 2.0], [0.0, 3.0, 0.0]], device=DEV)
    r, c, v, M, K = bnb.sparse_coo_from_dense(a)
    assert (M, K) == (2, 3) and len(v) == 3
    back = torch.zeros(M, K, device=DEV)
    back[r, c] = v
    assert torch.equal(back, a)
    t = torch.tensor([[0.01, 0.5, -0.02], [1.0, 0.03, -2.0]], device=DEV)
    _, _, v, _, _ = bnb.sparse_coo_from_dense(t, threshold=0.1)
    assert len(v) == 3 and bool((v.abs() >= 0.1).all())
    assert len(bnb.sparse_coo_from_dense(torch.zeros(4, 4, device=DEV))[2]) == 0
    vals = synthetic.normal_device((100,), torch.float32, seed=41, device=DEV)
    idx = torch.arange(100, device=DEV) % 10
    _, _, q, scale = bnb.quantize_sparse_coo(idx, idx, vals)
    assert torch.allclose(vals, q.float() * scale.float(), atol=0.05, rtol=0.05)
    signs = torch.tensor([1.0, -1.0, 0.5, -0.5, 0.0], device=DEV)
    _, _, q, scale = bnb.quantize_sparse_coo(torch.zeros(5, dtype=torch.long, device=DEV), torch.arange(5, device=DEV), signs)
    assert torch.equal(torch.sign(q.float() * scale), torch.sign(signs))
