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
from tests import int8_decomp_cases as cases_mod
from tests import int8_decomp_emul as emul
from tests.elementwise import UNIT, assert_bound_elementwise, assert_linear_elementwise, linear_bound
from tests.goldenio import DT, HERE, from_bits
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


def _shifted(t, view):
    """t itself, or a copy one element off 16-byte alignment (view == "misaligned")."""
    if view != "misaligned":
        return t
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _spread(R, C, T, seed):
    """A matrix whose rows and columns are scaled log-normally (several orders of magnitude), made on the device."""
    x = synthetic.normal_device((R, C), torch.float32, seed=seed, std=0.05, device=DEV)
    x = x * torch.exp(1.5 * synthetic.normal_device((R, 1), torch.float32, seed=seed + 1, device=DEV))
    x = x * torch.exp(1.5 * synthetic.normal_device((1, C), torch.float32, seed=seed + 2, device=DEV))
    return x.to(T)


def _check_quantize(x_dev, kernel=None):
    """quantize_colrow and dequantize_colrow (three dtypes) of x against the emulation, bit for bit; returns (q, rm, cm) on the device."""
    q, rm, cm = bnb.quantize_colrow(x_dev)
    if kernel is not None:
        assert _sparse_native.last_kernel() == kernel
    R, C = x_dev.shape
    assert q.dtype == torch.int8 and q.shape == (R, C) and rm.dtype == cm.dtype == torch.float32 and rm.shape == (R,) and cm.shape == (C,)
    x = x_dev.cpu()
    e_rm, e_cm = emul.colrow_stats(x)
    assert np.array_equal(rm.cpu().numpy().view(np.uint32), e_rm.view(np.uint32)), "row statistics differ from the emulation"
    assert np.array_equal(cm.cpu().numpy().view(np.uint32), e_cm.view(np.uint32)), "column statistics differ from the emulation"
    s = emul.colrow_scale(e_rm, e_cm)
    e_q = emul.colrow_codes(x, s)
    bad = int((q.cpu().numpy() != e_q).sum())
    assert bad == 0, f"{bad} of {q.numel()} codes differ from the emulation"
    return q, rm, cm, s, e_q


def _check_dequant(q, rm, cm, T, s=None, kernel=None, route=None):
    wd = F._colrow_dequant_pass(q, rm, cm, T) if route == "pass" else bnb.dequantize_colrow(q, rm, cm, T)
    if kernel is not None:
        assert _sparse_native.last_kernel() == kernel
    assert wd.dtype == T and wd.shape == q.shape
    if s is None:
        s = emul.colrow_scale(rm.cpu().numpy(), cm.cpu().numpy())
    e_wd = emul.colrow_wd(q.cpu().numpy(), s, T)
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
    """(out, path) of functional._spmm_coo: path is the first int32 of the workspace the call allocated, 0 where the device found
    `row_indices` non-decreasing and used the list in place, 1 where it built the CSR form.  The workspace is the call's last uint8
    allocation; it is caught on its way through the `torch` proxy that functional.py sees under this module's fixtures."""
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
    return out, int(seen[-1][:4].view(torch.int32).item())


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
@pytest.mark.parametrize("case", cases_mod.CASES, ids=cases_mod.case_id)
def test_case(case):
    T = DT[case["dt"]]
    op, kernel = case["op"], case["kernel"]
    seed = 2100 + sum(map(ord, cases_mod.case_id(case))) % 997
    if op == "quantize":
        x = _shifted(_spread(case["R"], case["C"], T, seed), case.get("view"))
        _check_quantize(x, kernel)
        return
    if op == "dequant":
        R, C = case["R"], case["C"]
        q = synthetic.int8_tensor((R, C), seed=seed).to(DEV)
        rm = synthetic.normal_device((R,), torch.float32, seed=seed + 1, device=DEV).abs().clamp_min(1e-8)
        cm = synthetic.normal_device((C,), torch.float32, seed=seed + 2, device=DEV).abs().clamp_min(1e-8)
        _check_dequant(q, rm, cm, T, kernel=kernel, route=case.get("route"))
        return
    if op == "matmul":
        N, K = case["N"], case["K"]
        lead = tuple(case["lead"]) if "lead" in case else (case["M"],)
        q, rm, cm = bnb.quantize_colrow(_spread(N, K, torch.float32, seed))
        x = _shifted(synthetic.normal_device(lead + (K,), T, seed=seed + 3, device=DEV), case.get("view"))
        b = synthetic.normal_device((N,), T, seed=seed + 4, device=DEV) if case.get("bias") else None
        flags = _sparse_native.FORCE_GENERIC if case.get("generic") else 0
        y = F._matmul_colrow(x, q, rm, cm, b, T, flags)
        assert _sparse_native.last_kernel() == kernel
        assert y.shape == lead + (N,) and y.dtype == T
        wd = emul.colrow_wd(q.cpu().numpy(), emul.colrow_scale(rm.cpu().numpy(), cm.cpu().numpy()), T)
        assert_linear_elementwise(y.reshape(-1, N), x.reshape(-1, K), wd, b, T, T, kernel)
        return
    if op in ("count", "from_dense"):
        R, C, thr = case["R"], case["C"], case.get("threshold", 0.0)
        x = synthetic.normal_device((R, C), T, seed=seed, device=DEV)
        if case["density"] < 1:
            keep = synthetic.normal_device((R, C), torch.float32, seed=seed + 1, device=DEV).abs() > float(
                torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - case["density"] / 2.0)))
            x = x * keep
        er, ec, ev = emul.coo_from_dense(x.cpu(), thr)
        if op == "count":
            _, _, row_ptr = F._coo_row_ptr(x, thr)
            assert _sparse_native.last_kernel() == kernel
            want = torch.zeros(R + 1, dtype=torch.int64)
            want[1:] = torch.cumsum(torch.bincount(er, minlength=R), 0)
            assert torch.equal(row_ptr.cpu(), want)
            return
        r, c, v, rows, cols = bnb.sparse_coo_from_dense(x, thr)
        assert _sparse_native.last_kernel() == kernel
        assert (rows, cols) == (R, C) and r.dtype == c.dtype == torch.int64 and v.dtype == T
        assert torch.equal(r.cpu(), er) and torch.equal(c.cpu(), ec) and torch.equal(_bits(v), _bits(ev))
        return
    if op == "quantize_coo":
        n = case["n"]
        v = synthetic.normal_device((n,), T, seed=seed, std=0.37, device=DEV)
        idx = torch.arange(n, device=DEV)
        r, c, q, scale = bnb.quantize_sparse_coo(idx, idx, v)
        assert _sparse_native.last_kernel() == kernel
        assert r is idx and c is idx and q.dtype == torch.int8 and q.shape == (n,) and scale.dtype == torch.float32 and scale.shape == (1,)
        eq, es = emul.coo_quantize(v.cpu())
        assert torch.equal(q.cpu(), eq) and torch.equal(_bits(scale), _bits(es))
        return
    assert op == "spmm"
    rows, cols, N = case["rows"], case["cols"], case["N"]
    r, c = _lists(rows, cols, case["density"], case["index"], seed)
    nnz = r.numel()
    vals = synthetic.normal_device((nnz,), T, seed=seed + 2, device=DEV)
    dense = _shifted(synthetic.normal_device((cols, N), T, seed=seed + 3, device=DEV), case.get("view"))
    flags = _sparse_native.FORCE_GENERIC if case.get("generic") else 0
    if case["values"] == "T":
        y, path = _spmm_and_path(r, c, vals, _sparse_native.COO_VALUES, None, dense, rows, cols, T, "spmm_coo", flags)
        used = vals
    else:
        q = synthetic.int8_tensor((max(nnz, 1),), seed=seed + 4)[:nnz].to(DEV)
        scale = torch.tensor([0.0123], device=DEV) if case["values"] == "int8" else synthetic.normal_device((nnz,), torch.float32, seed=seed + 5, std=0.01, device=DEV)
        kind = _sparse_native.COO_INT8_SCALAR if case["values"] == "int8" else _sparse_native.COO_INT8_ENTRY
        y, path = _spmm_and_path(r, c, q, kind, scale, dense, rows, cols, T, "spmm_coo_int8", flags)
        used = emul.coo_int8_values(q.cpu(), scale.cpu(), T).to(DEV)
    assert _sparse_native.last_kernel() == kernel
    assert path == (1 if case.get("generic") or case["index"] in ("permuted", "duplicates") else 0), "the device took the other path"
    if nnz == 0:
        assert not bool(_bits(y).any())
    _check_spmm(y, r, c, used, dense, rows, T, kernel)


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
    y_fast, path = _spmm_and_path(rs, cs, vs, _sparse_native.COO_VALUES, None, d, rows, cols, T, "spmm_coo")
    assert _sparse_native.last_kernel() == "spmm_coo8" and path == 0
    y_gen, path = _spmm_and_path(rs, cs, vs, _sparse_native.COO_VALUES, None, d, rows, cols, T, "spmm_coo", _sparse_native.FORCE_GENERIC)
    assert _sparse_native.last_kernel() == "spmm_coo8_general" and path == 1
    assert torch.equal(_bits(y_fast), _bits(y_gen)), "both paths sum a row's entries in entry order"
    # sorted by row, the order within a row is the permuted list's order too (stable sort), so all three agree bit for bit
    assert torch.equal(_bits(y_fast), _bits(runs[0]))
    _check_spmm(y_fast, rs, cs, vs, d, rows, T, "spmm_coo8")


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
    y, path = _spmm_and_path(_guarded_copy(proxy, r_bad), _guarded_copy(proxy, c_bad), _guarded_copy(proxy, v), _sparse_native.COO_VALUES, None,
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
