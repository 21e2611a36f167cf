#!/usr/bin/env python3
"""
Golden vectors for the col+row INT8 and COO sparse operations, captured by RUNNING THE REFERENCE's Python CPU path
(mps_bitsandbytes/functional.py), data only (same rules as make_golden.py).  The reference checkout is the first argument:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_int8_decomp.py /path/to/mps-bitsandbytes

Inputs are small and ship with the results (bit patterns), so a test needs nothing but the file:
- "cr" cases: quantize_colrow (codes, both statistics) and dequantize_colrow into f16 / bf16 / f32, for f16 / bf16 / f32 inputs on ragged
  and aligned shapes, a zero row, a zero column, 1 x C and R x 1, rows and columns spread log-normally over several orders of
  magnitude, a NaN and an Inf;
- "mm" cases: matmul_colrow with 2-D / 3-D / 1-D inputs, with and without bias;
- "fd" cases: sparse_coo_from_dense at thresholds 0 and > 0, with NaN, +-Inf, -0.0, the f16 value 0.1 rounds to and its two
  neighbours, an all-zero matrix;
- "qs" cases: quantize_sparse_coo;
- "sp" cases: spmm_coo and spmm_coo_int8 (one scale, and one scale per entry) for the three dtypes with sorted, permuted, int32 and
  duplicate-carrying index lists, with empty rows, and one with 170-180 entries per row.
While it writes them the script asserts that tests/int8_decomp_emul.py explains every col+row result: statistics bit-equal, each
code and each Wd element equal to the chain evaluated with s or with the next f32 below s.
Writes g12_int8_decomp.npz (bit patterns) and manifest_int8_decomp.json (case list) next to this file.
"""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from mps_bitsandbytes_amd import synthetic  # noqa: E402
from tests import int8_decomp_emul as emul  # noqa: E402

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}

# quantize_colrow: (R, C, dtype, kind)
SPECS_CR = [
    (37, 53, "f32", "spread"), (32, 64, "f16", "spread"), (40, 72, "bf16", "spread"), (33, 100, "f16", "plain"),
    (16, 48, "bf16", "zero_row_col"), (1, 77, "f32", "plain"), (90, 1, "f16", "plain"), (24, 40, "f32", "nan"), (24, 40, "bf16", "inf"),
    (48, 96, "bf16", "spread"),
]
# matmul_colrow: (lead shape of the input, N, K, dtype, bias)
SPECS_MM = [((7,), 40, 100, "f16", True), ((3, 5), 72, 136, "bf16", True), ((), 24, 64, "f32", True), ((33,), 64, 128, "bf16", False),
            ((5,), 48, 72, "f32", False)]
# spmm: (rows, cols, N, dtype, density, index kind)
SPECS_SP = [
    (12, 20, 8, "f32", 0.3, "sorted"), (12, 20, 8, "f16", 0.3, "permuted"), (17, 33, 10, "bf16", 0.25, "int32"),
    (9, 14, 16, "f16", 0.4, "duplicates"), (20, 16, 5, "f32", 0.1, "permuted"), (6, 700, 16, "f16", 0.25, "sorted"),
    (6, 700, 16, "bf16", 0.25, "permuted"), (5, 700, 16, "f32", 0.25, "duplicates"),
]


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.numpy().copy()


def colrow_input(R, C, dt, kind, seed):
    x = synthetic.normal((R, C), torch.float32, seed=seed, std=0.05)
    if kind == "spread":     # rows and columns scaled log-normally: several orders of magnitude
        x = x * torch.exp(2.0 * synthetic.normal((R, 1), torch.float32, seed=seed + 1)) * torch.exp(2.0 * synthetic.normal((1, C), torch.float32, seed=seed + 2))
    x = x.to(DT[dt])
    if kind == "zero_row_col":
        x[3, :] = 0
        x[:, 5] = 0
    if kind == "nan":
        x[2, 7] = float("nan")
    if kind == "inf":
        x[4, 9] = float("-inf")
    return x


def spmm_lists(rows, cols, density, kind, seed):
    """(row, col) index lists: a random pattern in row-major order, then permuted / narrowed to int32 / given duplicates."""
    u = synthetic.uniform_u64(rows * cols, seed).astype(np.float64) / 2.0 ** 64
    mask = torch.from_numpy(u < density).view(rows, cols)
    mask[rows // 2, :] = False          # an empty row
    idx = mask.nonzero()
    r, c = idx[:, 0].contiguous(), idx[:, 1].contiguous()
    if kind in ("permuted", "duplicates"):
        if kind == "duplicates":
            r, c = torch.cat([r, r[::3]]), torch.cat([c, c[::3]])
        perm = torch.from_numpy(np.argsort(synthetic.uniform_u64(r.numel(), seed + 1), kind="stable"))
        r, c = r[perm].contiguous(), c[perm].contiguous()
    if kind == "int32":
        r, c = r.to(torch.int32), c.to(torch.int32)
    return r, c


def main(reference):
    sys.path.insert(0, reference)
    import mps_bitsandbytes as ref  # noqa: E402  (the reference, CPU path)
    from mps_bitsandbytes import functional as RF  # noqa: E402

    arrays, cases = {}, []
    # ---- quantize_colrow / dequantize_colrow
    for ci, (R, C, dt, kind) in enumerate(SPECS_CR):
        seed = 1400 + 10 * ci
        x = colrow_input(R, C, dt, kind, seed)
        q, rm, cm = RF.quantize_colrow(x)
        arrays[f"cr{ci}_x"], arrays[f"cr{ci}_q"], arrays[f"cr{ci}_rm"], arrays[f"cr{ci}_cm"] = bits(x), bits(q), bits(rm), bits(cm)
        e_rm, e_cm = emul.colrow_stats(x)
        assert np.array_equal(bits(rm), e_rm.view(np.uint32)) and np.array_equal(bits(cm), e_cm.view(np.uint32)), ("statistics", ci)
        s, s_low = emul.colrow_scale(e_rm, e_cm), emul.colrow_scale(e_rm, e_cm, lower=True)
        ok = emul.explained(q, torch.from_numpy(emul.colrow_codes(x, s)), torch.from_numpy(emul.colrow_codes(x, s_low)))
        assert bool(ok.all()), ("codes", ci, int((~ok).sum()))
        for t in ("f16", "bf16", "f32"):
            wd = RF.dequantize_colrow(q, rm, cm, DT[t])
            arrays[f"cr{ci}_wd_{t}"] = bits(wd)
            ok = emul.explained(wd, emul.colrow_wd(q.numpy(), s, DT[t]), emul.colrow_wd(q.numpy(), s_low, DT[t]))
            assert bool(ok.all()), ("Wd", ci, t, int((~ok).sum()))
        cases.append(dict(kind="colrow", id=ci, R=R, C=C, dtype=dt, data=kind))
    # ---- matmul_colrow
    for ci, (lead, N, K, dt, has_bias) in enumerate(SPECS_MM):
        seed = 1500 + 10 * ci
        w = colrow_input(N, K, "f32", "spread" if ci % 2 == 0 else "plain", seed)
        q, rm, cm = RF.quantize_colrow(w)
        x = synthetic.normal(lead + (K,), torch.float32, seed=seed + 3)
        b = synthetic.normal((N,), torch.float32, seed=seed + 4) if has_bias else None
        y = RF.matmul_colrow(x, q, rm, cm, b, DT[dt])
        arrays[f"mm{ci}_q"], arrays[f"mm{ci}_rm"], arrays[f"mm{ci}_cm"] = bits(q), bits(rm), bits(cm)
        arrays[f"mm{ci}_x"], arrays[f"mm{ci}_y"] = bits(x), bits(y)
        if has_bias:
            arrays[f"mm{ci}_b"] = bits(b)
        cases.append(dict(kind="matmul_colrow", id=ci, lead=list(lead), N=N, K=K, dtype=dt, bias=has_bias))
    # ---- sparse_coo_from_dense
    fd = []
    x = synthetic.normal((9, 13), torch.float32, seed=1600)
    x[x.abs() < 0.6] = 0
    x[0, 1], x[2, 3], x[4, 5], x[6, 7] = float("nan"), float("inf"), float("-inf"), -0.0
    fd += [("f32", x, 0.0), ("f32", x, 0.9), ("bf16", x.to(torch.bfloat16), 0.0), ("bf16", x.to(torch.bfloat16), 0.75)]
    near = torch.tensor([0x2E65, 0x2E66, 0x2E67], dtype=torch.int16).view(torch.float16)     # 0.0999755859375 (what 0.1 rounds to) and its neighbours
    h = synthetic.normal((4, 10), torch.float16, seed=1601, std=0.2)
    h[1, 2:5] = near
    h[2, 6:9] = -near
    h[3, 0] = float("nan")
    fd += [("f16", h, 0.1), ("f16", h, 0.0), ("f32", torch.zeros(5, 6), 0.0), ("f16", torch.zeros(3, 4, dtype=torch.float16), 0.5)]
    for ci, (dt, x, thr) in enumerate(fd):
        r, c, v, rows, cols = RF.sparse_coo_from_dense(x, thr)
        arrays[f"fd{ci}_x"], arrays[f"fd{ci}_row"], arrays[f"fd{ci}_col"], arrays[f"fd{ci}_val"] = bits(x), bits(r), bits(c), bits(v)
        er, ec, ev = emul.coo_from_dense(x, thr)
        assert torch.equal(er, r) and torch.equal(ec, c) and torch.equal(emul.bits(ev), emul.bits(v)), ("from_dense", ci)
        cases.append(dict(kind="from_dense", id=ci, dtype=dt, threshold=thr, rows=rows, cols=cols, nnz=int(v.numel())))
    # ---- quantize_sparse_coo
    for ci, (n, dt, std) in enumerate([(100, "f32", 1.0), (333, "f16", 0.02), (64, "bf16", 30.0), (5, "f32", 0.0)]):
        v = synthetic.normal((n,), DT[dt], seed=1700 + ci, std=std)
        r = torch.arange(n) % 7
        _, _, q, scale = RF.quantize_sparse_coo(r, r, v)
        arrays[f"qs{ci}_v"], arrays[f"qs{ci}_q"], arrays[f"qs{ci}_scale"] = bits(v), bits(q), bits(scale)
        eq, es = emul.coo_quantize(v)
        assert torch.equal(eq, q) and torch.equal(emul.bits(es), emul.bits(scale)), ("quantize_sparse_coo", ci)
        cases.append(dict(kind="quantize_sparse_coo", id=ci, n=n, dtype=dt))
    # ---- spmm_coo / spmm_coo_int8
    for ci, (rows, cols, N, dt, density, kind) in enumerate(SPECS_SP):
        seed = 1800 + 10 * ci
        T = DT[dt]
        r, c = spmm_lists(rows, cols, density, kind, seed)
        v = synthetic.normal((r.numel(),), T, seed=seed + 2)
        d = synthetic.normal((cols, N), T, seed=seed + 3)
        y = RF.spmm_coo(r, c, v, d, rows, cols)
        _, _, q, scale = RF.quantize_sparse_coo(r, c, v)
        y8 = RF.spmm_coo_int8(r, c, q, scale, d, rows, cols, dtype=T)
        per = (scale * (1.0 + 0.25 * synthetic.normal((r.numel(),), torch.float32, seed=seed + 4))).abs()
        y8e = RF.spmm_coo_int8(r, c, q, per, d, rows, cols, dtype=T)
        for k, t in (("row", r), ("col", c), ("val", v), ("dense", d), ("y", y), ("q", q), ("scale", scale), ("y8", y8), ("per", per), ("y8e", y8e)):
            arrays[f"sp{ci}_{k}"] = bits(t)
        cases.append(dict(kind="spmm", id=ci, rows=rows, cols=cols, N=N, dtype=dt, index=kind, nnz=int(r.numel())))
    np.savez_compressed(os.path.join(HERE, "g12_int8_decomp.npz"), **arrays)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (CPU path)" % ref.__version__, torch=torch.__version__,
                                    generated=time.strftime("%Y-%m-%d"), script="tests/golden/make_golden_int8_decomp.py"), g12=cases)
    with open(os.path.join(HERE, "manifest_int8_decomp.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g12_int8_decomp.npz:", len(cases), "cases,", os.path.getsize(os.path.join(HERE, "g12_int8_decomp.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
