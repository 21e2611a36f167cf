#!/usr/bin/env python3
"""Cost of the col+row INT8 and COO sparse operations (libmbnb_sparse.so), each next to its yardstick measured in the same process:

- quantize_colrow / dequantize_colrow at 4096 x 4096 and 4096 x 11008, bf16, against a device-to-device copy that moves the same number
  of bytes (the matrix is read twice by design: 2 R C sizeof(T) + R C for quantize, R C + R C sizeof(T) for dequantize); quantize_rowwise
  and dequantize_rowwise for orientation;
- matmul_colrow against linear_int8 at 4096^3 and 4096 x 11008 x 4096, bf16: the whole op, its decode pass alone (dequantize_colrow /
  dequantize_rowwise) and the dense GEMM alone (linear_dense on the decoded weight: the same kernel on the same shape for both);
- spmm_coo, f16, at 1000 x 2000 x 256 and 4096 x 4096 x 4096 at 5 % and 0.1 % density, sorted and permuted index lists: time and the
  effective bandwidth against the bytes it must move (nnz rows of `dense` + the output); torch.sparse.mm on the same device, in f32 (it has no f16
  form here), as a context figure, labelled vendor library.

HIP events around `--steps` calls after `--warmup` calls; the arms of a group are interleaved (every repetition times each arm once) and
the median of `--reps` repetitions is reported, with the spread (min, max) of the yardstick.  One JSON line.  Kernel times: run it
under `rocprofv3 --kernel-trace --stats` separately (k_colrow_*, k_spmm_csr, k_coo_*, k_gemm_dense*)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _native, _sparse_native, synthetic  # noqa: E402
from mps_bitsandbytes_amd import functional as F  # noqa: E402

DEV = torch.device("cuda:0")


def time_once(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def interleaved(arms, args):
    """{name: fn} -> {name: (median, min, max)} in microseconds per call; every repetition times each arm once, in turn."""
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    runs = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            runs[k].append(time_once(fn, args.steps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def copy_arm(nbytes_moved):
    """A device-to-device copy that moves `nbytes_moved` bytes in all (half read, half written)."""
    src = torch.empty(nbytes_moved // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def colrow_rows(args):
    rows, dt = [], torch.bfloat16
    for R, C in ((4096, 4096), (4096, 11008)):
        x = synthetic.normal_device((R, C), dt, seed=1, std=0.02, device=DEV)
        q, rm, cm = bnb.quantize_colrow(x)
        q_bytes, dq_bytes = 2 * R * C * 2 + R * C, R * C + R * C * 2
        qr, sr = bnb.quantize_rowwise(x)
        t = interleaved({
            "quantize_colrow": lambda: bnb.quantize_colrow(x), "copy_q": copy_arm(q_bytes), "quantize_rowwise": lambda: bnb.quantize_rowwise(x),
            "dequantize_colrow": lambda: bnb.dequantize_colrow(q, rm, cm, dt), "copy_dq": copy_arm(dq_bytes),
            "dequantize_rowwise": lambda: bnb.dequantize_rowwise(qr, sr, dt),
        }, args)
        row = {"R": R, "C": C, "dtype": "bf16", "quantize_kernel": "colrow_quantize8", "quantize_bytes": q_bytes, "dequantize_bytes": dq_bytes}
        for k, (med, lo, hi) in t.items():
            row[k + "_us"] = round(med, 2)
        row["copy_q_spread_us"] = [round(t["copy_q"][1], 2), round(t["copy_q"][2], 2)]
        row["quantize_colrow_copy_fraction"] = round(t["copy_q"][0] / t["quantize_colrow"][0], 3)
        row["dequantize_colrow_copy_fraction"] = round(t["copy_dq"][0] / t["dequantize_colrow"][0], 3)
        row["quantize_rowwise_copy_fraction"] = round(copy_fraction_rowwise(t, R, C), 3)
        rows.append(row)
        del x, q, rm, cm, qr, sr
        torch.cuda.empty_cache()
    return rows


def copy_fraction_rowwise(t, R, C):
    """quantize_rowwise reads the matrix once or twice depending on its route; scale the measured copy to R C (2 + 1) bytes, one read."""
    per_byte = t["copy_q"][0] / (2 * R * C * 2 + R * C)
    return per_byte * (R * C * 2 + R * C) / t["quantize_rowwise"][0]


def matmul_rows(args):
    rows, dt = [], torch.bfloat16
    for M, N, K in ((4096, 4096, 4096), (4096, 11008, 4096)):
        w = synthetic.normal_device((N, K), dt, seed=2, std=0.02, device=DEV)
        x = synthetic.normal_device((M, K), dt, seed=3, device=DEV)
        q, rm, cm = bnb.quantize_colrow(w)
        qr, sr = bnb.quantize_rowwise(w)
        wd = bnb.dequantize_colrow(q, rm, cm, dt)
        wr = bnb.dequantize_rowwise(qr, sr, dt)
        arms = {
            "matmul_colrow": lambda: bnb.matmul_colrow(x, q, rm, cm, None, dt), "linear_int8": lambda: bnb.linear_int8(x, qr, sr, None, dt),
            "colrow_pass": lambda: bnb.dequantize_colrow(q, rm, cm, dt), "rowwise_pass": lambda: bnb.dequantize_rowwise(qr, sr, dt),
            "gemm_on_colrow_weight": lambda: F.linear_dense(x, wd), "gemm_on_rowwise_weight": lambda: F.linear_dense(x, wr),
        }
        t = interleaved(arms, args)
        bnb.matmul_colrow(x, q, rm, cm, None, dt)
        k_colrow = _sparse_native.last_kernel()
        bnb.linear_int8(x, qr, sr, None, dt)
        row = {"M": M, "N": N, "K": K, "dtype": "bf16", "matmul_colrow_kernel": k_colrow, "linear_int8_kernel": _native.last_kernel()}
        for k, (med, lo, hi) in t.items():
            row[k + "_us"] = round(med, 2)
        row["linear_int8_spread_us"] = [round(t["linear_int8"][1], 2), round(t["linear_int8"][2], 2)]
        row["gemm_spread_us"] = [round(t["gemm_on_rowwise_weight"][1], 2), round(t["gemm_on_rowwise_weight"][2], 2)]
        row["matmul_colrow_over_linear_int8"] = round(t["matmul_colrow"][0] / t["linear_int8"][0], 3)
        rows.append(row)
        del w, x, q, rm, cm, qr, sr, wd, wr, arms
        torch.cuda.empty_cache()
    return rows


def spmm_rows(args):
    rows, dt = [], torch.float16
    for (R, Kc, N) in ((1000, 2000, 256), (4096, 4096, 4096)):
        for density in (0.05, 0.001):
            a = synthetic.normal_device((R, Kc), dt, seed=5, device=DEV)
            u = synthetic.normal_device((R, Kc), torch.float32, seed=6, device=DEV)
            thr = float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - density / 2.0)))
            a = a * (u.abs() > thr)
            r, c, v, _, _ = bnb.sparse_coo_from_dense(a)
            nnz = v.numel()
            perm = torch.argsort(synthetic.normal_device((nnz,), torch.float32, seed=7, device=DEV))
            rp, cp, vp = r[perm].contiguous(), c[perm].contiguous(), v[perm].contiguous()
            d = synthetic.normal_device((Kc, N), dt, seed=8, device=DEV)
            # the vendor library has no f16 sparse product on this device: its arm runs in f32 (twice the bytes per element)
            sp, d32 = torch.sparse_coo_tensor(torch.stack([r, c]), v.float(), (R, Kc)).coalesce(), d.float()
            moved = nnz * N * 2 + R * N * 2
            t = interleaved({
                "sorted": lambda: bnb.spmm_coo(r, c, v, d, R, Kc), "permuted": lambda: bnb.spmm_coo(rp, cp, vp, d, R, Kc),
                "copy": copy_arm(moved), "from_dense": lambda: bnb.sparse_coo_from_dense(a),
                "vendor_torch_sparse_mm_f32": lambda: torch.sparse.mm(sp, d32),
            }, args)
            row = {"rows": R, "cols": Kc, "N": N, "density": density, "nnz": nnz, "dtype": "f16", "bytes": moved}
            for k, (med, lo, hi) in t.items():
                row[k + "_us"] = round(med, 2)
            row["sorted_GBps"] = round(moved / (t["sorted"][0] * 1e-6) / 1e9, 1)
            row["permuted_GBps"] = round(moved / (t["permuted"][0] * 1e-6) / 1e9, 1)
            row["copy_GBps"] = round(moved / (t["copy"][0] * 1e-6) / 1e9, 1)
            rows.append(row)
            del a, u, r, c, v, rp, cp, vp, d, sp, d32
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["colrow", "matmul", "spmm"], default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(DEV), "warmup": args.warmup, "steps": args.steps, "reps": args.reps}
    if args.only in (None, "colrow"):
        out["colrow"] = colrow_rows(args)
    if args.only in (None, "matmul"):
        out["matmul"] = matmul_rows(args)
    if args.only in (None, "spmm"):
        out["spmm"] = spmm_rows(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
