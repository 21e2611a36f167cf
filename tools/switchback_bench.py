#!/usr/bin/env python3
"""Cost of SwitchBackLinear's products (libmbnb_train.so) per shape, bf16: the forward (Wd pass + dense GEMM + bias pass), the forward
without a bias, dX = dY . weight_fp (mbnb_linear_grad_input, dense format), dW = dY^T . X (two transposing passes + dense GEMM), the Wd
pass alone against dequantize_rowwise, each transposing pass alone (with its HBM rate: bytes read + written), linear_dense at the
forward's shape and at dW's (the GEMM alone, for the overheads), and sync_weights.  Workspace allocation included, as the layer runs
them.  HIP events around `--steps` calls after `--warmup` calls, the median of `--reps` runs; one JSON line.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` separately (k_switchback_dq8, k_transpose_pad, k_bias_add, k_gemm_dense*)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _train_native, synthetic  # noqa: E402
from mps_bitsandbytes_amd import functional as F  # noqa: E402

# (name, M tokens, N out_features, K in_features)
SHAPES = [("4096x4096x4096", 4096, 4096, 4096), ("up 4096x11008x4096", 4096, 11008, 4096)]


def timed(fn, warmup, steps, reps):
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) * 1e3 / steps)
    return statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    out = {"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "warmup": args.warmup, "steps": args.steps, "reps": args.reps,
           "shapes": []}
    for name, M, N, K in SHAPES:
        m = bnb.SwitchBackLinear(K, N, compute_dtype=dt, device=dev)
        with torch.no_grad():
            m.weight_fp.copy_(synthetic.normal_device((N, K), dt, seed=1, std=0.02))
            m.bias.copy_(synthetic.normal_device((N,), dt, seed=4))
        m.sync_weights()
        x = synthetic.normal_device((M, K), dt, seed=2)
        dY = synthetic.normal_device((M, N), dt, seed=3)
        q, s, wfp, b = m.weight_int8, m.weight_scales, m.weight_fp.detach(), m.bias.detach()
        Mp = _train_native.padded_rows(M)
        ops = {
            "fwd": lambda: F._switchback_forward(x, q, s, b),
            "fwd_nobias": lambda: F._switchback_forward(x, q, s, None),
            "dx": lambda: F._grad_input(dY, F._FMT_DENSE, wfp, None, None, K, K, 0, dt, dt),
            "dw": lambda: F._linear_grad_weight(dY, x),
            "sb_pass": lambda: F._switchback_dequant(q, s, dt),
            "dequantize_rowwise": lambda: F.dequantize_rowwise(q, s, dt),
            "transpose_dY": lambda: F._transpose_pad(dY),
            "transpose_X": lambda: F._transpose_pad(x),
            "linear_dense_fwd": lambda: F.linear_dense(x, wfp),
            "sync": m.sync_weights,
        }
        row = {"shape": name, "M": M, "N": N, "K": K}
        kernels = {}
        for key, fn in ops.items():
            row[key + "_us"] = round(timed(fn, args.warmup, args.steps, args.reps), 2)
            if key in ("fwd", "dw"):
                kernels[key] = _train_native.last_kernel()
        # the GEMM of dW alone: the same call mbnb_linear_grad_weight makes on the transposed operands
        yt, xt = F._transpose_pad(dY), F._transpose_pad(x)
        row["gemm_dw_us"] = round(timed(lambda: F.linear_dense(yt, xt), args.warmup, args.steps, args.reps), 2)
        row["kernels"] = kernels
        row["bias_pass_us"] = round(row["fwd_us"] - row["fwd_nobias_us"], 2)
        row["sb_pass_over_dequantize_rowwise"] = round(row["sb_pass_us"] / row["dequantize_rowwise_us"], 3)
        row["transpose_dY_GBps"] = round((M * N * 2 + N * Mp * 2) / (row["transpose_dY_us"] * 1e-6) / 1e9, 1)
        row["transpose_X_GBps"] = round((M * K * 2 + K * Mp * 2) / (row["transpose_X_us"] * 1e-6) / 1e9, 1)
        row["dw_over_linear_dense_fwd"] = round(row["dw_us"] / row["linear_dense_fwd_us"], 3)
        out["shapes"].append(row)
        del m, x, dY, q, s, wfp, b, yt, xt, ops
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
