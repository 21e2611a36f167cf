#!/usr/bin/env python3
"""Cost of the input gradient of matmul_4bit against its forward: per shape the forward matmul_4bit, dX = dY . dequant(W) through
mbnb_linear_grad_input (transposed dequantise pass + dense GEMM, workspace allocation included, as the backward runs it), the
transposed pass alone, and dX / forward.  HIP events around `--steps` calls after `--warmup` calls, the median of `--reps` runs; one
JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` separately (k_dequant_t, k_dequantize_4bit_flat,
k_gemm_dense*)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mps_bitsandbytes_amd import _native, synthetic  # noqa: E402
from mps_bitsandbytes_amd import functional as F  # noqa: E402

# (name, M, N, K, double quant): NF4 bf16, blocksize 64
SHAPES = [("4096x4096x4096", 4096, 4096, 4096, False), ("up 4096x11008x4096", 4096, 11008, 4096, True),
          ("down 4096x4096x11008", 4096, 4096, 11008, True), ("512x4096x4096", 512, 4096, 4096, False)]


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
    out = {"device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "steps": args.steps, "reps": args.reps, "shapes": []}
    for name, M, N, K, dq in SHAPES:
        W = synthetic.normal_device((N, K), dt, seed=1, std=0.05)
        packed, st = F.quantize_4bit(W, blocksize=64, compress_statistics=dq, quant_type="nf4")
        del W
        x = synthetic.normal_device((M, K), dt, seed=2)
        dY = synthetic.normal_device((M, N), dt, seed=3)
        keep: list = []
        desc = F._absmax_desc(st.absmax, st.state2, keep)

        def fwd():
            return F.matmul_4bit(x, packed, st)

        def dx():
            return F._grad_input(dY, _native.NF4, packed, desc, None, K, K, 64, dt, dt)

        def pass_t():
            return F._dequantize_t(packed, st)

        t_fwd = timed(fwd, args.warmup, args.steps, args.reps)
        fwd()
        k_fwd = _native.last_kernel()
        t_dx = timed(dx, args.warmup, args.steps, args.reps)
        dx()
        k_dx = _native.last_kernel()
        t_pass = timed(pass_t, args.warmup, args.steps, args.reps)
        out["shapes"].append({"shape": name, "M": M, "N": N, "K": K, "double_quant": dq, "fwd_us": round(t_fwd, 2), "fwd_kernel": k_fwd,
                              "dx_us": round(t_dx, 2), "dx_kernel": k_dx, "dx_over_fwd": round(t_dx / t_fwd, 3),
                              "transpose_pass_us": round(t_pass, 2),
                              "transpose_pass_GBps": round((N * K // 2 + N * K * 2) / (t_pass * 1e-6) / 1e9, 1)})
        del x, dY, packed, st, keep, desc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
