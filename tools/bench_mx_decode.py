#!/usr/bin/env python
"""
Measure the weight-only MXFP4 decode linear (`matmul_mxfp4(..., act_format="none")`, k_mx_decode) against the
quantising route (`act_format="fp8"`) and matmul_4bit NF4 bf16 of the same tree, in one process.

The method is tools/bench_mx.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5), the
median of 5 repetitions; the figures are whole Python calls (allocation of the output, and of the fp8 route's workspace,
included).  For each N x K and each M one JSON line: microseconds of the three paths, the ratios of `none` to the other two
(below 1: faster), the last-launch text, and the weight bytes (codes + scale bytes) per second of the `none` call in GB/s.
Then one JSON line with the relative Frobenius error of `none`, `fp8` and NF4 against the bf16 linear of the UNQUANTISED weight
on the same data (N(0, 1) activations, N(0, 0.02^2) weights).

    python tools/bench_mx_decode.py [--steps 20] [--warmup 5] [--rows 1,2,4,8,16] [--shapes NxK,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _mx_native, _native, synthetic  # noqa: E402

DEFAULT_SHAPES = "4096x4096,11008x4096,5120x2880"
DEFAULT_ROWS = "1,2,4,8,16"


def time_us(fn, steps, warmup, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    vals = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        vals.append(e0.elapsed_time(e1) / steps * 1e3)
    return statistics.median(vals)


def rel_fro(y, ref):
    y, ref = y.double(), ref.double()
    return float((y - ref).norm() / ref.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default=DEFAULT_ROWS, help="comma-separated M")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated NxK")
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _mx_native.lib(), _native.lib()
    first = None
    for spec in args.shapes.split(","):
        N, K = (int(v) for v in spec.split("x"))
        w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
        wc, ws = bnb.quantize_mxfp4(w)
        nf4 = bnb.quantize_nf4(w, blocksize=64) if K % 64 == 0 else None
        first = first or (N, K, w, wc, ws, nf4)
        weight_bytes = wc.numel() + ws.numel()
        for M in (int(v) for v in args.rows.split(",")):
            x = synthetic.normal_device((M, K), torch.bfloat16, seed=8, device=dev)
            with torch.no_grad():
                none_us = time_us(lambda: bnb.matmul_mxfp4(x, wc, ws, act_format="none"), args.steps, args.warmup)
                launch = _mx_native.last_launch()
                fp8_us = time_us(lambda: bnb.matmul_mxfp4(x, wc, ws, act_format="fp8"), args.steps, args.warmup)
                line = {"shape": [M, N, K], "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                        "none": {"us": round(none_us, 2), "launch": launch, "weight_gbps": round(weight_bytes / none_us * 1e-3, 1)},
                        "mx_fp8": {"us": round(fp8_us, 2), "launch": _mx_native.last_launch()},
                        "none_to_fp8": round(none_us / fp8_us, 3)}
                if nf4 is not None:
                    nf4_us = time_us(lambda: bnb.matmul_4bit(x, nf4[0], nf4[1]), args.steps, args.warmup)
                    line["nf4"] = {"us": round(nf4_us, 2), "kernel": _native.last_kernel()}
                    line["none_to_nf4"] = round(none_us / nf4_us, 3)
            print(json.dumps(line), flush=True)
    N, K, w, wc, ws, nf4 = first
    x = synthetic.normal_device((16, K), torch.bfloat16, seed=9, device=dev)
    with torch.no_grad():
        ref = x.double() @ w.double().t()
        acc = {"accuracy": "relative Frobenius error against the bf16 linear of the unquantised weight, in float64", "shape": [16, N, K],
               "none": rel_fro(bnb.matmul_mxfp4(x, wc, ws, act_format="none"), ref),
               "mx_fp8": rel_fro(bnb.matmul_mxfp4(x, wc, ws, act_format="fp8"), ref)}
        if nf4 is not None:
            acc["nf4"] = rel_fro(bnb.matmul_4bit(x, nf4[0], nf4[1]), ref)
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in acc.items()}), flush=True)


if __name__ == "__main__":
    main()
