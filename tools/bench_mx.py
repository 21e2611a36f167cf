#!/usr/bin/env python
"""
Measure matmul_mxfp4 (both activation formats) against matmul_4bit NF4 bf16 of the same tree, in one process.

The method is bench.py's: HIP events around `--steps` launches (default 20) after `--warmup` untimed ones (default 5), the
median of 5 repetitions.  For each shape one JSON line: microseconds and TFLOP/s (2 M N K) of each path, and the ratio of the
MX step to the NF4 step (below 1: faster).  Then one JSON line with the relative Frobenius error of the two MX paths and of NF4
against the bf16 linear of the UNQUANTISED weight on the same data (N(0,1) activations, N(0, 0.02^2) weights).

The matmul_mxfp4 figures include its activation quantiser (two launches per call); matmul_4bit's include its dequantise pass
where it takes the decode-once path.

    python tools/bench_mx.py [--steps 20] [--warmup 5] [--shapes MxNxK,...]
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

DEFAULT_SHAPES = "4096x4096x4096,4096x11008x4096,1x4096x4096,8x4096x4096,64x4096x4096,512x4096x4096"


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
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated MxNxK")
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _mx_native.lib(), _native.lib()
    weights = {}
    for spec in args.shapes.split(","):
        M, N, K = (int(v) for v in spec.split("x"))
        if (N, K) not in weights:
            w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
            weights[(N, K)] = (w, bnb.quantize_mxfp4(w), bnb.quantize_nf4(w, blocksize=64))
        w, (wc, ws), (packed, state) = weights[(N, K)]
        x = synthetic.normal_device((M, K), torch.bfloat16, seed=8, device=dev)
        flop = 2.0 * M * N * K
        with torch.no_grad():
            nf4_us = time_us(lambda: bnb.matmul_4bit(x, packed, state), args.steps, args.warmup)
            nf4_kernel = _native.last_kernel()
            line = {"shape": [M, N, K], "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                    "nf4": {"us": round(nf4_us, 2), "tflops": round(flop / nf4_us * 1e-6, 1), "kernel": nf4_kernel}}
            for act in ("fp8", "fp4"):
                us = time_us(lambda: bnb.matmul_mxfp4(x, wc, ws, act_format=act), args.steps, args.warmup)
                line["mx_" + act] = {"us": round(us, 2), "tflops": round(flop / us * 1e-6, 1), "ratio_to_nf4": round(us / nf4_us, 3),
                                     "launch": _mx_native.last_launch()}
        print(json.dumps(line), flush=True)
    # accuracy on the first shape's weight, 512 rows
    (N, K), (w, (wc, ws), (packed, state)) = next(iter(weights.items()))
    x = synthetic.normal_device((512, K), torch.bfloat16, seed=9, device=dev)
    with torch.no_grad():
        ref = x.double() @ w.double().t()
        acc = {"accuracy": "relative Frobenius error against the bf16 linear of the unquantised weight, in float64", "shape": [512, N, K],
               "nf4": rel_fro(bnb.matmul_4bit(x, packed, state), ref),
               "mx_fp8": rel_fro(bnb.matmul_mxfp4(x, wc, ws, act_format="fp8"), ref),
               "mx_fp4": rel_fro(bnb.matmul_mxfp4(x, wc, ws, act_format="fp4"), ref),
               "mxfp4_weight_only": rel_fro(x.double() @ bnb.dequantize_mxfp4(wc, ws, torch.float32).double().t(), ref)}
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in acc.items()}), flush=True)


if __name__ == "__main__":
    main()
