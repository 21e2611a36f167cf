#!/usr/bin/env python
"""
Measure the W8A8 FP8 linear against the other 8-bit and 4-bit linears of the same tree, in one process.

The method is bench.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5), bf16 in and
out.  Every route of a shape is timed once per repetition, the routes in turn (alternated), 5 repetitions; a route's figure is the
median of its 5 and `spread` its (max - min) / median.  For each shape one JSON line with, in microseconds: `w8a16`
(matmul_fp8_e4m3), `int8` (matmul_int8 over the same shape), `nf4` (matmul_4bit), `quant` (quantize_fp8_rows alone), `gemm`
(matmul_fp8_w8a8 alone) and `linear` (linear_fp8_w8a8 whole), and the TFLOP/s (2 M N K) of `gemm` and `linear`.  Then one JSON line
with the relative Frobenius error of linear_fp8_w8a8 and of matmul_fp8_e4m3 against the bf16 linear of the UNQUANTISED weight on
512 rows (N(0,1) activations, N(0, 0.02^2) weights), and one with what v_mfma_scale_f32_16x16x128_f8f6f4 returns for an E4M3 NaN
code in either operand.  With --out the lines are also written to that file.

    python tools/bench_fp8.py [--steps 20] [--warmup 5] [--shapes MxNxK,...] [--out profiles/fp8_bench.jsonl]
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
from mps_bitsandbytes_amd import _fp8_native, _native, synthetic  # noqa: E402

DEFAULT_SHAPES = "4096x4096x4096,4096x11008x4096,512x4096x4096,64x4096x4096"
REPS = 5


def time_routes(routes, steps, warmup):
    """{name: (median us, spread)}: every route warmed up, then REPS rounds over the routes in turn"""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    vals = {name: [] for name in routes}
    for _ in range(REPS):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            vals[name].append(e0.elapsed_time(e1) / steps * 1e3)
    return {name: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for name, v in vals.items()}


def rel_fro(y, ref):
    y, ref = y.double(), ref.double()
    return float((y - ref).norm() / ref.norm())


def nan_code_probe(dev):
    """one NaN code (0x7F) in activation row 3 / weight row 5 of a 16 x 16 x 128 problem of ones: where the NaNs come out"""
    ones = torch.full((16, 128), 0x38, dtype=torch.uint8, device=dev)
    s = torch.ones(16, device=dev)
    out = {}
    for name, (ra, rw) in (("in_a", (3, None)), ("in_w", (None, 5))):
        a, w = ones.clone(), ones.clone()
        if ra is not None:
            a[ra, 70] = 0x7F
        if rw is not None:
            w[rw, 9] = 0xFF
        y = bnb.matmul_fp8_w8a8(a, s, w, s, None, torch.float32)
        nan = torch.isnan(y)
        out[name] = {"nan_rows": sorted(set(nan.nonzero()[:, 0].tolist())), "nan_cols": sorted(set(nan.nonzero()[:, 1].tolist())),
                     "others_are_128": bool((y[~nan] == 128.0).all())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated MxNxK")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _fp8_native.lib(), _native.lib()
    lines, weights = [], {}
    for spec in args.shapes.split(","):
        M, N, K = (int(v) for v in spec.split("x"))
        if (N, K) not in weights:
            w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
            wi, wis = bnb.quantize_rowwise(w)
            weights[(N, K)] = (bnb.quantize_fp8_rows(w), bnb.quantize_fp8_e4m3(w), (wi.t().contiguous(), wis), bnb.quantize_nf4(w, blocksize=64))
        (wq, ws), (we, wes), (wi_t, wis), (packed, state) = weights[(N, K)]
        x = synthetic.normal_device((M, K), torch.bfloat16, seed=8, device=dev)
        xq, xs = bnb.quantize_fp8_rows(x)
        xi, xis = bnb.quantize_rowwise(x)
        routes = {
            "w8a16": lambda: bnb.matmul_fp8_e4m3(x, we, wes, None, torch.bfloat16),
            "int8": lambda: bnb.matmul_int8(xi, wi_t, xis, wis, dtype=torch.bfloat16),
            "nf4": lambda: bnb.matmul_4bit(x, packed, state),
            "quant": lambda: bnb.quantize_fp8_rows(x),
            "gemm": lambda: bnb.matmul_fp8_w8a8(xq, xs, wq, ws, None, torch.bfloat16),
            "linear": lambda: bnb.linear_fp8_w8a8(x, wq, ws),
        }
        got = time_routes(routes, args.steps, args.warmup)
        line = {"shape": [M, N, K], "kernel": _fp8_native.last_launch(), "steps": args.steps, "warmup": args.warmup, "reps": REPS}
        for name, (us, spread) in got.items():
            line[name + "_us"], line[name + "_spread"] = round(us, 2), round(spread, 3)
        for name in ("gemm", "linear"):
            line[name + "_tflops"] = round(2.0 * M * N * K / got[name][0] * 1e-6, 1)
        line["gemm_vs_int8"] = round(got["gemm"][0] / got["int8"][0], 3)
        line["linear_vs_w8a16"] = round(got["linear"][0] / got["w8a16"][0], 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    N, K = 4096, 4096
    w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
    x = synthetic.normal_device((512, K), torch.bfloat16, seed=9, device=dev)
    ref = torch.nn.functional.linear(x, w)                   # the bf16 linear of the unquantised weight
    lines.append({"accuracy_rows": 512, "shape": [512, N, K],
                  "rel_fro_linear_fp8_w8a8": rel_fro(bnb.linear_fp8_w8a8(x, *bnb.quantize_fp8_rows(w)), ref),
                  "rel_fro_matmul_fp8_e4m3": rel_fro(bnb.matmul_fp8_e4m3(x, *bnb.quantize_fp8_e4m3(w), None, torch.bfloat16), ref),
                  "rel_fro_linear_fp8_w8a8_over_the_reference_encoders_weight": rel_fro(bnb.linear_fp8_w8a8(x, *bnb.quantize_fp8_e4m3(w)), ref)})
    print(json.dumps(lines[-1]), flush=True)
    lines.append({"nan_code_probe": nan_code_probe(dev)})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
