#!/usr/bin/env python
"""
Measure the weight-only decode of a block-scaled FP8 weight against the two routes such a weight had at decode row
counts, in one process: `linear_fp8_block` (the quantiser and the 128 x 128 GEMM: two launches) and torch.matmul over a kept bf16
copy of the dequantised weight.

The method is tools/bench_fp8.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5), bf16 in
and out; every route of a shape is timed once per repetition, the routes in turn, 5 repetitions; a figure is the median of its 5 and
`spread` its (max - min) / median.  The figures are of whole Python calls.  For each shape one JSON line with, in microseconds,
`weight_only` (linear_fp8_block_weight_only), `linear` (linear_fp8_block) and `torch_kept`, the launch text of the new route, the
ratios, and `weight_gb_per_s_of_call`: the weight's N x K bytes over the time of the whole call (NOT a kernel rate: the call's host
side is inside it).  The timed calls read the same weight back to back, so every figure of every route is a warm-cache figure
(16 MB and 50 MB fit the Infinity Cache), not an HBM streaming rate.

    python tools/bench_fp8_decode.py [--steps 20] [--warmup 5] [--shapes MxNxK,...] [--out profiles/fp8_decode_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _fp8dec_native, synthetic  # noqa: E402
from tools.bench_fp8 import REPS, time_routes  # noqa: E402
from tools.bench_fp8_block import dequantise  # noqa: E402

# the projection shapes of Qwen3-8B-FP8 at decode row counts
DEFAULT_SHAPES = ",".join(f"{M}x{N}x{K}" for N, K in ((4096, 4096), (12288, 4096), (4096, 12288)) for M in (1, 2, 4, 8, 16, 32, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated MxNxK")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _fp8dec_native.lib()
    lines, weights = [], {}
    for spec in args.shapes.split(","):
        M, N, K = (int(v) for v in spec.split("x"))
        if (N, K) not in weights:
            wq, ws = bnb.quantize_fp8_blocks(synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev))
            weights = {(N, K): (wq, ws, dequantise(wq, ws))}         # one weight and its 16-bit copy at a time
        wq, ws, kept = weights[(N, K)]
        x = synthetic.normal_device((M, K), torch.bfloat16, seed=8, device=dev)
        routes = {
            "weight_only": lambda: bnb.linear_fp8_block_weight_only(x, wq, ws),
            "linear": lambda: bnb.linear_fp8_block(x, wq, ws),
            "torch_kept": lambda: torch.matmul(x, kept.t()),
        }
        got = time_routes(routes, args.steps, args.warmup)
        bnb.linear_fp8_block_weight_only(x, wq, ws)
        line = {"shape": [M, N, K], "kernel": _fp8dec_native.last_launch(), "steps": args.steps, "warmup": args.warmup, "reps": REPS}
        for name, (us, spread) in got.items():
            line[name + "_us"], line[name + "_spread"] = round(us, 2), round(spread, 3)
        line["weight_gb_per_s_of_call"] = round(N * K / got["weight_only"][0] * 1e-3, 1)
        line["weight_only_vs_linear"] = round(got["weight_only"][0] / got["linear"][0], 3)
        line["weight_only_vs_torch_kept"] = round(got["weight_only"][0] / got["torch_kept"][0], 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
