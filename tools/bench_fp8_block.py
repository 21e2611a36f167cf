#!/usr/bin/env python
"""
Measure the block-scaled FP8 linear against the per-row W8A8 FP8 linear of the same tree and against the only
route a block-scaled checkpoint had before it, in one process.

The method is tools/bench_fp8.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5), bf16
in and out; every route of a shape is timed once per repetition, the routes in turn, 5 repetitions; a figure is the median of its 5
and `spread` its (max - min) / median.  For each shape one JSON line with, in microseconds: `quant` (quantize_fp8_groups), `gemm`
(matmul_fp8_block alone), `linear` (linear_fp8_block whole), `rows_gemm` / `rows_linear` (matmul_fp8_w8a8 / linear_fp8_w8a8: the same
pipeline without the fold), `torch_dequant` (expand weight_scale_inv, dequantise the weight to bf16 with torch ops, torch.matmul)
and `torch_kept` (torch.matmul over that 16-bit copy, kept), and the ratios.  Then one JSON line with the relative Frobenius error
of linear_fp8_block and of linear_fp8_w8a8 against the bf16 linear of the UNQUANTISED weight on 512 rows.

    python tools/bench_fp8_block.py [--steps 20] [--warmup 5] [--shapes MxNxK,...] [--out profiles/fp8_block_bench.jsonl]
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
from mps_bitsandbytes_amd import _fp8blk_native, synthetic  # noqa: E402
from tools.bench_fp8 import DEFAULT_SHAPES, REPS, rel_fro, time_routes  # noqa: E402


def dequantise(wq, ws):
    """the torch route: weight_scale_inv expanded to [N, K], the codes decoded, their product in bf16"""
    N, K = wq.shape
    s = ws.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K]
    return (wq.view(torch.float8_e4m3fn).float() * s).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated MxNxK")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _fp8blk_native.lib()
    lines, weights = [], {}
    for spec in args.shapes.split(","):
        M, N, K = (int(v) for v in spec.split("x"))
        if (N, K) not in weights:
            w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
            weights[(N, K)] = (bnb.quantize_fp8_blocks(w), bnb.quantize_fp8_rows(w))
        (wq, ws), (rq, rs) = weights[(N, K)]
        kept = dequantise(wq, ws)
        x = synthetic.normal_device((M, K), torch.bfloat16, seed=8, device=dev)
        xq, xs = bnb.quantize_fp8_groups(x)
        xrq, xrs = bnb.quantize_fp8_rows(x)
        routes = {
            "quant": lambda: bnb.quantize_fp8_groups(x),
            "gemm": lambda: bnb.matmul_fp8_block(xq, xs, wq, ws, None, torch.bfloat16),
            "linear": lambda: bnb.linear_fp8_block(x, wq, ws),
            "rows_gemm": lambda: bnb.matmul_fp8_w8a8(xrq, xrs, rq, rs, None, torch.bfloat16),
            "rows_linear": lambda: bnb.linear_fp8_w8a8(x, rq, rs),
            "torch_dequant": lambda: torch.matmul(x, dequantise(wq, ws).t()),
            "torch_kept": lambda: torch.matmul(x, kept.t()),
        }
        got = time_routes(routes, args.steps, args.warmup)
        bnb.linear_fp8_block(x, wq, ws)
        line = {"shape": [M, N, K], "kernel": _fp8blk_native.last_launch(), "steps": args.steps, "warmup": args.warmup, "reps": REPS}
        for name, (us, spread) in got.items():
            line[name + "_us"], line[name + "_spread"] = round(us, 2), round(spread, 3)
        for name in ("gemm", "linear"):
            line[name + "_tflops"] = round(2.0 * M * N * K / got[name][0] * 1e-6, 1)
        line["gemm_vs_rows_gemm"] = round(got["gemm"][0] / got["rows_gemm"][0], 3)          # the cost of the fold (and of this tile)
        line["linear_vs_rows_linear"] = round(got["linear"][0] / got["rows_linear"][0], 3)
        line["linear_vs_torch_dequant"] = round(got["linear"][0] / got["torch_dequant"][0], 3)
        line["linear_vs_torch_kept"] = round(got["linear"][0] / got["torch_kept"][0], 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    N, K = 4096, 4096
    w = synthetic.normal_device((N, K), torch.bfloat16, seed=7, std=0.02, device=dev)
    x = synthetic.normal_device((512, K), torch.bfloat16, seed=9, device=dev)
    ref = torch.nn.functional.linear(x, w)                   # the bf16 linear of the unquantised weight
    lines.append({"accuracy_rows": 512, "shape": [512, N, K],
                  "rel_fro_linear_fp8_block": rel_fro(bnb.linear_fp8_block(x, *bnb.quantize_fp8_blocks(w)), ref),
                  "rel_fro_linear_fp8_w8a8": rel_fro(bnb.linear_fp8_w8a8(x, *bnb.quantize_fp8_rows(w)), ref),
                  "rel_fro_torch_dequant_of_the_blocks": rel_fro(torch.matmul(x, dequantise(*bnb.quantize_fp8_blocks(w)).t()), ref)})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
