#!/usr/bin/env python
"""
Measure the prefill-sized grouped GEMM over MXFP4 experts (libmbnb_moegemm.so) against the route the library took
before it, in one process: the decode launches of §28 / §29 (k_mx_experts_rt, k_routed_sum), cut over the tokens into calls of at
most 1024 pairs.  That route is the existing functions with `functional.MOE_GROUPED_MIN_PAIRS = None`; the grouped route is the
three `matmul_mxfp4_experts_grouped*` functions, and `moe_mlp_mxfp4` with the threshold at 1 pair.  Both routes give the same bits,
which is asserted at every size before anything is timed.

The method is tools/bench_mx_moe_mlp.py's: HIP events around `--steps` whole Python calls (default 20) after `--warmup` untimed ones
(default 5), five repetitions, the median and the spread (max - min) / median.  The shapes are the MLP block of gpt-oss: bf16,
H = I = 2880, A = 4 slots per token, seeded uniformly drawn DISTINCT experts per token, at E = 32 and E = 128, T = 64 .. 8192.
Codes and scale bytes are random bytes (scale bytes 118 .. 126, no NaN block): the time does not depend on the values.

Per (E, T) three projections: gate / up + GLU (5760 x 2880), down + sum (2880 x 2880) and the whole moe_mlp_mxfp4; for each the
time of both routes, their ratio and 2 P N K / time of the grouped route in TFLOP/s.

One JSON line per (E, T), printed and written to `--out` (default profiles/moegemm_bench.jsonl).

    python tools/bench_mx_moegemm.py [--steps 20] [--warmup 5] [--tokens 64,256,512,1024,4096,8192] [--experts 32,128] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _moegemm_native, functional as F, synthetic  # noqa: E402

SLOTS, HIDDEN, INTER = 4, 2880, 2880


def time_us(fn, steps, warmup, reps=5):
    """(the median of `reps` repetitions in microseconds per call, their spread (max - min) / median)"""
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
    med = statistics.median(vals)
    return med, (max(vals) - min(vals)) / med


def pair(new, old, flop):
    (n, ns), (o, os_) = new, old
    return {"grouped_us": round(n, 1), "parent_us": round(o, 1), "grouped_to_parent": round(n / o, 3), "spread": round(max(ns, os_), 3),
            "grouped_tflops": round(flop / n * 1e-6, 1)}


def with_threshold(value, fn):
    def run():
        F.MOE_GROUPED_MIN_PAIRS = value
        return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="64,256,512,1024,4096,8192", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moegemm_bench.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _moegemm_native.lib()
    H, I, A = HIDDEN, INTER, SLOTS
    shipped = F.MOE_GROUPED_MIN_PAIRS
    lines = []
    for E in (int(v) for v in args.experts.split(",")):
        g = torch.Generator(device=dev).manual_seed(37 * E)
        wgu = torch.randint(0, 256, (E, 2 * I, H // 2), dtype=torch.uint8, device=dev, generator=g)
        sgu = torch.randint(118, 127, (E, 2 * I, H // 32), dtype=torch.uint8, device=dev, generator=g)
        wd = torch.randint(0, 256, (E, H, I // 2), dtype=torch.uint8, device=dev, generator=g)
        sd = torch.randint(118, 127, (E, H, I // 32), dtype=torch.uint8, device=dev, generator=g)
        bgu = synthetic.normal_device((E, 2 * I), torch.bfloat16, seed=9, device=dev)
        bd = synthetic.normal_device((E, H), torch.bfloat16, seed=10, device=dev)
        for T in (int(v) for v in args.tokens.split(",")):
            rng = np.random.default_rng(1000 * E + T)
            ids = torch.from_numpy(np.stack([rng.permutation(E)[:A] for _ in range(T)]).astype(np.int32)).to(dev)
            rw = torch.softmax(synthetic.normal_device((T, A), torch.float32, seed=11, device=dev), dim=1)
            x = synthetic.normal_device((T, H), torch.bfloat16, seed=8, device=dev) * 0.05
            P = T * A
            with torch.no_grad():
                F.MOE_GROUPED_MIN_PAIRS = None
                h = bnb.matmul_mxfp4_experts_glu(x, wgu, sgu, ids, bgu)
                routes = {
                    "gate_up_glu": (lambda: bnb.matmul_mxfp4_experts_grouped_glu(x, wgu, sgu, ids, bgu),
                                    with_threshold(None, lambda: bnb.matmul_mxfp4_experts_glu(x, wgu, sgu, ids, bgu)), 2.0 * P * 2 * I * H),
                    "down_sum": (lambda: bnb.matmul_mxfp4_experts_grouped_sum(h, wd, sd, ids, rw, bd),
                                 with_threshold(None, lambda: bnb.matmul_mxfp4_experts_sum(h, wd, sd, ids, rw, bd)), 2.0 * P * H * I),
                    "moe_mlp": (with_threshold(1, lambda: bnb.moe_mlp_mxfp4(x, wgu, sgu, bgu, wd, sd, bd, ids, rw)),
                                with_threshold(None, lambda: bnb.moe_mlp_mxfp4(x, wgu, sgu, bgu, wd, sd, bd, ids, rw)), 2.0 * P * 3 * I * H),
                }
                line = {"E": E, "shape": [T, A, H, I], "pairs": P, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                        "row_tile": _moegemm_native.ROW_TILE, "col_tile": _moegemm_native.TILE_N,
                        "workgroups_gate_up": -(-2 * I // _moegemm_native.TILE_N) * _moegemm_native.max_tiles(min(P, F.MOE_GROUPED_MAX_PAIRS), E)}
                for name, (new_fn, old_fn, flop) in routes.items():
                    assert torch.equal(new_fn().view(torch.int16), old_fn().view(torch.int16)), f"{name}: the two routes disagree"
                    line[name] = pair(time_us(new_fn, args.steps, args.warmup), time_us(old_fn, args.steps, args.warmup), flop)
                del h
            print(json.dumps(line), flush=True)
            lines.append(line)
        del wgu, sgu, wd, sd
        torch.cuda.empty_cache()
    F.MOE_GROUPED_MIN_PAIRS = shipped
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
