#!/usr/bin/env python3
"""
Measure the grouped expert GEMM on the block-scaled MFMA (libmbnb_moemx.so) against the grouped GEMM of §32 of the
same tree in the same process: whole Python calls, the quantiser launch of the new route included.

bf16, top-k 4, H = I = 2880; the gate / up shape (N = 5760, a token's slots share its row) and the down shape (N = 2880, a row per
pair); events around `--steps` calls after `--warmup`, the median of 5 repetitions and their spread.  Per shape also the relative
Frobenius error of each route against the f32 product over the dequantised weight, on the pairs of the first experts.

One JSON line per (E, T), printed and written to `--out` (default profiles/moemx_bench.jsonl).

    python tools/bench_mx_moemx.py [--steps 20] [--warmup 5] [--tokens 256,1024,4096,8192] [--experts 32,128] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mps_bitsandbytes_amd import _moemx_native, functional as F, synthetic  # noqa: E402
from tools.bench_mx_moegemm import HIDDEN, INTER, SLOTS, time_us  # noqa: E402


def rel_error(y, x, w, s, ids, experts=2):
    """|y - ref| / |ref| over the pairs of the first `experts` experts; ref = row . dequantize(W[e])^T in f32"""
    num = den = 0.0
    rows = x.reshape(-1, x.shape[-1]) if x.dim() == 3 else x.repeat_interleave(ids.shape[1], dim=0)
    for e in range(experts):
        at = (ids.reshape(-1) == e).nonzero().squeeze(1)
        ref = rows[at].float() @ F.dequantize_mx(w[e], s[e], "fp4", torch.float32).t()
        num += float((y.reshape(-1, y.shape[-1])[at].float() - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
    return (num / den) ** 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="256,1024,4096,8192", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moemx_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _moemx_native.lib()
    H, I, A = HIDDEN, INTER, SLOTS
    lines = []
    for E in (int(v) for v in args.experts.split(",")):
        weights = {}
        for name, (N, K) in (("gate_up", (2 * I, H)), ("down", (H, I))):
            w, s = F.quantize_mx(synthetic.normal_device((E * N, K), torch.bfloat16, seed=3 * E + N, device=dev) * 0.02, "fp4")
            weights[name] = (w.view(E, N, -1), s.view(E, N, -1))
        for T in (int(v) for v in args.tokens.split(",")):
            rng = np.random.default_rng(1000 * E + T)
            ids = torch.from_numpy(np.stack([rng.permutation(E)[:A] for _ in range(T)]).astype(np.int32)).to(dev)
            inputs = {"gate_up": synthetic.normal_device((T, H), torch.bfloat16, seed=8, device=dev),
                      "down": synthetic.normal_device((T, A, I), torch.bfloat16, seed=9, device=dev)}
            line = {"E": E, "shape": [T, A, H, I], "pairs": T * A, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                    "tile": [_moemx_native.ROW_TILE, _moemx_native.COL_TILE, _moemx_native.K_STEP]}
            with torch.no_grad():
                for name, x in inputs.items():
                    (w, s), res = weights[name], {}
                    flop = 2.0 * T * A * w.shape[1] * x.shape[-1]
                    for fmt in ("none", "fp8", "fp4"):
                        fn = lambda: F.matmul_mxfp4_experts_scaled(x, w, s, ids, act_format=fmt)
                        us, spread = time_us(fn, args.steps, args.warmup)
                        res[fmt] = {"us": round(us, 1), "tflops": round(flop / us * 1e-6, 1), "spread": round(spread, 3),
                                    "rel_error": round(rel_error(fn(), x, w, s, ids), 4)}
                    for fmt in ("fp8", "fp4"):
                        res[fmt]["to_none"] = round(res[fmt]["us"] / res["none"]["us"], 3)
                    line[name] = res
            print(json.dumps(line), flush=True)
            lines.append(line)
        del weights
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
