#!/usr/bin/env python
"""
Measure the MXFP4 expert linears (`matmul_mxfp4_experts`, k_mx_experts) against the only route the library had
before them, in one process: copy the router's ids to the host (which synchronises), then one
`matmul_mxfp4(..., act_format="none")` per distinct expert on the rows gathered for it, and an `index_copy_` back.

The method is tools/bench_mx_decode.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5),
five repetitions; the figures are whole Python calls (the allocation of the output included), so the baseline's host wait is inside
its figure.  The shapes are the two projections of a gpt-oss MLP block, bf16, A = 4 slots per token, T = 1, 2, 4, 8, 16 tokens with
seeded, uniformly drawn DISTINCT experts per token: gate / up (N, K) = (5760, 2880) on an input shared by a token's slots, and
down (2880, 2880) on a row per slot, each at E = 32 and at E = 128 (46 080 and 23 040 workgroups, most of them empty).  The codes
and scale bytes are random bytes (scale bytes 118 .. 126, no NaN block): the time does not depend on the values.

One JSON line per (E, form, T), printed and written to `--out` (default profiles/mx_experts_bench.jsonl): the microseconds of both
routes (the median of the five repetitions), their ratio (below 1: the one launch is faster), the spread of the five repetitions
of each route ((max - min) / median) and the larger of the two, the number of distinct experts, and the codes + scale bytes of the
distinct experts per second of the new call in GB/s.

    python tools/bench_mx_experts.py [--steps 20] [--warmup 5] [--tokens 1,2,4,8,16] [--experts 32,128] [--out FILE]
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
from mps_bitsandbytes_amd import _moe_native, _mx_native, synthetic  # noqa: E402

SLOTS = 4
FORMS = (("shared", 5760, 2880), ("slot", 2880, 2880))      # gate / up on the token's row; down on a row per slot


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


def per_expert_route(x, wc, ws, ids, per_slot):
    """What the library offered before k_mx_experts: ids to the host, a launch per distinct expert, an index-copy back."""
    T, A = ids.shape
    N, K = wc.shape[1], x.shape[-1]
    flat = ids.reshape(-1).cpu()                             # the device-to-host wait
    rows = x.reshape(T * A, K) if per_slot else x
    out = torch.empty(T * A, N, dtype=x.dtype, device=x.device)
    for e in torch.unique(flat).tolist():
        idx = (flat == e).nonzero().squeeze(1).to(x.device)
        y = bnb.matmul_mxfp4(rows.index_select(0, idx if per_slot else idx // A), wc[e], ws[e], act_format="none")
        out.index_copy_(0, idx, y)
    return out.view(T, A, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="1,2,4,8,16", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_experts_bench.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    _moe_native.lib(), _mx_native.lib()
    lines = []
    for E in (int(v) for v in args.experts.split(",")):
        for form, N, K in FORMS:
            g = torch.Generator(device=dev).manual_seed(31 * E + N)
            wc = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=g)
            ws = torch.randint(118, 127, (E, N, K // 32), dtype=torch.uint8, device=dev, generator=g)
            expert_bytes = N * (K // 2) + N * (K // 32)
            for T in (int(v) for v in args.tokens.split(",")):
                rng = np.random.default_rng(1000 * E + T)
                ids = torch.from_numpy(np.stack([rng.permutation(E)[:SLOTS] for _ in range(T)]).astype(np.int32)).to(dev)
                shape = (T, SLOTS, K) if form == "slot" else (T, K)
                x = synthetic.normal_device(shape, torch.bfloat16, seed=8, device=dev)
                distinct = int(torch.unique(ids).numel())
                with torch.no_grad():
                    new = bnb.matmul_mxfp4_experts(x, wc, ws, ids)
                    old = per_expert_route(x, wc, ws, ids, form == "slot")
                    # (an expert with ONE pair takes the per-expert route's FMA form: the same sum in another order, so no bit check)
                    assert float((new.float() - old.float()).abs().max()) <= 0.02 * float(old.float().abs().max()), "the two routes disagree"
                    new_us, new_spread = time_us(lambda: bnb.matmul_mxfp4_experts(x, wc, ws, ids), args.steps, args.warmup)
                    launch = _moe_native.last_launch()
                    old_us, old_spread = time_us(lambda: per_expert_route(x, wc, ws, ids, form == "slot"), args.steps, args.warmup)
                line = {"E": E, "form": form, "shape": [T, SLOTS, N, K], "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                        "distinct_experts": distinct, "workgroups": E * ((N + 15) // 16),
                        "experts": {"us": round(new_us, 2), "spread": round(new_spread, 3), "launch": launch,
                                    "weight_gbps": round(distinct * expert_bytes / new_us * 1e-3, 1)},
                        "per_expert": {"us": round(old_us, 2), "spread": round(old_spread, 3), "launches": distinct},
                        "experts_to_per_expert": round(new_us / old_us, 3), "spread": round(max(new_spread, old_spread), 3)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del wc, ws
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
