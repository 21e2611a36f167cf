#!/usr/bin/env python3
"""matmul_4bit_grouped and matmul_4bit_lora_grouped on 2 to 16 rows (libmbnb_batch.so: one launch per group, two with adapters) against
the forms these row counts took before: matmul_4bit per member, and with adapters the composed form per member (matmul_4bit plus four
torch launches).  The baseline never runs the new code.  Prints one JSON line per shape, row count and rank (and appends it to --out).

Shapes (bf16 NF4):  qkv = 3 x [4096, 4096];  gate_up = 2 x [11008, 4096];  qkv_dq = qkv with double-quantised absmax; each at --rows
(2, 8, 16) and --ranks (0 = no adapters, 16, 64; scaling 2 / r).  Each shape rotates over --sets (64) distinct weight AND adapter sets,
so both come from HBM and not from the Infinity Cache (as tools/group_bench.py and tools/lora_bench.py do).

  device   one linear chain of the 64 steps captured into a HIP graph per form (one stream, no parallel branches); a sample is the
           mean of --replays (20) replays between two device events, and the forms are sampled ALTERNATELY, --reps (5) samples each.
           Reported per group (replay time / sets): the median, and the spread (max - min) of the samples.

`ok` says that fused beats the baseline by more than the two spreads together, and that the outputs agree on the first set: bit for
bit without adapters, within 2^-6 of the largest magnitude with them (bf16, five roundings against one).

    python tools/batch_bench.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _batch_native, synthetic  # noqa: E402
from mps_bitsandbytes_amd.functional import _lora_composed  # noqa: E402
from tools.group_bench import SHAPES, capture, replay_us, summary  # noqa: E402


def run(name, rows, ranks, args):
    Ns, K, nested = SHAPES[name]
    dt, dev = torch.bfloat16, torch.device("cuda:0")
    sets = []
    for s in range(args.sets):
        members = []
        for g, N in enumerate(Ns):
            W = synthetic.normal_device((N, K), dt, seed=7000 + 16 * s + g, device=dev)
            members.append(bnb.quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=nested))
            del W
        sets.append(members)
    lines = []
    for r in ranks:
        adapters = None
        if r > 0:
            adapters = [[(synthetic.normal_device((r, K), dt, seed=9000 + 16 * s + g, device=dev),
                          synthetic.normal_device((N, r), dt, seed=9500 + 16 * s + g, device=dev), 2.0 / r) for g, N in enumerate(Ns)]
                        for s in range(args.sets)]
        for M in rows:
            x = synthetic.normal_device((M, K), dt, seed=6999, device=dev)

            def fused_one(s):
                if adapters is None:
                    return bnb.matmul_4bit_grouped(x, sets[s])
                return bnb.matmul_4bit_lora_grouped(x, sets[s], adapters[s])

            def baseline_one(s):      # what these row counts ran before: member by member
                if adapters is None:
                    return tuple(bnb.matmul_4bit(x, p, st) for p, st in sets[s])
                return tuple(_lora_composed(x, p, st, None, ad, None) for (p, st), ad in zip(sets[s], adapters[s]))

            def fused():
                for s in range(args.sets):
                    fused_one(s)

            def baseline():
                for s in range(args.sets):
                    baseline_one(s)

            with torch.no_grad():
                _batch_native.reset_launch_log()
                got = fused_one(0)
                want = [(len(Ns), M, K, dt)] if adapters is None else [(len(Ns), r * len(Ns), M, K, dt)]
                assert _batch_native.launch_log == want, f"{name} M={M} r={r}: not one fused call: {_batch_native.launch_log}"
                form = _batch_native.last_launch()
                ref = baseline_one(0)
                assert _batch_native.launch_log == want, "the baseline ran the new code"
                if adapters is None:
                    agree = all(torch.equal(y, c) for y, c in zip(got, ref))
                else:
                    agree = all(float((y.float() - c.float()).abs().max()) <= 2.0 ** -6 * float(c.float().abs().max()) for y, c in zip(got, ref))
                for _ in range(3):
                    fused()
                    baseline()
                torch.cuda.synchronize()
                graphs = {"baseline": capture(baseline), "fused": capture(fused)}
                samples = {k: [] for k in graphs}
                for _ in range(args.reps):           # alternating: what else runs on the machine hits every form alike
                    for k, graph in graphs.items():
                        samples[k].append(replay_us(graph, args.replays))
            dev_us = {k: summary(v, args.sets) for k, v in samples.items()}
            f, b = dev_us["fused"], dev_us["baseline"]
            lines.append({"shape": name, "members": list(Ns), "K": K, "M": M, "r": r, "dtype": "bf16", "quant_type": "nf4", "double_quant": nested,
                          "sets": args.sets, "form": form, "agree": agree, "baseline_form": "matmul_4bit per member" if r == 0 else "composed per member",
                          "device": {"fused": f, "baseline": b, "ratio": round(f["median_us"] / b["median_us"], 4),
                                     "saved_us_per_group": round(b["median_us"] - f["median_us"], 3),
                                     "note": f"one graph of {args.sets} steps per form, median of {args.reps} x {args.replays} replays, alternating"},
                          "ok": bool(agree and f["median_us"] + f["spread_us"] + b["spread_us"] < b["median_us"])})
            del graphs
            torch.cuda.empty_cache()
        del adapters
    del sets
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="qkv,gate_up,qkv_dq")
    ap.add_argument("--rows", default="2,8,16")
    ap.add_argument("--ranks", default="0,16,64")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batch_bench.py needs a GPU"
    for name in args.shapes.split(","):
        for result in run(name, [int(m) for m in args.rows.split(",")], [int(r) for r in args.ranks.split(",")], args):
            line = json.dumps(result)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
