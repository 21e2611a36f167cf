#!/usr/bin/env python3
"""matmul_4bit_lora_grouped (two launches per group) against the composed form of the parent commit -- matmul_4bit_grouped plus the
torch adapter expression per member -- and, for scale, against the adapter-free grouped launch; prints one JSON line per shape and
rank (and appends it to --out).

Shapes (bf16 NF4, one activation row):  qkv = 3 x [4096, 4096];  gate_up = 2 x [11008, 4096];  qkv_dq = qkv with double-quantised
absmax; each at --ranks (16, 64) with scaling 2 / r.  Each shape rotates over --sets (64) distinct weight AND adapter sets, so both
come from HBM and not from the Infinity Cache (as tools/group_bench.py does).

  device   one linear chain of the 64 steps captured into a HIP graph per form (one stream, no parallel branches); a sample is the
           mean of --replays (20) replays between two device events, and the forms are sampled ALTERNATELY, --reps (5) samples each.
           Reported per group (replay time / sets): the median, and the spread (max - min) of the samples.

`fused` is one mbnb_lora_gemv4 call per group (the binding's log is checked); `composed` is 1 + 4 G launches; `grouped` has no
adapters at all.  `ok` says that fused beats composed by more than the two spreads together.  The outputs of the two forms are
compared on the first set: their largest difference must stay within 2^-6 of the largest magnitude (bf16, five roundings against one).

    python tools/lora_bench.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _lora_native, synthetic  # noqa: E402
from tools.group_bench import SHAPES, capture, replay_us, summary  # noqa: E402


def run(name, ranks, args):
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
    x = synthetic.normal_device((1, K), dt, seed=6999, device=dev)
    lines = []
    for r in ranks:
        adapters = [[(synthetic.normal_device((r, K), dt, seed=9000 + 16 * s + g, device=dev),
                      synthetic.normal_device((N, r), dt, seed=9500 + 16 * s + g, device=dev), 2.0 / r) for g, N in enumerate(Ns)]
                    for s in range(args.sets)]

        def fused():
            for members, ads in zip(sets, adapters):
                bnb.matmul_4bit_lora_grouped(x, members, ads)

        def composed_one(members, ads):
            ys = bnb.matmul_4bit_grouped(x, members)
            return tuple(y + ((x @ a.t()) @ b.t()) * s for y, (a, b, s) in zip(ys, ads))

        def composed():
            for members, ads in zip(sets, adapters):
                composed_one(members, ads)

        def grouped():
            for members in sets:
                bnb.matmul_4bit_grouped(x, members)

        with torch.no_grad():
            _lora_native.reset_launch_log()
            got = bnb.matmul_4bit_lora_grouped(x, sets[0], adapters[0])
            assert _lora_native.launch_log == [(len(Ns), r * len(Ns), K, dt)], f"{name} r={r}: not one fused call: {_lora_native.launch_log}"
            form = _lora_native.last_launch()
            close = all(float((y.float() - c.float()).abs().max()) <= 2.0 ** -6 * float(c.float().abs().max())
                        for y, c in zip(got, composed_one(sets[0], adapters[0])))
            for _ in range(3):
                fused()
                composed()
                grouped()
            torch.cuda.synchronize()
            graphs = {"composed": capture(composed), "fused": capture(fused), "grouped": capture(grouped)}
            samples = {k: [] for k in graphs}
            for _ in range(args.reps):           # alternating: what else runs on the machine hits every form alike
                for k, graph in graphs.items():
                    samples[k].append(replay_us(graph, args.replays))
        dev_us = {k: summary(v, args.sets) for k, v in samples.items()}
        f, c, g = dev_us["fused"], dev_us["composed"], dev_us["grouped"]
        lines.append({"shape": name, "members": list(Ns), "K": K, "r": r, "dtype": "bf16", "quant_type": "nf4", "double_quant": nested,
                      "sets": args.sets, "form": form, "close": close,
                      "device": {"fused": f, "composed": c, "grouped_no_adapter": g, "ratio": round(f["median_us"] / c["median_us"], 4),
                                 "saved_us_per_group": round(c["median_us"] - f["median_us"], 3),
                                 "adapter_cost_us_per_group": round(f["median_us"] - g["median_us"], 3),
                                 "note": f"one graph of {args.sets} steps per form, median of {args.reps} x {args.replays} replays, alternating"},
                      "ok": bool(close and f["median_us"] + f["spread_us"] + c["spread_us"] < c["median_us"])})
        del adapters, graphs
        torch.cuda.empty_cache()
    del sets
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="qkv,gate_up,qkv_dq")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lora_bench.py needs a GPU"
    for name in args.shapes.split(","):
        for result in run(name, [int(r) for r in args.ranks.split(",")], args):
            line = json.dumps(result)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
