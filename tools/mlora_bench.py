#!/usr/bin/env python3
"""matmul_4bit_multilora_grouped on 2 to 16 rows (libmbnb_mlora.so: two launches per group, the rows' adapter slots read on the device)
against what a caller had before it.  The baselines are the earlier code and never run the new kernels:

  split    the batch split by adapter ON THE HOST (the ids known there): per distinct id one gather of its rows, one
           matmul_4bit_lora_grouped call with that slot's adapters, one scatter per member into the outputs;
  single   with ONE distinct adapter in the batch: the single-adapter fused call, matmul_4bit_lora_grouped on all rows.  Against it the
           new path is reported as an OVERHEAD (it stages B per row and reads the ids), not as a win.

Prints one JSON line per shape, rank, row count and number of distinct adapters in the batch (and appends it to --out).

Shapes (bf16 NF4):  qkv = 3 x [4096, 4096];  gate_up = 2 x [11008, 4096]; --ranks (16, 64), --rows (2, 8, 16), distinct adapters per batch
1, 2 and M (row m uses slot m mod distinct; banks of --slots (16) adapters, scaling 2 / r).  Each shape rotates over --sets (64) distinct
weight AND bank sets, so both come from HBM and not from the Infinity Cache (as tools/batch_bench.py does).

  device   one linear chain of the 64 steps captured into a HIP graph per form (one stream, no parallel branches); a sample is the
           mean of --replays (20) replays between two device events, and the forms are sampled ALTERNATELY, --reps (5) samples each.
           Reported per group (replay time / sets): the median, and the spread (max - min) of the samples.

`won` says that fused beats `split` by more than the two spreads together; `agree` that the outputs agree on the first set within
2^-6 of the largest magnitude (a group of one row runs the M = 1 launches, whose sums run in another order), `bit_equal` that they are
the same bits (expected wherever every split group has 2 rows or more).

    python tools/mlora_bench.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _mlora_native, synthetic  # noqa: E402
from tools.group_bench import SHAPES, capture, replay_us, summary  # noqa: E402


def run(name, rows, ranks, args):
    Ns, K, nested = SHAPES[name]
    dt, dev, S = torch.bfloat16, torch.device("cuda:0"), args.slots
    gen = torch.Generator(device=dev).manual_seed(9000)
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
        scale = [2.0 / r] * S
        scaling = torch.tensor(scale, dtype=torch.float32, device=dev)
        banks = [[(torch.randn(S, r, K, generator=gen, device=dev, dtype=dt), torch.randn(S, N, r, generator=gen, device=dev, dtype=dt), scaling)
                  for N in Ns] for _ in range(args.sets)]
        for M in rows:
            x = synthetic.normal_device((M, K), dt, seed=6999, device=dev)
            for distinct in sorted({1, 2, M}):
                host_ids = [m % distinct for m in range(M)]
                ids = torch.tensor(host_ids, dtype=torch.int32, device=dev)
                index = [torch.tensor([m for m in range(M) if host_ids[m] == d], device=dev) for d in range(distinct)]

                def single_adapters(s, d):
                    return [(a[d], b[d], scale[d]) for a, b, _ in banks[s]]

                def fused_one(s):
                    return bnb.matmul_4bit_multilora_grouped(x, sets[s], banks[s], ids)

                def split_one(s):      # the ids are known on the host: one call per distinct id, gathers and scatters included
                    outs = [torch.empty(M, N, dtype=dt, device=dev) for N in Ns]
                    for d in range(distinct):
                        ys = bnb.matmul_4bit_lora_grouped(x.index_select(0, index[d]), sets[s], single_adapters(s, d))
                        for out, y in zip(outs, ys):
                            out.index_copy_(0, index[d], y)
                    return tuple(outs)

                def single_one(s):
                    return bnb.matmul_4bit_lora_grouped(x, sets[s], single_adapters(s, 0))

                forms = {"split": split_one, "fused": fused_one}
                if distinct == 1:
                    forms["single"] = single_one

                def chain(one):
                    def fn():
                        for s in range(args.sets):
                            one(s)
                    return fn

                with torch.no_grad():
                    _mlora_native.reset_launch_log()
                    got = fused_one(0)
                    want = [(len(Ns), r * len(Ns), M, K, dt)]
                    assert _mlora_native.launch_log == want, f"{name} M={M} r={r}: not one fused call: {_mlora_native.launch_log}"
                    form = _mlora_native.last_launch()
                    ref = split_one(0)
                    if distinct == 1:
                        single_one(0)
                    assert _mlora_native.launch_log == want, "a baseline ran the new code"
                    agree = all(float((y.float() - c.float()).abs().max()) <= 2.0 ** -6 * float(c.float().abs().max()) for y, c in zip(got, ref))
                    bit_equal = all(torch.equal(y, c) for y, c in zip(got, ref))
                    for one in forms.values():
                        chain(one)()
                    torch.cuda.synchronize()
                    graphs = {k: capture(chain(one)) for k, one in forms.items()}
                    samples = {k: [] for k in graphs}
                    for _ in range(args.reps):           # alternating: what else runs on the machine hits every form alike
                        for k, graph in graphs.items():
                            samples[k].append(replay_us(graph, args.replays))
                dev_us = {k: summary(v, args.sets) for k, v in samples.items()}
                f, b = dev_us["fused"], dev_us["split"]
                line = {"shape": name, "members": list(Ns), "K": K, "M": M, "r": r, "distinct": distinct, "slots": S, "dtype": "bf16", "quant_type": "nf4",
                        "sets": args.sets, "form": form, "agree": agree, "bit_equal": bit_equal,
                        "device": dict(dev_us, ratio_to_split=round(f["median_us"] / b["median_us"], 4),
                                       saved_us_per_group=round(b["median_us"] - f["median_us"], 3),
                                       note=f"one graph of {args.sets} steps per form, median of {args.reps} x {args.replays} replays, alternating"),
                        "won": bool(agree and f["median_us"] + f["spread_us"] + b["spread_us"] < b["median_us"])}
                if distinct == 1:
                    line["device"]["overhead_us_over_single"] = round(f["median_us"] - dev_us["single"]["median_us"], 3)
                lines.append(line)
                print(json.dumps(line), flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps(line) + "\n")
                del graphs
                torch.cuda.empty_cache()
        del banks
    del sets
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="qkv,gate_up")
    ap.add_argument("--rows", default="2,8,16")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlora_bench.py needs a GPU"
    for name in args.shapes.split(","):
        run(name, [int(m) for m in args.rows.split(",")], [int(r) for r in args.ranks.split(",")], args)


if __name__ == "__main__":
    main()
