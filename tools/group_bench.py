#!/usr/bin/env python3
"""matmul_4bit_grouped against the same members called one by one; prints one JSON line per shape (and appends it to --out).

Shapes (bf16 NF4, one activation row):  qkv = 3 x [4096, 4096];  gate_up = 2 x [11008, 4096];  qkv_dq = qkv with
double-quantised absmax.  Each shape rotates over --sets (64) distinct weight sets, so the weights come from HBM and not from the
Infinity Cache (as bench.py's `gemv` figure does).

  device   one linear chain of the 64 steps captured into a HIP graph per form (one stream, no parallel branches); a sample is the
           mean of --replays (20) replays between two device events, and the two forms are sampled ALTERNATELY, --reps (5) samples
           each.  Reported per group (replay time / sets): the median, and the spread (max - min) of the samples.
  host     the eager loop of the 64 steps by the host clock, ending in a device synchronise, per group (median of --reps).

`grouped` is one launch per group (the log of the binding is checked); `members` is the member-by-member form of the same
commit, which is matmul_4bit's unchanged code.  `ok` says that the grouped median is no slower than the members' median by more
than the spread of the members' own samples.  The outputs of the two forms are compared bit for bit on the first set.

    python tools/group_bench.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import _group_native, synthetic  # noqa: E402

SHAPES = {"qkv": ((4096, 4096, 4096), 4096, False), "gate_up": ((11008, 11008), 4096, False), "qkv_dq": ((4096, 4096, 4096), 4096, True)}


def replay_us(graph, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / replays * 1e3


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return graph


def host_us(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def summary(samples, sets):
    per = [s / sets for s in samples]
    return {"median_us": round(statistics.median(per), 3), "spread_us": round(max(per) - min(per), 3), "samples_us": [round(p, 3) for p in per]}


def run(name, args):
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

    def grouped():
        for members in sets:
            bnb.matmul_4bit_grouped(x, members)

    def by_member():
        for members in sets:
            for p, st in members:
                bnb.matmul_4bit(x, p, st)

    with torch.no_grad():
        _group_native.reset_launch_log()
        got = bnb.matmul_4bit_grouped(x, sets[0])
        assert _group_native.launch_log == [(len(Ns), K, dt)], f"{name}: not one fused launch: {_group_native.launch_log}"
        form = _group_native.last_launch()
        equal = all(torch.equal(y, bnb.matmul_4bit(x, p, st)) for y, (p, st) in zip(got, sets[0]))
        for _ in range(3):
            grouped()
            by_member()
        torch.cuda.synchronize()
        g_graph, m_graph = capture(grouped), capture(by_member)
        g_dev, m_dev = [], []
        for _ in range(args.reps):           # alternating: what else runs on the machine hits both forms alike
            m_dev.append(replay_us(m_graph, args.replays))
            g_dev.append(replay_us(g_graph, args.replays))
        g_host, m_host = [], []
        for _ in range(args.reps):
            m_host += host_us(by_member, 1)
            g_host += host_us(grouped, 1)
    dev_g, dev_m = summary(g_dev, args.sets), summary(m_dev, args.sets)
    host_g, host_m = summary(g_host, args.sets), summary(m_host, args.sets)
    packed_bytes = sum(N * K // 2 for N in Ns)
    line = {"shape": name, "members": list(Ns), "K": K, "dtype": "bf16", "quant_type": "nf4", "double_quant": nested, "sets": args.sets,
            "form": form, "bit_equal": equal,
            "device": {"grouped": dev_g, "members": dev_m, "ratio": round(dev_g["median_us"] / dev_m["median_us"], 4),
                       "saved_us_per_group": round(dev_m["median_us"] - dev_g["median_us"], 3),
                       "grouped_packed_GBps": round(packed_bytes / dev_g["median_us"] / 1e3, 1),
                       "note": f"one graph of {args.sets} steps per form, median of {args.reps} x {args.replays} replays, alternating"},
            "host": {"grouped": host_g, "members": host_m, "ratio": round(host_g["median_us"] / host_m["median_us"], 4),
                     "note": f"eager loop of {args.sets} steps ending in a synchronise, median of {args.reps}"},
            "ok": bool(equal and dev_g["median_us"] <= dev_m["median_us"] + dev_m["spread_us"])}
    del sets
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="qkv,gate_up,qkv_dq")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "group_bench.py needs a GPU"
    for name in args.shapes.split(","):
        line = json.dumps(run(name, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
