#!/usr/bin/env python
"""
Measure the MXFP4 mixture-of-experts MLP (`moe_mlp_mxfp4`) against the route the library offered before it, in one
process: two `matmul_mxfp4_experts` calls (k_mx_experts on its ceil(N / 16) x E grid) with the gated activation
between them and the routed sum after them as torch ops.

The method is tools/bench_mx_experts.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5),
five repetitions, the median and the spread (max - min) / median.  The shapes are the MLP block of gpt-oss: bf16, H = I = 2880,
A = 4 slots per token, T = 1, 2, 4, 8, 16 tokens with seeded, uniformly drawn DISTINCT experts per token, at E = 32 and E = 128.
Codes and scale bytes are random bytes (scale bytes 118 .. 126, no NaN block): the time does not depend on the values.

Each (E, T) point is measured three ways:
  eager     whole Python calls of both routes, output and workspace allocations included;
  graph     the replay of one captured graph of each route;
  launches  the C calls alone on preallocated buffers, to isolate the grid: gate / up with the activation (ceil(2I / 16) x R
            workgroups) against the gate / up launch of k_mx_experts (x E), and the down projection with k_routed_sum against
            the down launch of k_mx_experts without any sum.

One JSON line per (E, T), printed and written to `--out` (default profiles/moe_mlp_bench.jsonl).

    python tools/bench_mx_moe_mlp.py [--steps 20] [--warmup 5] [--tokens 1,2,4,8,16] [--experts 32,128] [--out FILE]
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
from mps_bitsandbytes_amd import _moe_native, _moemlp_native, synthetic  # noqa: E402
from mps_bitsandbytes_amd._native import BF16, F32, ptr, stream_ptr  # noqa: E402

SLOTS, HIDDEN, INTER = 4, 2880, 2880
ALPHA, LIMIT = 1.702, 7.0


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


def parent_route(x, wgu, sgu, bgu, wd, sd, bd, ids, rw):
    """Two k_mx_experts launches, and the activation and the routed sum as the torch ops a caller writes"""
    pre = bnb.matmul_mxfp4_experts(x, wgu, sgu, ids, bgu)
    g, u = pre[..., 0::2].clamp(max=LIMIT), pre[..., 1::2].clamp(min=-LIMIT, max=LIMIT)
    h = (u + 1) * (g * torch.sigmoid(g * ALPHA))
    y = bnb.matmul_mxfp4_experts(h, wd, sd, ids, bd)
    return (y * rw.unsqueeze(-1).to(y.dtype)).sum(dim=1)


def graphed(fn):
    """`fn` captured once on a side stream -> (a replay callable, the captured output)"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = fn()
    return graph.replay, out


def pair(new, old):
    (n, ns), (o, os_) = new, old
    return {"new_us": round(n, 2), "parent_us": round(o, 2), "new_to_parent": round(n / o, 3), "spread": round(max(ns, os_), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="1,2,4,8,16", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_mlp_bench.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    moe, mlp = _moe_native.lib(), _moemlp_native.lib()
    H, I, A = HIDDEN, INTER, SLOTS
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
            distinct = int(torch.unique(ids).numel())
            new_fn = lambda: bnb.moe_mlp_mxfp4(x, wgu, sgu, bgu, wd, sd, bd, ids, rw)
            old_fn = lambda: parent_route(x, wgu, sgu, bgu, wd, sd, bd, ids, rw)
            with torch.no_grad():
                new, old = new_fn(), old_fn()
                # (the parent rounds pre, y and every torch op to bf16: the same block in another precision, so no bit check)
                assert float((new.float() - old.float()).abs().max()) <= 0.05 * float(old.float().abs().max()), "the two routes disagree"
                eager = pair(time_us(new_fn, args.steps, args.warmup), time_us(old_fn, args.steps, args.warmup))
                new_replay, _ = graphed(new_fn)
                old_replay, _ = graphed(old_fn)
                graph = pair(time_us(new_replay, args.steps, args.warmup), time_us(old_replay, args.steps, args.warmup))
                # the C calls alone, on preallocated buffers
                P = T * A
                h = torch.empty(T, A, I, dtype=torch.bfloat16, device=dev)
                pre = torch.empty(T, A, 2 * I, dtype=torch.bfloat16, device=dev)
                y = torch.empty(T, A, H, dtype=torch.bfloat16, device=dev)
                out = torch.empty(T, H, dtype=torch.bfloat16, device=dev)
                ws_bytes = _moemlp_native.workspace_bytes(T, A, H)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                s = stream_ptr(dev)
                c_glu = lambda: mlp.mbnb_moemlp_gate_up_glu(ptr(x), T, A, H, BF16, ptr(wgu), ptr(sgu), E, I, ptr(ids), ptr(bgu), BF16, ALPHA, LIMIT,
                                                            ptr(h), BF16, s)
                c_down = lambda: mlp.mbnb_moemlp_down_sum(ptr(h), T, A, I, BF16, ptr(wd), ptr(sd), E, H, ptr(ids), ptr(bd), BF16, ptr(rw), F32,
                                                          ptr(out), BF16, ptr(ws), ws_bytes, s)
                p_gu = lambda: moe.mbnb_moe_mxfp4_experts(ptr(x), T, A, 0, H, BF16, ptr(wgu), ptr(sgu), E, 2 * I, ptr(ids), ptr(bgu), BF16,
                                                          ptr(pre), BF16, s)
                p_down = lambda: moe.mbnb_moe_mxfp4_experts(ptr(h), T, A, 1, I, BF16, ptr(wd), ptr(sd), E, H, ptr(ids), ptr(bd), BF16, ptr(y),
                                                            BF16, s)
                assert c_glu() == 0 and c_down() == 0 and p_gu() == 0 and p_down() == 0
                gate_up = pair(time_us(c_glu, args.steps, args.warmup), time_us(p_gu, args.steps, args.warmup))
                down = pair(time_us(c_down, args.steps, args.warmup), time_us(p_down, args.steps, args.warmup))
            R = min(E, P)
            line = {"E": E, "shape": [T, A, H, I], "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "distinct_experts": distinct,
                    "workgroups": {"new": R * (2 * I // 16 + (H + 15) // 16), "parent": E * (2 * I // 16 + (H + 15) // 16)},
                    "eager": eager, "graph": graph, "launches": {"gate_up": gate_up, "down": down, "note": "new down includes k_routed_sum"}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del wgu, sgu, wd, sd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
