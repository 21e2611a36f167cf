#!/usr/bin/env python
"""
Measure the mixture-of-experts router (`moe_router_topk`) and the whole block (`MoEBlockMXFP4`) against the route a
caller had before them, in one process: the router as four torch ops,

    F.linear(x, W, b) -> torch.topk -> torch.softmax -> .to(int32)

alone, and feeding `MoEMLPMXFP4`.

The method is tools/bench_mx_moe_mlp.py's: HIP events around `--steps` calls (default 20) after `--warmup` untimed ones (default 5),
five repetitions with the two routes ALTERNATED (new, torch, new, torch, ...), the median of each and the spread (max - min) / median.
The shapes are gpt-oss's: bf16, H = I = 2880, A = 4, E = 32 and 128, T = 1 .. 256 tokens of seeded normal rows; the expert codes
and scale bytes are random bytes (scale bytes 118 .. 126): the time does not depend on the values.

Each (E, T) point is measured three ways:
  router eager   whole Python calls of both routers, output allocations included;
  router graph   the replay of one captured graph of each;
  block  eager   `MoEBlockMXFP4(x)` against the torch router feeding `MoEMLPMXFP4` (T up to 256: 1024 pairs, one call of the MLP).

The two routers are not the same function: torch rounds the logits to bf16 and leaves the order of ties open, so the ids are only
required to agree where the f32 logits are apart (reported as `ids_agree`, the share of tokens with the same set of experts).

One JSON line per (E, T), printed and written to `--out` (default profiles/router_bench.jsonl).

    python tools/bench_mx_router.py [--steps 20] [--warmup 5] [--tokens 1,2,4,8,16,64,256] [--experts 32,128] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mps_bitsandbytes_amd as bnb  # noqa: E402
from mps_bitsandbytes_amd import synthetic  # noqa: E402

SLOTS, HIDDEN, INTER = 4, 2880, 2880


def once_us(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def time_pair(new, old, steps, warmup, reps=5):
    """the two routes alternated, repetition by repetition -> {new_us, torch_us, new_to_torch, spread}: medians in microseconds per
    call, and the larger of the two spreads (max - min) / median"""
    for fn in (new, old):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    vals = ([], [])
    for _ in range(reps):
        for fn, v in zip((new, old), vals):
            v.append(once_us(fn, steps))
    n, o = statistics.median(vals[0]), statistics.median(vals[1])
    spread = max((max(v) - min(v)) / m for v, m in zip(vals, (n, o)))
    return {"new_us": round(n, 2), "torch_us": round(o, 2), "new_to_torch": round(n / o, 3), "spread": round(spread, 3)}


def torch_router(x, W, b, A):
    """the four eager kernels of a caller's router"""
    logits = torch.nn.functional.linear(x, W, b)
    v, i = torch.topk(logits, A, dim=-1)
    return i.to(torch.int32), torch.softmax(v, dim=-1, dtype=torch.float32)


def graphed(fn):
    """`fn` captured once on a side stream -> a replay callable"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        keep = fn()

    def replay():
        graph.replay()
    replay.keep = keep                                       # the captured outputs live as long as the replay does
    return replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="1,2,4,8,16,64,256", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "router_bench.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 1 and args.warmup >= 0
    dev = torch.device("cuda:0")
    H, I, A = HIDDEN, INTER, SLOTS
    lines = []
    for E in (int(v) for v in args.experts.split(",")):
        block = bnb.MoEBlockMXFP4(E, H, I, top_k=A, device=dev)
        g = torch.Generator(device=dev).manual_seed(41 * E)
        ex = block.experts
        ex.gate_up_proj_blocks.copy_(torch.randint(0, 256, tuple(ex.gate_up_proj_blocks.shape), dtype=torch.uint8, device=dev, generator=g))
        ex.gate_up_proj_scales.copy_(torch.randint(118, 127, tuple(ex.gate_up_proj_scales.shape), dtype=torch.uint8, device=dev, generator=g))
        ex.down_proj_blocks.copy_(torch.randint(0, 256, tuple(ex.down_proj_blocks.shape), dtype=torch.uint8, device=dev, generator=g))
        ex.down_proj_scales.copy_(torch.randint(118, 127, tuple(ex.down_proj_scales.shape), dtype=torch.uint8, device=dev, generator=g))
        ex.gate_up_proj_bias.copy_(synthetic.normal_device((E, 2 * I), torch.bfloat16, seed=9, device=dev))
        ex.down_proj_bias.copy_(synthetic.normal_device((E, H), torch.bfloat16, seed=10, device=dev))
        block.router.weight.copy_(synthetic.normal_device((E, H), torch.bfloat16, seed=12, device=dev) * 0.05)
        block.router.bias.copy_(synthetic.normal_device((E,), torch.bfloat16, seed=13, device=dev))
        W, b = block.router.weight, block.router.bias
        for T in (int(v) for v in args.tokens.split(",")):
            x = synthetic.normal_device((T, H), torch.bfloat16, seed=8, device=dev)
            new_router = lambda: bnb.moe_router_topk(x, W, b, A)
            old_router = lambda: torch_router(x, W, b, A)
            new_block = lambda: block(x)
            old_block = lambda: ex(x, *torch_router(x, W, b, A))
            with torch.no_grad():
                (ni, nw), (oi, ow) = new_router(), old_router()
                same = (torch.sort(ni, dim=1).values == torch.sort(oi, dim=1).values).all(dim=1)
                agree = float(same.float().mean())
                if bool(same.any()):
                    assert float((nw[same] - ow[same]).abs().max()) < 0.02, "the two routers disagree on the weights"
                eager = time_pair(new_router, old_router, args.steps, args.warmup)
                graph = time_pair(graphed(new_router), graphed(old_router), args.steps, args.warmup)
                whole = time_pair(new_block, old_block, args.steps, args.warmup)
            line = {"E": E, "shape": [T, A, H, I], "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "ids_agree": round(agree, 3),
                    "router_eager": eager, "router_graph": graph, "block_eager": whole}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del block, ex, W, b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
