#!/usr/bin/env python3
"""Paged optimizer step timing; prints one JSON line per configuration (and appends it to --out when given).

Two configurations under PagedAdamW: (a) one 4096 x 11008 bf16 parameter, (b) --count (32) such f32 parameters.  For each, in the
same run, the median of --reps windows of --steps steps after --warmup (a host clock around work that ends in a device
synchronise: a paged step ends on the copy-out stream, which an event on the caller's stream would not see):

  resident      the step with the moments on the device (page_to_cpu=False): the fused kernel alone, one launch per 48 tensors
  device_copy   a device-to-device copy of the bytes the kernel moves (7 x numel x element size: p, g, m, v read; p, m, v written)
  page_in       the moments host -> device alone (pinned memory, one stream), page_out the same bytes device -> host alone,
  both          both directions at once on two streams: the floor of a paged step, which must move every moment both ways
  paged[n]      the paged step (page_to_cpu=True) at _page_elems = n, across --pages

    python tools/paged_bench.py --steps 5 --warmup 2 --reps 3
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mps_bitsandbytes_amd import optim  # noqa: E402
from mps_bitsandbytes_amd.optim import paged as paged_mod  # noqa: E402


def timed(fn, steps, warmup, reps, finish=lambda: None):
    """us per call of fn: the host clock over `steps` calls followed by finish() and a device synchronise."""
    for _ in range(warmup):
        fn()
    finish()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        finish()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / steps)
    return statistics.median(out), min(out), max(out)


def make_params(count, shape, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ps = []
    for _ in range(count):
        p = torch.nn.Parameter(torch.randn(shape, dtype=torch.float32, device="cuda", generator=gen).to(dtype))
        p.grad = torch.randn(shape, dtype=torch.float32, device="cuda", generator=gen).to(dtype)
        ps.append(p)
    return ps


def run(name, count, shape, dtype, pages, st, wu, reps):
    ps = make_params(count, shape, dtype, 1)
    numel = sum(p.numel() for p in ps)
    esize = ps[0].element_size()
    res = dict(config=name, tensors=count, numel=numel, dtype=str(dtype).replace("torch.", ""), moment_bytes=2 * numel * esize)

    # the kernel alone: moments resident
    opt = optim.PagedAdamW(ps, lr=1e-5, page_to_cpu=False)
    us = timed(opt.step, st, wu, reps)
    kbytes = 7 * numel * esize
    res["resident"] = dict(us=round(us[0], 1), min=round(us[1], 1), max=round(us[2], 1), bytes=kbytes, gbps=round(kbytes / us[0] / 1e3, 1))
    dev = [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]
    half = min(kbytes // 2, 1 << 32)
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cu = timed(lambda: dst.copy_(src), st, wu, reps)
    res["device_copy"] = dict(us=round(cu[0] * (kbytes / 2 / half), 1), gbps=round(2 * half / cu[0] / 1e3, 1),
                              resident_rate_over_copy_rate=round(cu[0] * (kbytes / 2 / half) / us[0], 3))
    del src, dst

    # the copies alone, the moments' bytes: host -> device, device -> host, both at once
    host = [tuple(torch.empty(m.shape, dtype=m.dtype, pin_memory=True).copy_(m) for m in pair) for pair in dev]
    s_in, s_out = paged_mod._copy_streams(ps[0].device)

    def page_in():
        with torch.cuda.stream(s_in):
            for hp, dp in zip(host, dev):
                for h, d in zip(hp, dp):
                    d.copy_(h, non_blocking=True)

    def page_out():
        with torch.cuda.stream(s_out):
            for hp, dp in zip(host, dev):
                for h, d in zip(hp, dp):
                    h.copy_(d, non_blocking=True)

    def both():          # the same buffers both ways at once: the contents race and are not used again, the bytes moved are the point
        page_in()
        page_out()

    mb = res["moment_bytes"]
    for key, fn in (("page_in", page_in), ("page_out", page_out)):
        t = timed(fn, st, wu, reps)
        res[key] = dict(us=round(t[0], 1), min=round(t[1], 1), max=round(t[2], 1), gbps=round(mb / t[0] / 1e3, 1))
    t = timed(both, st, wu, reps)
    res["both"] = dict(us=round(t[0], 1), min=round(t[1], 1), max=round(t[2], 1), gbps_each_way=round(mb / t[0] / 1e3, 1))
    del host, dev, opt
    torch.cuda.empty_cache()

    # the paged step across page sizes
    serial = res["page_in"]["us"] + res["resident"]["us"] + res["page_out"]["us"]
    res["serial_sum_us"] = round(serial, 1)
    res["paged"] = {}
    popt = optim.PagedAdamW(ps, lr=1e-5, page_to_cpu=True)
    for n in pages:
        popt._page_elems = n
        t = timed(popt.step, st, wu, reps, finish=popt.synchronize)
        res["paged"][str(n)] = dict(us=round(t[0], 1), min=round(t[1], 1), max=round(t[2], 1), pages=-(-numel // n),
                                    over_serial_sum=round(t[0] / serial, 3), over_both=round(t[0] / res["both"]["us"], 3),
                                    slot_mib=round(popt._slots * 2 * n * esize / 2 ** 20, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--count", type=int, default=32, help="f32 parameters of configuration (b)")
    ap.add_argument("--pages", type=int, nargs="+", default=[1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 26])
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--out", default=None, help="also append each JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("paged_bench.py needs a GPU")
    head = dict(tool="paged_bench", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, reps=args.reps)
    configs = [("a", "a_single_4096x11008_bf16", 1, torch.bfloat16), ("b", f"b_{args.count}x_4096x11008_f32", args.count, torch.float32)]
    for key, name, count, dtype in configs:
        if args.only and args.only != key:
            continue
        line = json.dumps(dict(head, **run(name, count, (4096, 11008), dtype, args.pages, args.steps, args.warmup, args.reps)))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
