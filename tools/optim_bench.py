#!/usr/bin/env python3
"""8-bit optimizer step timing (HIP events, median of --reps windows of --steps steps after --warmup); prints one JSON line.

(a) one 4096 x 11008 bf16 parameter under AdamW8bit: us per step, bytes per step from shapes (2 B param read + write,
    2 B grad, 1 + 1 B codes read + write, 16 B of maxima per 256-element block) over time, and a device-to-device copy
    of the same byte count timed in the same run.
(b) the LoRA set, 128 x (16 x 4096) + 128 x (4096 x 16) bf16: the fused multi-tensor step, a loop of one step per
    tensor, and torch.optim.AdamW (foreach; fused where this torch offers it) on the same tensors.
(c) optimizer state bytes per parameter against torch.optim.AdamW.

    python tools/optim_bench.py --steps 20 --warmup 5 --reps 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mps_bitsandbytes_amd import optim, synthetic  # noqa: E402


def timed(fn, steps, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return statistics.median(out)


def params(shapes, seed):
    ps = []
    for i, s in enumerate(shapes):
        p = torch.nn.Parameter(synthetic.normal_device(s, torch.bfloat16, seed=seed + i))
        p.grad = synthetic.normal_device(s, torch.bfloat16, seed=seed + 10000 + i)
        ps.append(p)
    return ps


def state_bytes(opt):
    return sum(v.numel() * v.element_size() for st in opt.state.values() for v in st.values() if isinstance(v, torch.Tensor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py needs a GPU")
    st, wu, reps = args.steps, args.warmup, args.reps

    # (a) one large parameter
    (big,) = params([(4096, 11008)], 1)
    n = big.numel()
    opt = optim.AdamW8bit([big], lr=1e-5)
    us = timed(opt.step, st, wu, reps)
    nbytes = n * 2 * 2 + n * 2 + n * 1 * 4 + (n // 256) * 16      # param r+w, grad, two codes r+w, 2 x (r+w) f32 maxima per block
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src), st, wu, reps)      # reads nbytes/2 and writes nbytes/2
    a = dict(numel=n, us_per_step=round(us, 2), bytes_per_step=nbytes, gbps=round(nbytes / us / 1e3, 1),
             copy_us=round(copy_us, 2), copy_gbps=round(nbytes / copy_us / 1e3, 1), fraction_of_copy=round(copy_us / us, 3))
    ab = state_bytes(opt) / n
    del opt, big, src, dst

    # (b) the LoRA set
    shapes = [(16, 4096)] * 128 + [(4096, 16)] * 128
    ps = params(shapes, 100)
    fused = optim.AdamW8bit(ps, lr=1e-5)
    b = dict(tensors=len(ps), fused_us=round(timed(fused.step, st, wu, reps), 2))
    singles = [optim.AdamW8bit([p], lr=1e-5) for p in ps]
    b["per_tensor_loop_us"] = round(timed(lambda: [o.step() for o in singles], st, wu, reps), 2)
    tf = torch.optim.AdamW(ps, lr=1e-5, foreach=True)
    b["torch_adamw_foreach_us"] = round(timed(tf.step, st, wu, reps), 2)
    tb = state_bytes(tf) / sum(p.numel() for p in ps)
    try:
        tfu = torch.optim.AdamW(ps, lr=1e-5, fused=True)
        b["torch_adamw_fused_us"] = round(timed(tfu.step, st, wu, reps), 2)
    except (RuntimeError, ValueError) as e:
        b["torch_adamw_fused_us"] = None
        b["torch_adamw_fused_error"] = str(e)[:120]
    c = dict(adamw8bit_bytes_per_param=round(ab, 4), torch_adamw_bytes_per_param=round(tb, 4))
    print(json.dumps(dict(tool="optim_bench", device=torch.cuda.get_device_name(0), steps=st, warmup=wu, reps=reps,
                          a_single_4096x11008_bf16=a, b_lora_set=b, c_state=c)))


if __name__ == "__main__":
    main()
