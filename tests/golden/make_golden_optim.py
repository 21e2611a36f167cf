#!/usr/bin/env python3
"""
Golden vectors for the 8-bit optimizers (Adam8bit, AdamW8bit, Lion8bit, SGD8bit), captured by RUNNING THE REFERENCE's
optimizers on CPU (its Python path) in the build container (same rules as make_golden.py: data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim.py

Each case is one parameter group.  Parameter j of a case starts as synthetic.normal(shape, param dtype, seed + 100 * j)
and its gradient at step s is synthetic.normal(shape, grad dtype, seed + 100 * j + s) -- regenerated bit for bit by the
tests, so only results ship -- except on the steps listed in `none_steps[j]`, where its .grad is None.  After every step
the fixture holds the parameter bits and the state (codes and per-block maxima) of every parameter that has state.
Writes g10_optim.npz and manifest_optim.json next to this file.
"""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

import mps_bitsandbytes as ref  # noqa: E402  (the reference, CPU path)
from mps_bitsandbytes.optim import Adam8bit, AdamW8bit, Lion8bit, SGD8bit  # noqa: E402
from mps_bitsandbytes_amd import synthetic  # noqa: E402
from make_golden import bits, DT  # noqa: E402

OPT = {"adam": Adam8bit, "adamw": AdamW8bit, "lion": Lion8bit, "sgd": SGD8bit}
STATE_KEYS = {"adam": ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"),
              "adamw": ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"),
              "lion": ("exp_avg_int8", "exp_avg_absmax"), "sgd": ("momentum_int8", "momentum_absmax")}

# (optimizer, kwargs, param dtype, grad dtype, shapes of the group's parameters, steps on which parameter j has no grad, steps)
SPECS = [
    ("adam", dict(lr=1e-2), "f16", "f16", [(1000,)], None, 4),
    ("adam", dict(lr=1e-2, weight_decay=0.01), "bf16", "bf16", [(1000,)], None, 4),
    ("adam", dict(lr=1e-2, weight_decay=0.01), "f32", "f32", [(1000,)], None, 4),
    ("adam", dict(lr=1e-2, block_size=64), "f16", "f16", [(1,), (255,)], None, 3),
    ("adamw", dict(lr=1e-2), "f16", "f16", [(1000,)], None, 4),
    ("adamw", dict(lr=1e-2, weight_decay=0), "bf16", "bf16", [(16, 64)], None, 3),
    ("adamw", dict(lr=1e-2, block_size=100), "f32", "f32", [(257,)], None, 4),
    ("adamw", dict(lr=1e-2, block_size=64), "f16", "f32", [(255,)], None, 4),
    ("adamw", dict(lr=1e-2, max_grad_norm=5.0), "bf16", "bf16", [(1000,)], None, 3),
    ("adamw", dict(lr=1e-2), "f16", "f16", [(300,), (700,), (257,)], [[], [2, 3], [1]], 4),
    ("lion", dict(lr=1e-2), "f16", "f16", [(1000,)], None, 4),
    ("lion", dict(lr=1e-2, weight_decay=0.1, block_size=64), "bf16", "bf16", [(257,)], None, 4),
    ("lion", dict(lr=1e-2, block_size=100), "f32", "f32", [(1000,)], None, 3),
    ("lion", dict(lr=1e-2), "f16", "f32", [(255,)], None, 3),
    ("sgd", dict(lr=1e-2, momentum=0.9), "f16", "f16", [(1000,)], None, 4),
    ("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.01, block_size=100), "bf16", "bf16", [(1000,)], None, 4),
    ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01, block_size=64), "f32", "f32", [(16, 64)], None, 4),
    ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01), "f16", "f32", [(257,)], None, 3),
    ("sgd", dict(lr=1e-2, momentum=0.8, weight_decay=0.01), "f16", "f16", [(255,)], None, 3),
]


def main():
    arrays, cases = {}, []
    for ci, (opt, kw, pdt, gdt, shapes, none_steps, steps) in enumerate(SPECS):
        seed = 2000 + 1000 * ci
        none_steps = none_steps or [[] for _ in shapes]
        params = []
        for j, shp in enumerate(shapes):
            p = torch.nn.Parameter(synthetic.normal(shp, DT[pdt], seed=seed + 100 * j))
            p.grad_dtype = None            # allow an f32 gradient on a 16-bit parameter
            params.append(p)
        o = OPT[opt](params, **kw)
        for s in range(1, steps + 1):
            for j, p in enumerate(params):
                p.grad = None if s in none_steps[j] else synthetic.normal(shapes[j], DT[gdt], seed=seed + 100 * j + s)
            o.step()
            for j, p in enumerate(params):
                arrays[f"c{ci}_p{j}_s{s}"] = bits(p.detach())
                st = o.state[p]
                for k in STATE_KEYS[opt] if st else ():
                    arrays[f"c{ci}_p{j}_s{s}_{k}"] = bits(st[k])
        cases.append(dict(id=ci, opt=opt, kwargs=kw, param_dtype=pdt, grad_dtype=gdt, shapes=[list(s) for s in shapes],
                          none_steps=none_steps, steps=steps, seed=seed))
    np.savez_compressed(os.path.join(HERE, "g10_optim.npz"), **arrays)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (/root/reference, CPU path)" % ref.__version__,
                                    torch=torch.__version__, generated=time.strftime("%Y-%m-%d"),
                                    script="tests/golden/make_golden_optim.py"),
                    state_keys=STATE_KEYS, g10=cases)
    with open(os.path.join(HERE, "manifest_optim.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g10_optim.npz:", len(cases), "cases")


if __name__ == "__main__":
    main()
