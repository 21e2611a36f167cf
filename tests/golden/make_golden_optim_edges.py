#!/usr/bin/env python3
"""
Golden vectors for the 8-bit optimizers at the edges (tests/optim_cases.py EDGES), captured by RUNNING THE REFERENCE's
optimizers on CPU (its Python path) in the build container (same rules as make_golden_optim.py: data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim_edges.py

The inputs come from tests/optim_data.py (seeded, regenerated bit for bit by the tests), so only results ship: after every
step, the parameter bits and the state (codes and per-block maxima) of every parameter that has state.  All inputs are
finite (asserted here); bit parity with the reference is a claim about finite inputs.
Writes g13_optim_edges.npz and manifest_optim_edges.json next to this file.
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
sys.path.insert(0, os.path.dirname(HERE))     # tests/: optim_cases and optim_data (the reference has a `tests` package too)
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

import mps_bitsandbytes as ref  # noqa: E402  (the reference, CPU path)
from mps_bitsandbytes.optim import Adam8bit, AdamW8bit, Lion8bit, SGD8bit  # noqa: E402
from make_golden import bits  # noqa: E402
import optim_cases  # noqa: E402
import optim_data  # noqa: E402

OPT = {"adam": Adam8bit, "adamw": AdamW8bit, "lion": Lion8bit, "sgd": SGD8bit, "sgd_nesterov": SGD8bit}
ADAM_KEYS = ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max")
STATE_KEYS = {"adam": ADAM_KEYS, "adamw": ADAM_KEYS, "lion": ("exp_avg_int8", "exp_avg_absmax"),
              "sgd": ("momentum_int8", "momentum_absmax"), "sgd_nesterov": ("momentum_int8", "momentum_absmax")}
LIMIT = 1 << 20


def main():
    arrays, cases = {}, []
    for c in optim_cases.EDGES:
        ci, n = c["edge"], len(c["shapes"])
        params = []
        for j in range(n):
            p = torch.nn.Parameter(optim_data.param(c, j))
            assert bool(torch.isfinite(p).all())
            p.grad_dtype = None            # allow an f32 gradient on a 16-bit parameter
            params.append(p)
        group_of = c.get("group_of") or [0] * n
        groups = [dict(params=[p for p, g in zip(params, group_of) if g == gi], **optim_cases.group_kwargs(c, gi))
                  for gi in range(max(group_of) + 1)]
        o = OPT[c["rule"]](groups, **c["kwargs"])
        none_steps = c.get("none_steps") or [[] for _ in range(n)]
        for s in range(1, c["steps"] + 1):
            if s in c.get("set_step", {}):
                for p in params:
                    o.state[p]["step"] = c["set_step"][s]
            for j, p in enumerate(params):
                if s in none_steps[j]:
                    p.grad = None
                else:
                    p.grad = optim_data.grad(c, j, s, optim_cases.block_size_of(c, j))
                    assert bool(torch.isfinite(p.grad).all())
            o.step()
            for j, p in enumerate(params):
                arrays[f"e{ci}_p{j}_s{s}"] = bits(p.detach())
                st = o.state[p]
                for k in STATE_KEYS[c["rule"]] if st else ():
                    arrays[f"e{ci}_p{j}_s{s}_{k}"] = bits(st[k])
        cases.append(dict(edge=ci, id=optim_cases.case_id(c), rule=c["rule"], param_dtype=c["pdt"], grad_dtype=c["gdt"],
                          shapes=[list(s) for s in c["shapes"]], steps=c["steps"], seed=c["seed"]))
    path = os.path.join(HERE, "g13_optim_edges.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (/root/reference, CPU path)" % ref.__version__,
                                    torch=torch.__version__, generated=time.strftime("%Y-%m-%d"),
                                    script="tests/golden/make_golden_optim_edges.py", cases="tests/optim_cases.py EDGES",
                                    inputs="tests/optim_data.py"),
                    state_keys=STATE_KEYS, g13=cases)
    with open(os.path.join(HERE, "manifest_optim_edges.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g13_optim_edges.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
