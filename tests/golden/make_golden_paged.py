#!/usr/bin/env python3
"""
Golden vectors for the paged optimizers (PagedAdam, PagedAdamW, PagedLion), captured by RUNNING THE REFERENCE's three classes on
CPU tensors in the build container (same rules as make_golden.py: data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paged.py

Each case is one parameter group of one dtype; its inputs are the recipes of tests/paged_cases.py, so only results ship: after
every step the bits of the parameter, exp_avg and exp_avg_sq of every parameter that has state (and the loaded moments of a case
that starts from a state).  Writes g14_paged.npz and manifest_paged.json next to this file.
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
sys.path.insert(0, os.path.dirname(HERE))      # tests/: paged_cases (the reference has a `tests` package of its own)
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

import mps_bitsandbytes as ref  # noqa: E402  (the reference, CPU path)
from mps_bitsandbytes.optim import PagedAdam, PagedAdamW, PagedLion  # noqa: E402
from make_golden import bits  # noqa: E402
import paged_cases  # noqa: E402

OPT = {"adam": PagedAdam, "adamw": PagedAdamW, "lion": PagedLion}
MOMENTS = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "lion": ("exp_avg",)}
WD = {"adam": 0.01, "adamw": 0.01, "lion": 0.1}
STEPS = 4


def specs():
    """Every rule x dtype once at 512 elements (no tail: exact everywhere) and once with a tail (257; 1000 for bf16 AdamW), one of
    the two with weight decay; tailed 16-bit cases and f32 Adam / AdamW cases keep |p| >= 1, and the tailed 16-bit cases' gradients
    take the parameter's sign (tests/paged_cases.py)."""
    out = []
    for opt in ("adam", "adamw", "lion"):
        for d, dt in enumerate(("f16", "bf16", "f32")):
            for tail in (False, True):
                n = 512 if not tail else (1000 if (opt, dt) == ("adamw", "bf16") else 257)
                wd = WD[opt] if (d % 2 == 0) != tail else 0
                away = (tail and dt != "f32") or (dt == "f32" and opt != "lion")
                out.append(dict(opt=opt, kwargs=dict(lr=1e-2, weight_decay=wd), dtype=dt, shapes=[[n]], away=away,
                                same_sign=tail and dt != "f32"))
    # one group of three tensors, gradients missing on some steps (each tensor keeps its own step count)
    out.append(dict(opt="adamw", kwargs=dict(lr=1e-2), dtype="bf16", shapes=[[40], [9, 8], [33]], away=True, same_sign=True,
                    none_steps=[[], [2, 3], [1]]))
    out.append(dict(opt="lion", kwargs=dict(lr=1e-2, weight_decay=0.1), dtype="f16", shapes=[[64], [40]], away=True, same_sign=True,
                    none_steps=[[2], []]))
    # Adam far into a run: a loaded state at step 1000
    out.append(dict(opt="adam", kwargs=dict(lr=1e-2, weight_decay=0.01), dtype="f32", shapes=[[257]], away=True, start_step=1000))
    return out


def main():
    arrays, cases = {}, []
    for ci, case in enumerate(specs()):
        case = dict(case, id=ci, seed=5000 + 1000 * ci, steps=STEPS)
        case.setdefault("none_steps", [[] for _ in case["shapes"]])
        case.setdefault("start_step", 0)
        opt, keys = case["opt"], MOMENTS[case["opt"]]
        params = [torch.nn.Parameter(paged_cases.initial_param(case, j)) for j in range(len(case["shapes"]))]
        o = OPT[opt](params, **case["kwargs"])
        if case["start_step"]:
            state = {}
            for j in range(len(params)):
                m, v = paged_cases.initial_moments(case, j)
                state[j] = dict(step=case["start_step"], exp_avg=m, exp_avg_sq=v)
                arrays[f"c{ci}_p{j}_s0_exp_avg"], arrays[f"c{ci}_p{j}_s0_exp_avg_sq"] = bits(m), bits(v)
            sd = o.state_dict()
            sd["state"] = state
            o.load_state_dict(sd)
        for s in range(1, STEPS + 1):
            for j, p in enumerate(params):
                p.grad = None if s in case["none_steps"][j] else paged_cases.gradient(case, j, s)
            o.step()
            for j, p in enumerate(params):
                arrays[f"c{ci}_p{j}_s{s}"] = bits(p.detach()).reshape(-1)
                assert not case["away"] or float(p.detach().abs().min()) >= 1.0, (ci, j, s)
                st = o.state[p]
                for k in keys if st else ():
                    assert st[k].dtype == p.dtype and st[k].shape == p.shape
                    arrays[f"c{ci}_p{j}_s{s}_{k}"] = bits(st[k]).reshape(-1)
        cases.append(case)
    np.savez_compressed(os.path.join(HERE, "g14_paged.npz"), **arrays)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (/root/reference, CPU path)" % ref.__version__,
                                    torch=torch.__version__, generated=time.strftime("%Y-%m-%d"),
                                    script="tests/golden/make_golden_paged.py"),
                    moments=MOMENTS, g14=cases)
    with open(os.path.join(HERE, "manifest_paged.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g14_paged.npz:", len(cases), "cases,", os.path.getsize(os.path.join(HERE, "g14_paged.npz")), "bytes")


if __name__ == "__main__":
    main()
