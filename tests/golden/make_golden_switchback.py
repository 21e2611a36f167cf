#!/usr/bin/env python3
"""
Golden vectors for SwitchBackLinear, captured by RUNNING THE REFERENCE's Python CPU path (nn/switchback.py), data only (same rules as
make_golden.py).  The reference checkout is the first argument:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_switchback.py /path/to/mps-bitsandbytes

Every input is a synthetic.normal draw from the case's seed (regenerated bit for bit by the tests, so only the results ship):
- "fl" cases: SwitchBackLinear.from_linear of an nn.Linear in f32 / f16 / bf16 -- the int8 codes and scales, and the forward's decoded
  weight Wd = weight_int8.to(T) * (weight_scales[:, None] / 127.0).to(T) for T in f16 / bf16 / f32;
- "fb" cases: forward output y, and for loss = (y.float() * G).sum() the gradients x.grad, weight_fp.grad and bias.grad; ragged M, N, K,
  with and without bias, f16 and bf16, 2-D and 3-D inputs.  The two "rows" cases are shaped for the dense routes (forward: M = 512,
  N = 3072; weight gradient: M = 64, N = 256, K = 6144) and keep a few rows of y / weight_fp.grad only;
- "loop": three SGD steps (lr 0.1 on weight_fp and bias) on ((y - target) ** 2).mean(), SwitchBackLinearCallback.sync() after each;
  the losses, weight_fp and the int8 codes / scales after every step.
Writes g11_switchback.npz (bit patterns) and manifest_switchback.json (case list) next to this file.
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
warnings.filterwarnings("ignore")

from mps_bitsandbytes_amd import synthetic  # noqa: E402

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
NAME = {v: k for k, v in DT.items()}

# from_linear: (N, K, linear dtype)
SPECS_FL = [(48, 100, "f32"), (64, 128, "f16"), (40, 72, "bf16")]
# forward + backward: (lead shape of x, N, K, dtype, bias, rows kept of y, rows kept of weight_fp.grad)  (None: all)
SPECS_FB = [
    ((7,), 40, 100, "f16", True, None, None),
    ((3, 5), 72, 136, "bf16", True, None, None),
    ((33,), 64, 128, "bf16", False, None, None),
    ((1,), 96, 64, "f16", True, None, None),
    ((100,), 24, 264, "f16", False, None, None),
    ((512,), 3072, 128, "bf16", True, [0, 1, 255, 256, 511], [0, 3071]),
    ((64,), 256, 6144, "f16", True, [0, 63], [0, 1, 128, 255]),
]


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.numpy().copy()


def linear(N, K, dt, has_bias, seed):
    lin = torch.nn.Linear(K, N, bias=has_bias)
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=seed, std=0.05))
        if has_bias:
            lin.bias.copy_(synthetic.normal((N,), torch.float32, seed=seed + 1))
    return lin.to(DT[dt])


def main(reference):
    sys.path.insert(0, reference)
    import mps_bitsandbytes as ref  # noqa: E402  (the reference, CPU path)
    from mps_bitsandbytes.nn import SwitchBackLinear, SwitchBackLinearCallback  # noqa: E402

    arrays, cases = {}, []
    for ci, (N, K, dt) in enumerate(SPECS_FL):
        seed = 1100 + 10 * ci
        mod = SwitchBackLinear.from_linear(linear(N, K, dt, True, seed))
        arrays[f"fl{ci}_q"] = bits(mod.weight_int8)
        arrays[f"fl{ci}_s"] = bits(mod.weight_scales)
        for t in ("f16", "bf16", "f32"):
            T = DT[t]
            arrays[f"fl{ci}_wd_{t}"] = bits(mod.weight_int8.to(T) * (mod.weight_scales.unsqueeze(1) / 127.0).to(T))
        cases.append(dict(kind="from_linear", id=ci, seed=seed, N=N, K=K, dtype=dt, compute_dtype=NAME[mod.compute_dtype]))
    for ci, (lead, N, K, dt, has_bias, yrows, wrows) in enumerate(SPECS_FB):
        seed = 1200 + 10 * ci
        mod = SwitchBackLinear.from_linear(linear(N, K, dt, has_bias, seed))
        x = synthetic.normal(lead + (K,), DT[dt], seed=seed + 2).requires_grad_(True)
        y = mod(x)
        G = synthetic.normal(tuple(y.shape), torch.float32, seed=seed + 3)
        (y.float() * G).sum().backward()
        y2, gw = y.detach().reshape(-1, N), mod.weight_fp.grad
        arrays[f"fb{ci}_y"] = bits(y2 if yrows is None else y2[yrows])
        arrays[f"fb{ci}_xgrad"] = bits(x.grad) if yrows is None else bits(x.grad.reshape(-1, K)[yrows])
        arrays[f"fb{ci}_wgrad"] = bits(gw if wrows is None else gw[wrows])
        if has_bias:
            arrays[f"fb{ci}_bgrad"] = bits(mod.bias.grad)
        cases.append(dict(kind="forward_backward", id=ci, seed=seed, lead=list(lead), N=N, K=K, dtype=dt, bias=has_bias,
                          y_rows=yrows, wgrad_rows=wrows))
    # training loop
    seed = 1300
    N, K, M = 32, 64, 8
    mod = SwitchBackLinear.from_linear(linear(N, K, "f16", True, seed))
    mod.train()
    cb = SwitchBackLinearCallback(mod)
    opt = torch.optim.SGD([mod.weight_fp, mod.bias], lr=0.1)
    x = synthetic.normal((M, K), torch.float16, seed=seed + 2)
    target = synthetic.normal((M, N), torch.float16, seed=seed + 3)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = ((mod(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        cb.sync()
        losses.append(loss.detach())
        arrays[f"loop{step}_wfp"] = bits(mod.weight_fp)
        arrays[f"loop{step}_q"] = bits(mod.weight_int8)
        arrays[f"loop{step}_s"] = bits(mod.weight_scales)
    arrays["loop_loss"] = bits(torch.stack(losses))
    cases.append(dict(kind="loop", seed=seed, N=N, K=K, M=M, dtype="f16", lr=0.1, steps=3))
    np.savez_compressed(os.path.join(HERE, "g11_switchback.npz"), **arrays)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (CPU path)" % ref.__version__, torch=torch.__version__,
                                    generated=time.strftime("%Y-%m-%d"), script="tests/golden/make_golden_switchback.py"), g11=cases)
    with open(os.path.join(HERE, "manifest_switchback.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g11_switchback.npz:", len(cases), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
