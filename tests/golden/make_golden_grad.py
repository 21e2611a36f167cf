#!/usr/bin/env python3
"""
Golden vectors for the input and bias gradients of the quantised linears -- matmul_4bit / Linear4bit, Linear8bit, LinearFP8 --
captured by RUNNING THE REFERENCE's Python CPU path, which is differentiable (every forward ends in F.linear on the dequantised
weight), in the build container (same rules as make_golden.py: data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad.py

For each case the weight, bias, input x and upstream gradient G (so dY is not all ones) are synthetic.normal draws from the
case's `seed` (seed, +1, +2, +3; regenerated bit for bit by the tests, so only the results ship) and the fixture holds what the
reference's autograd gives for loss = (y.float() * G).sum(): x.grad and bias.grad.  Writes g9_grad.npz (bit patterns) and
manifest_grad.json (case list) next to this file.
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
from mps_bitsandbytes.nn import Linear4bit, Linear8bit, LinearFP8  # noqa: E402
from mps_bitsandbytes_amd import synthetic  # noqa: E402
from make_golden import bits, DT  # noqa: E402

# matmul_4bit cases: (lead shape of x, N, K, quant_type, blocksize, compress_statistics, weight dtype, x dtype, compute dtype, bias dtype, via)
# via "fn": functional.matmul_4bit on quantize_4bit's output; "module": Linear4bit.from_linear
SPECS_4BIT = [
    ((1,), 64, 128, "nf4", 64, False, "f16", "f16", None, "f16", "fn"),
    ((7,), 64, 128, "fp4", 32, True, "bf16", "bf16", None, "bf16", "fn"),
    ((32,), 63, 127, "nf4", 128, False, "f32", "f32", None, "f32", "fn"),
    ((32,), 64, 65, "fp4", 64, True, "f16", "f16", None, None, "fn"),
    ((128,), 256, 512, "nf4", 32, True, "bf16", "bf16", None, "bf16", "fn"),
    ((128,), 256, 512, "fp4", 128, False, "f16", "f32", "f32", "f16", "fn"),       # compute_dtype != weight dtype
    ((7,), 64, 128, "nf4", 64, False, "bf16", "bf16", None, "f32", "fn"),          # an f32 bias on a bf16 weight
    ((2, 5), 64, 128, "nf4", 64, True, "bf16", "bf16", "bf16", "bf16", "module"),  # 3-D input through Linear4bit
    ((32,), 64, 128, "nf4", 32, True, "f32", "f32", None, None, "fn"),
]
# Linear8bit / LinearFP8 cases: (kind, lead shape of x, N, K, dtype, bias)
SPECS_8BIT = [("linear8bit", (16,), 96, 128, "f16", True), ("linear8bit", (3, 4), 40, 64, "bf16", False),
              ("linearfp8", (16,), 96, 128, "f16", True), ("linearfp8", (3, 4), 40, 64, "bf16", True)]


def _linear(N, K, dt, has_bias, seed):
    lin = torch.nn.Linear(K, N, bias=has_bias)
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=seed, std=0.05))
        if has_bias:
            lin.bias.copy_(synthetic.normal((N,), torch.float32, seed=seed + 1))
    return lin.to(DT[dt])


def main():
    arrays, cases = {}, []
    for ci, (lead, N, K, qt, bs, cs, wdt, xdt, cdt, bdt, via) in enumerate(SPECS_4BIT):
        seed = 900 + 10 * ci
        W = synthetic.normal((N, K), DT[wdt], seed=seed, std=0.05)
        bias = None if bdt is None else synthetic.normal((N,), DT[bdt], seed=seed + 1).requires_grad_(True)
        x = synthetic.normal(lead + (K,), DT[xdt], seed=seed + 2).requires_grad_(True)
        if via == "fn":
            packed, st = ref.functional.quantize_4bit(W, blocksize=bs, compress_statistics=cs, quant_type=qt)
            y = ref.functional.matmul_4bit(x, packed, st, bias, compute_dtype=None if cdt is None else DT[cdt])
        else:
            lin = torch.nn.Linear(K, N, bias=True).to(DT[wdt])
            with torch.no_grad():
                lin.weight.copy_(W)
                lin.bias.copy_(bias.detach().to(DT[wdt]))
            mod = Linear4bit.from_linear(lin, compute_dtype=DT[cdt], quant_type=qt, blocksize=bs, compress_statistics=cs)
            bias = mod.bias
            y = mod(x)
        G = synthetic.normal(tuple(y.shape), torch.float32, seed=seed + 3)
        (y.float() * G).sum().backward()
        arrays[f"m{ci}_xgrad"] = bits(x.grad)
        if bias is not None:
            arrays[f"m{ci}_bgrad"] = bits(bias.grad)
        cases.append(dict(kind="matmul_4bit", id=ci, seed=seed, lead=list(lead), N=N, K=K, quant_type=qt, blocksize=bs, compress_statistics=cs,
                          w_dtype=wdt, x_dtype=xdt, compute_dtype=cdt, bias_dtype=None if bias is None else {v: k for k, v in DT.items()}[bias.dtype],
                          via=via, y_dtype={v: k for k, v in DT.items()}[y.dtype]))
    for ci, (kind, lead, N, K, dt, has_bias) in enumerate(SPECS_8BIT):
        seed = 1000 + 10 * ci
        lin = _linear(N, K, dt, has_bias, seed)
        mod = (Linear8bit if kind == "linear8bit" else LinearFP8).from_linear(lin)
        x = synthetic.normal(lead + (K,), DT[dt], seed=seed + 2).requires_grad_(True)
        y = mod(x)
        G = synthetic.normal(tuple(y.shape), torch.float32, seed=seed + 3)
        (y.float() * G).sum().backward()
        arrays[f"q{ci}_xgrad"] = bits(x.grad)
        if has_bias:
            arrays[f"q{ci}_bgrad"] = bits(mod.bias.grad)
        cases.append(dict(kind=kind, id=ci, seed=seed, lead=list(lead), N=N, K=K, dtype=dt, bias=has_bias))
    np.savez_compressed(os.path.join(HERE, "g9_grad.npz"), **arrays)
    manifest = dict(provenance=dict(reference="mpsops/mps-bitsandbytes v%s (/root/reference, CPU path)" % ref.__version__,
                                    torch=torch.__version__, generated=time.strftime("%Y-%m-%d"),
                                    script="tests/golden/make_golden_grad.py"), g9=cases)
    with open(os.path.join(HERE, "manifest_grad.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote g9_grad.npz:", len(cases), "cases")


if __name__ == "__main__":
    main()
