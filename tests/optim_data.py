"""
Seeded inputs for the 8-bit optimizer tests, shared by tests/golden/make_golden_optim_edges.py (which runs the reference on
them), tests/test_optim_emul_host.py and tests/test_gpu_optim_elementwise.py, so only results ship in the fixture.

Data kinds (the `data` key of a case in tests/optim_cases.py; `grange` = (lo, hi) binary exponents):
  normal    parameter and gradient ~N(0, 1)
  binades   gradient element i is N(0, 1) * 2^e_i with e_i uniform on lo..hi; block 1 of the tensor (when it has one) is all
            zeros and block 2 is the constant 2^lo (not with holes=False); the parameter is ~N(0, 1)
  top       f16 parameters near +-3e4, the top of the f16 range (run with lr = 1); gradient ~N(0, 1)
  ties_s    the first block's gradient is 254, -254, then +-(2k + 1): with a first moment of g / 2 (beta 0.5 from a zero state) or
            of g the requantisation argument (m / absmax) * 127 is k + 1/2 on the first step; the rest ~N(0, 1)
  ties_u    the first block's gradient is 510, then 2k + 1: with beta2 = 0.75 the second moment is g^2 / 4 and
            sqrt(v / max) * 255 is k + 1/2 on the first step; the rest ~N(0, 1)
A case with `pmin` keeps its parameters away from zero: +-(pmin + |N(0, 1)|).  The f32 Adam / AdamW cases that are compared with
the reference use pmin = 1.  Reason: torch's vectorised CPU sqrt is 1 ulp low on 0.7 % of inputs, which moves the
update u by a few ulp OF u; the gate on the parameter is 1 ulp OF p, and u stays below about 10 lr = 0.1, so with |p| >= 1 an ulp
of u is at most 1/8 ulp of p and the reference's own inconsistency cannot pass 1 ulp.  With p near zero, or cancelling against u,
it reaches tens of ulp of p (seen: 64) without any error in the rule.  The GPU tests, which compare with the emulation at zero
tolerance, keep parameters near zero in their other f32 cases.
Every value is finite.
"""
import numpy as np
import torch

from mps_bitsandbytes_amd import synthetic

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def numel_of(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def param(case: dict, j: int) -> torch.Tensor:
    """Parameter j of a case, on the CPU."""
    shape, dt = tuple(case["shapes"][j]), DT[case["pdt"]]
    seed = case["seed"] + 100 * j
    if case.get("data") == "top":
        v = synthetic.normal_f64(numel_of(shape), seed)
        return torch.from_numpy(np.where(v >= 0, 3.0e4, -3.0e4) + 1000.0 * v).to(dt).reshape(shape)
    if case.get("pmin"):
        v = synthetic.normal_f64(numel_of(shape), seed)
        return torch.from_numpy(np.where(v >= 0, 1.0, -1.0) * (case["pmin"] + np.abs(v))).to(dt).reshape(shape)
    return synthetic.normal(shape, dt, seed=seed)


def _tie_block(kind: str, n: int) -> np.ndarray:
    if kind == "ties_s":
        k = np.arange(n) // 2
        v = (2.0 * (k % 127) + 1.0) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        v[:2] = (254.0, -254.0)[:n]
    else:
        v = 2.0 * (np.arange(n) % 255) + 1.0
        v[0] = 510.0
    return v


def grad(case: dict, j: int, step: int, block_size: int = None) -> torch.Tensor:
    """The gradient of parameter j at step `step` (1-based), on the CPU.  `block_size`: the group's (for the block-wise kinds)."""
    shape, dt = tuple(case["shapes"][j]), DT[case["gdt"]]
    n = numel_of(shape)
    seed = case["seed"] + 100 * j + step
    kind = case.get("data", "normal")
    v = synthetic.normal_f64(n, seed)
    bs = int(block_size or case.get("block_size", 256))
    if kind == "binades":
        lo, hi = case["grange"]
        e = lo + (synthetic.uniform_u64(n, seed + 7) % np.uint64(hi - lo + 1)).astype(np.int64)
        v = v * np.exp2(e.astype(np.float64))
        if case.get("holes", True):
            v[bs:2 * bs] = 0.0
            v[2 * bs:3 * bs] = 2.0 ** lo
    elif kind in ("ties_s", "ties_u"):
        k = min(n, bs)
        v[:k] = _tie_block(kind, k)
    t = torch.from_numpy(v).to(dt).reshape(shape)
    assert bool(torch.isfinite(t).all()), (case, j, step)
    return t


def emulation(case: dict) -> list:
    """One EmuTensor per parameter of a case, with its group's hyperparameters and block size."""
    from tests import optim_cases, optim_emul
    out = []
    for j in range(len(case["shapes"])):
        gi = case["group_of"][j] if case.get("group_of") else 0
        out.append(optim_emul.EmuTensor(case["rule"], optim_cases.group_kwargs(case, gi), param(case, j), optim_cases.block_size_of(case, j)))
    return out


def step_grads(case: dict, step: int) -> list:
    """The gradients of one step (1-based), None where the case says so."""
    from tests import optim_cases
    none = case.get("none_steps") or [[] for _ in case["shapes"]]
    return [None if step in none[j] else grad(case, j, step, optim_cases.block_size_of(case, j)) for j in range(len(case["shapes"]))]
