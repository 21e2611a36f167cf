"""
The inputs of the paged-optimizer fixture (tests/golden/g14_paged.npz), regenerated bit for bit from seeds so that only results ship.

Parameter j of a case starts as synthetic.normal(shape, dtype, seed + 100 * j); with `away` it is pushed away from zero,
sign(x) * (1.25 + |x|) computed in float64 and rounded once to the dtype, so |p| >= 1 through the case's steps.  Its gradient at step s
(1-based, counted from the case's first step) is synthetic.normal(shape, dtype, seed + 100 * j + s); with `same_sign` every gradient
element takes the sign of its parameter element, so that no sum of the moment chain cancels (torch's twice-rounded
16-bit tail is within 1 ulp of the once-rounded body only where the sum does not cancel).  A case with `start_step` begins from a loaded state: step
count `start_step`, exp_avg = normal(std 0.1, seed + 100 * j + 50), exp_avg_sq = the square (in float64, rounded once) of
normal(std 0.1, seed + 100 * j + 51).
"""
import torch

from mps_bitsandbytes_amd import synthetic

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def initial_param(case: dict, j: int) -> torch.Tensor:
    x = synthetic.normal(case["shapes"][j], DT[case["dtype"]], seed=case["seed"] + 100 * j)
    if case.get("away"):
        d = x.double()
        x = torch.where(d >= 0, 1.25 + d, d - 1.25).to(x.dtype)
    return x


def gradient(case: dict, j: int, s: int) -> torch.Tensor:
    g = synthetic.normal(case["shapes"][j], DT[case["dtype"]], seed=case["seed"] + 100 * j + s)
    if case.get("same_sign"):
        g = torch.where(initial_param(case, j) >= 0, g.abs(), -g.abs())
    return g


def initial_moments(case: dict, j: int):
    """(exp_avg, exp_avg_sq) of a case that starts from a loaded state."""
    dt, shape, seed = DT[case["dtype"]], case["shapes"][j], case["seed"] + 100 * j
    m = synthetic.normal(shape, dt, seed=seed + 50, std=0.1)
    v = (synthetic.normal(shape, torch.float64, seed=seed + 51, std=0.1) ** 2).to(dt)
    return m, v
