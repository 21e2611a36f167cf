"""
The paged optimizers' step as executable numpy: DESIGN.md §14 and include/mbnb_paged.h restated per element.  Importable without a
GPU and without the reference.

Every tensor op of the reference's chain works on tensors of ONE dtype T (parameter, gradient and moments alike), so each op's f32
result is rounded to T: r(x).  A Python scalar meets a tensor either as a plain f32 operand, s32(x) = double -> f32, or as the
`alpha` of add / add_, which torch converts to the tensor's scalar type, sT(x) = double -> f32 -> T.

    Adam only, wd != 0:   g = r(fma(p, sT(wd), g))
    AdamW only, wd != 0:  p = r(p * s32(1 - lr*wd))
    m = r(m * s32(beta1));  m = r(fma(g, sT(1-beta1), m))
    v = r(v * s32(beta2));  v = r(fma(s32(1-beta2) * g, g, v))
    den = r(r(r(sqrt(v)) / s32((1-beta2**t)**0.5)) + s32(eps))
    p = r(p + (s32(-(lr/(1-beta1**t))) * m) / den)
    Lion, wd != 0:        p = r(p * s32(1 - lr*wd))
    u = r(fma(g, sT(1-beta1), r(m * s32(beta1))));  p = r(fma(sign(u), sT(-lr), p))
    m = r(fma(g, sT(1-beta2), r(m * s32(beta2))))

fma is exact (tests/optim_emul.py), division and sqrt are correctly rounded (numpy's f32 `/` and `np.sqrt`), plain products and sums
round once to f32.  The host scalars are computed here, in double; nothing is taken from mps_bitsandbytes_amd/optim/paged.py.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests.optim_emul import DT, F32, bits, fma, from_bits, rnd, scalar_in  # noqa: F401  (bits, from_bits: re-exported for the tests)

RULES = ("adam", "adamw", "lion")
TWO_MOMENTS = ("adam", "adamw")
NAME = {v: k for k, v in DT.items()}
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")


def host_scalars(rule: str, hp: dict, step: int, dt: str) -> SimpleNamespace:
    f = lambda x: F32(np.float64(x))
    lr, wd = float(hp["lr"]), float(hp.get("weight_decay", 0.0))
    b1, b2 = (float(b) for b in hp["betas"])
    s = SimpleNamespace(wd_on=wd != 0, b1=f(b1), b2=f(b2), omb1=scalar_in(1.0 - b1, dt), decay=f(1.0 - lr * wd))
    if rule in TWO_MOMENTS:
        s.omb2, s.eps, s.wd = f(1.0 - b2), f(hp["eps"]), scalar_in(wd, dt)
        s.bc2_sqrt = f(math.sqrt(1.0 - math.pow(b2, step)))
        s.neg_step_size = f(-(lr / (1.0 - math.pow(b1, step))))
    else:
        s.omb2, s.neg_lr = scalar_in(1.0 - b2, dt), scalar_in(-lr, dt)
    return s


def step_elems(rule: str, s: SimpleNamespace, dt: str, p, g, m, v=None):
    """One step of flat f32 arrays that hold values of `dt`.  Returns (p, m, v) after the step (v None for Lion)."""
    assert rule in RULES
    r = lambda x: rnd(np.asarray(x, dtype=F32), dt)
    p, g, m = (np.asarray(x, dtype=F32) for x in (p, g, m))
    with np.errstate(**_ERR):
        if rule == "lion":
            if s.wd_on:
                p = r(p * s.decay)
            u = r(fma(g, s.omb1, r(m * s.b1)))
            sg = (u > 0).astype(F32) - (u < 0).astype(F32)
            p = r(fma(sg, s.neg_lr, p))
            m = r(fma(g, s.omb2, r(m * s.b2)))
            return p, m, None
        v = np.asarray(v, dtype=F32)
        if rule == "adam" and s.wd_on:
            g = r(fma(p, s.wd, g))
        if rule == "adamw" and s.wd_on:
            p = r(p * s.decay)
        m = r(m * s.b1)
        m = r(fma(g, s.omb1, m))
        v = r(v * s.b2)
        v = r(fma(s.omb2 * g, g, v))
        den = r(r(r(np.sqrt(v)) / s.bc2_sqrt) + s.eps)
        p = r(p + (s.neg_step_size * m) / den)
    return p, m, v


def step_tensors(rule: str, hp: dict, step: int, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor = None):
    """One step of CPU torch tensors of one dtype; returns new (p, m, v) tensors of that dtype, flat."""
    dt = NAME[p.dtype]
    assert g.dtype == p.dtype and m.dtype == p.dtype
    f = lambda t: None if t is None else t.detach().cpu().reshape(-1).float().numpy()
    out = step_elems(rule, host_scalars(rule, hp, step, dt), dt, f(p), f(g), f(m), f(v))
    return tuple(None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(p.dtype) for x in out)


class EmuTensor:
    """One parameter and its moments on the host, stepped by the emulation with its own step count."""

    def __init__(self, rule: str, hp: dict, p: torch.Tensor):
        self.rule, self.hp = rule, dict(hp)
        self.p = p.detach().cpu().reshape(-1).clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p) if rule in TWO_MOMENTS else None
        self.step_count = 0

    def step(self, g: torch.Tensor):
        self.step_count += 1
        if self.p.numel():
            self.p, self.m, self.v = step_tensors(self.rule, self.hp, self.step_count, self.p, g.detach().cpu().reshape(-1), self.m, self.v)
