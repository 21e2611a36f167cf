"""Machinery shared by the optimizers.  FusedOptimizer: what the 8-bit and the paged ones have in common (hyper-parameter and gradient
checks, staging of operands a kernel cannot take in place).  Optimizer8bit: state dtypes across load_state_dict, state checks, and one
fused HIP step per (parameter dtype, gradient dtype) pair of a group (libmbnb_optim.so; no CPU path)."""
import numbers
from collections import defaultdict
from typing import Dict, List, Tuple

import numpy as np
import torch
from torch.optim import Optimizer

from .. import _native, _optim_native
from ..functional import _check_device

# the reference's state layout (mps_bitsandbytes/optim/*.py); torch's load_state_dict casts all of these to the
# parameter dtype, the optimizers put them back
STATE_DTYPES = {"exp_avg_int8": torch.int8, "exp_avg_absmax": torch.float32, "exp_avg_sq_uint8": torch.uint8,
                "exp_avg_sq_max": torch.float32, "momentum_int8": torch.int8, "momentum_absmax": torch.float32}


def f32(x: float) -> float:
    """x rounded once (RNE) to f32: what torch does with a Python scalar in an f32 op."""
    return float(np.float32(x))


def in_dtype(x: float, dtype: torch.dtype) -> float:
    """x as torch rounds an `alpha` for a tensor of `dtype`: double -> f32 -> dtype."""
    return torch.tensor(x, dtype=torch.float32).to(dtype).float().item()


def _aligned(t: torch.Tensor) -> bool:
    return t.is_contiguous() and t.data_ptr() % 16 == 0


def check_hyper(lr=None, eps=None, betas=None, weight_decay=None) -> None:
    """The constructors' range checks, with the reference's texts; an optimizer passes the hyper-parameters it has."""
    if lr is not None and lr < 0.0:
        raise ValueError(f"Invalid learning rate: {lr}")
    if eps is not None and eps < 0.0:
        raise ValueError(f"Invalid epsilon: {eps}")
    if betas is not None:
        for i in (0, 1):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError(f"Invalid beta{i + 1}: {betas[i]}")
    if weight_decay is not None and weight_decay < 0.0:
        raise ValueError(f"Invalid weight_decay: {weight_decay}")


class FusedOptimizer(Optimizer):
    """Base of the 8-bit and the paged optimizers: a step hands raw pointers of parameters and gradients to one fused kernel."""

    _name = "FusedOptimizer"
    _f32_grads = True      # a gradient may be float32 beside a 16-bit parameter (the 8-bit kernels); False: the parameter's dtype alone

    def _grads(self, group) -> List[torch.nn.Parameter]:
        """The group's parameters that have a gradient, checked (sparse, device, dtypes)."""
        out = []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError(f"{self._name} does not support sparse gradients")
            _check_device(p, self._name)
            _check_device(p.grad, self._name)
            _native.dtype_code(p.dtype, self._name)
            if p.grad.dtype != p.dtype and not (self._f32_grads and p.grad.dtype == torch.float32):
                rule = "be the parameter's dtype or float32" if self._f32_grads else "have the parameter's dtype"
                raise TypeError(f"mps_bitsandbytes_amd {self._name}: gradient dtype {p.grad.dtype} does not go with parameter "
                                f"dtype {p.dtype} (the gradient must {rule})")
            if p.grad.device != p.device:
                raise ValueError(f"mps_bitsandbytes_amd {self._name}: gradient on {p.grad.device}, parameter on {p.device}")
            out.append(p)
        return out

    @staticmethod
    def _stage(params) -> Tuple[list, list]:
        """(parameter, gradient) as the kernel can address them, per parameter: itself where it is contiguous and 16-byte aligned, else a
        clone.  Also the (parameter, clone) pairs to copy back after the launch (_unstage); the caller keeps the first list until then."""
        staged, writeback = [], []
        for p in params:
            w, g = p, p.grad
            if not _aligned(w):
                w = p.detach().clone(memory_format=torch.contiguous_format)
                writeback.append((p, w))
            if not _aligned(g):
                g = g.clone(memory_format=torch.contiguous_format)
            staged.append((w, g))
        return staged, writeback

    @staticmethod
    def _unstage(writeback) -> None:
        for p, w in writeback:
            p.copy_(w)


class Optimizer8bit(FusedOptimizer):
    """Base of Adam8bit / AdamW8bit / Lion8bit / SGD8bit."""

    _name = "Optimizer8bit"
    _step_flags = 0        # mbnb_optim_step flags (tests set FORCE_GENERIC to compare the two kernel paths)

    def load_state_dict(self, state_dict) -> None:
        # torch.optim.Optimizer.load_state_dict casts every state tensor of a floating-point parameter to the parameter's
        # dtype (f16 would turn an absmax of 1e-8 into 0); take the saved tensors as they were, in the reference's dtypes
        saved = {pid: {k: v for k, v in st.items() if k in STATE_DTYPES and isinstance(v, torch.Tensor)}
                 for pid, st in state_dict["state"].items()}
        super().load_state_dict(state_dict)
        self.__dict__.pop("_checked_state", None)
        ids = [pid for g in state_dict["param_groups"] for pid in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for pid, p in zip(ids, params):
            if pid not in saved:
                continue
            st = self.state[p]
            for k, v in saved[pid].items():
                dt = STATE_DTYPES[k]
                if not dt.is_floating_point and v.is_floating_point():
                    v = v.round()             # codes that were cast to a float dtype (integers up to 255: exact)
                w = v.to(device=p.device, dtype=dt).contiguous()
                st[k] = w.clone() if w is v else w      # never share state tensors with the optimizer the dict came from
            if "step" in st and isinstance(st["step"], torch.Tensor):
                st["step"] = int(st["step"].item())

    def _block_size(self, group) -> int:
        block_size = group["block_size"]
        if not isinstance(block_size, numbers.Integral) or isinstance(block_size, bool) or block_size <= 0:
            raise ValueError(f"{self._name}: block_size must be a positive int, got {block_size!r}")
        return int(block_size)

    def _state_tensors(self, p, state, keys, block_size) -> tuple:
        """(codes1, max1, codes2, max2) of `p`, checked by check_state before they can reach a launch."""
        tensors = tuple(state.get(k) for k in keys) + (None,) * (4 - len(keys))
        # checked once per layout: again whenever the block size or any pointer (a new state tensor, a parameter moved or
        # replaced) changes
        try:
            key = (block_size, p.data_ptr(), p.numel()) + tuple(t.data_ptr() for t in tensors[:len(keys)])
        except AttributeError:          # a state entry that is missing or not a tensor
            key = None
        checked = self.__dict__.setdefault("_checked_state", {})
        if key is None or checked.get(p) != key:
            check_state(p, tensors, block_size, self._name, two_moments=len(keys) == 4)
            checked[p] = key
        return tensors

    def _run(self, kind: int, block_size: int, items: List[tuple], scalars_for) -> None:
        """items: (param, [state tensors: codes1, max1, codes2, max2 or None] from _state_tensors, bc2_sqrt, neg_step_size) per parameter.
        One fused launch per (param dtype, grad dtype) pair and device (chunked at the kernel-argument limit)."""
        buckets: Dict[tuple, list] = defaultdict(list)
        for it in items:
            p = it[0]
            buckets[(p.device, p.dtype, p.grad.dtype)].append(it)
        for (dev, pdt, gdt), its in buckets.items():
            staged, writeback = self._stage([it[0] for it in its])
            descs = [(w.data_ptr(), g.data_ptr(), c1.data_ptr(), m1.data_ptr(), 0 if c2 is None else c2.data_ptr(),
                      0 if m2 is None else m2.data_ptr(), w.numel(), bc2, nss)
                     for (w, g), (_, (c1, m1, c2, m2), bc2, nss) in zip(staged, its)]
            with _native.on_device(dev):
                _optim_native.step(kind, pdt, gdt, block_size, scalars_for(pdt, gdt), descs, _native.stream_ptr(dev),
                                   self._step_flags)
            self._unstage(writeback)


def check_state(p: torch.Tensor, tensors, block_size: int, name: str, two_moments: bool = False) -> None:
    """The state tensors of `p` as the kernel will address them: codes of p.numel() int8 / uint8 elements and
    ceil(numel / block_size) f32 maxima, contiguous, on p's device.  The kernel gets raw pointers and sizes from the
    parameter, so anything else -- a checkpoint of a model with other shapes, a changed block_size, a parameter moved
    to another device -- is refused here rather than read or written out of bounds."""
    c1, m1, c2, m2 = tensors
    nb = _optim_native.n_blocks(p.numel(), block_size)
    want = [(c1, "codes", torch.int8, p.numel()), (m1, "maxima", torch.float32, nb)]
    if two_moments:
        want += [(c2, "second-moment codes", torch.uint8, p.numel()), (m2, "second-moment maxima", torch.float32, nb)]
    for t, what, dt, n in want:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: optimizer state {what} missing for a parameter of shape {tuple(p.shape)}")
        if t.dtype != dt or t.device != p.device or not t.is_contiguous() or t.numel() != n:
            raise ValueError(
                f"{name}: optimizer state {what} do not fit the parameter: got {t.numel()} {t.dtype} elements on {t.device}"
                f"{'' if t.is_contiguous() else ' (non-contiguous)'}, need {n} contiguous {dt} on {p.device} for a parameter of "
                f"shape {tuple(p.shape)} with block_size {block_size} (state from another model, or block_size / device changed "
                f"after the state was created)")


def new_state(p: torch.Tensor, block_size: int, signed: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """The quantisation of zeros (adam8bit.py quantize_state / quantize_state_unsigned): codes 0 with the parameter's
    shape, per-block maxima 1e-8 (signed) or 1e-12 (unsigned) in f32."""
    if block_size <= 0:
        raise ValueError(f"block_size must be positive, got {block_size}")
    nb = _optim_native.n_blocks(p.numel(), block_size)
    codes = torch.zeros(p.shape, dtype=torch.int8 if signed else torch.uint8, device=p.device)
    mx = torch.full((nb,), 1e-8 if signed else 1e-12, dtype=torch.float32, device=p.device)
    return codes, mx
