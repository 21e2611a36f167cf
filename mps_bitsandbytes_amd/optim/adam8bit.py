"""
8-bit Adam and AdamW (reference: mps_bitsandbytes/optim/adam8bit.py).

The moments live blockwise in 8 bits: exp_avg as signed absmax/127 codes, exp_avg_sq as sqrt-compressed unsigned /255
codes, one f32 maximum per `block_size` elements.  Each step is one fused HIP launch per 48 tensors of a (parameter
dtype, gradient dtype) pair of a parameter group (csrc/optim_kernels.hip): dequantise, update in f32, requantise, bit for bit the reference's
Python path.
"""
from typing import Callable, Optional, Tuple

import torch

from .. import _optim_native
from ._base import Optimizer8bit, check_hyper, f32, new_state


# ---------------------------------------------------------------- state codes (torch ops: utilities, not the step)
def _blocks(x: torch.Tensor, block_size: int) -> torch.Tensor:
    flat = x.flatten().float()
    pad = -flat.numel() % block_size
    if pad:
        flat = torch.nn.functional.pad(flat, (0, pad))
    return flat.view(-1, block_size)


def quantize_state(state: torch.Tensor, block_size: int = 256) -> Tuple[torch.Tensor, torch.Tensor]:
    """Signed blockwise int8 codes of `state` and the per-block absmax (clamped below at 1e-8)."""
    b = _blocks(state, block_size)
    absmax = b.abs().max(dim=1).values.clamp(min=1e-8)
    q = ((b / absmax.unsqueeze(1)) * 127).round().clamp(-127, 127).to(torch.int8)
    return q.flatten()[:state.numel()].view(state.shape), absmax


def dequantize_state(state_int8: torch.Tensor, absmax: torch.Tensor, block_size: int = 256,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Inverse of quantize_state: (q / 127) * absmax."""
    b = _blocks(state_int8, block_size)
    return ((b / 127.0) * absmax.unsqueeze(1)).flatten()[:state_int8.numel()].view(state_int8.shape).to(dtype)


def quantize_state_unsigned(state: torch.Tensor, block_size: int = 256,
                            warn_on_negative: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Unsigned sqrt-compressed uint8 codes of a non-negative `state` and the per-block max (clamped below at 1e-12).
    Negative values are clamped to 0 (with a warning when `warn_on_negative`)."""
    if warn_on_negative:
        neg = int((state < 0).sum().item())
        if neg:
            import warnings
            warnings.warn(f"quantize_state_unsigned: {neg} negative values clamped to 0. "
                          f"This may indicate an issue with the optimizer state.", UserWarning, stacklevel=2)
    b = _blocks(state, block_size).clamp(min=0)
    mx = b.max(dim=1).values.clamp(min=1e-12)
    q = ((b / mx.unsqueeze(1)).sqrt() * 255).round().clamp(0, 255).to(torch.uint8)
    return q.flatten()[:state.numel()].view(state.shape), mx


def dequantize_state_unsigned(state_uint8: torch.Tensor, block_max: torch.Tensor, block_size: int = 256,
                              dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Inverse of quantize_state_unsigned: (q / 255)^2 * max."""
    s = _blocks(state_uint8, block_size) / 255.0
    return ((s * s) * block_max.unsqueeze(1)).flatten()[:state_uint8.numel()].view(state_uint8.shape).to(dtype)


_KEYS = ('exp_avg_int8', 'exp_avg_absmax', 'exp_avg_sq_uint8', 'exp_avg_sq_max')


class _Adam8bitBase(Optimizer8bit):
    _kind = _optim_native.ADAM

    def __init__(self, params, lr, betas, eps, weight_decay, block_size, max_grad_norm):
        check_hyper(lr=lr, eps=eps, betas=betas, weight_decay=weight_decay)
        if max_grad_norm is not None and max_grad_norm <= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        block_size=block_size, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """Performs a single optimization step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            lr, wd, block_size = group['lr'], group['weight_decay'], self._block_size(group)
            max_grad_norm = group.get('max_grad_norm')
            if max_grad_norm is not None:
                with_grad = [p for p in group['params'] if p.grad is not None]
                if with_grad:
                    torch.nn.utils.clip_grad_norm_(with_grad, max_grad_norm)
            items = []
            for p in self._grads(group):
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg_int8'], state['exp_avg_absmax'] = new_state(p, block_size, signed=True)
                    state['exp_avg_sq_uint8'], state['exp_avg_sq_max'] = new_state(p, block_size, signed=False)
                tensors = self._state_tensors(p, state, _KEYS, block_size)
                state['step'] += 1
                step = state['step']
                # the reference's host scalars, in double, each rounded once to f32 where the f32 tensor op meets it
                bias_correction1 = 1 - beta1 ** step
                bias_correction2 = 1 - beta2 ** step
                step_size = lr / bias_correction1
                items.append((p, tensors, f32(bias_correction2 ** 0.5), f32(-step_size)))
            if not items:
                continue
            s = _optim_native.Scalars(f32(beta1), f32(1 - beta1), f32(beta2), f32(1 - beta2), f32(group['eps']),
                                      f32(wd), f32(1 - lr * wd), 0.0, _optim_native.WEIGHT_DECAY if wd != 0 else 0, 0)
            self._run(self._kind, block_size, items, lambda pdt, gdt: s)
        return loss


class Adam8bit(_Adam8bitBase):
    """
    8-bit Adam optimizer with blockwise quantization (L2 weight decay folded into the gradient).

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (default: 1e-3)
        betas: Coefficients for computing running averages (default: (0.9, 0.999))
        eps: Term added to denominator for numerical stability (default: 1e-8)
        weight_decay: Weight decay (L2 penalty) (default: 0)
        block_size: Block size for quantization (default: 256)
        max_grad_norm: clip the group's gradients to this total norm first (default: None)
    """
    _name = "Adam8bit"
    _kind = _optim_native.ADAM

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, block_size: int = 256, max_grad_norm: Optional[float] = None):
        super().__init__(params, lr, betas, eps, weight_decay, block_size, max_grad_norm)


class AdamW8bit(_Adam8bitBase):
    """
    8-bit AdamW optimizer with decoupled weight decay.

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (default: 1e-3)
        betas: Coefficients for computing running averages (default: (0.9, 0.999))
        eps: Term added to denominator for numerical stability (default: 1e-8)
        weight_decay: Weight decay coefficient (default: 1e-2)
        block_size: Block size for quantization (default: 256)
        max_grad_norm: clip the group's gradients to this total norm first (default: None)
    """
    _name = "AdamW8bit"
    _kind = _optim_native.ADAMW

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, block_size: int = 256, max_grad_norm: Optional[float] = None):
        super().__init__(params, lr, betas, eps, weight_decay, block_size, max_grad_norm)
