"""8-bit SGD with momentum (reference: mps_bitsandbytes/optim/sgd8bit.py): a signed 8-bit momentum buffer, one fused
HIP step.  Without momentum there is no state and the step is the reference's plain `p.add_(grad, alpha=-lr)`."""
from typing import Callable, Optional

import torch

from .. import _optim_native
from ._base import Optimizer8bit, check_hyper, f32, in_dtype, new_state


class SGD8bit(Optimizer8bit):
    """
    8-bit SGD optimizer with momentum.

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (required)
        momentum: Momentum factor (default: 0)
        dampening: Dampening for momentum (default: 0)
        weight_decay: Weight decay (L2 penalty) (default: 0)
        nesterov: Enables Nesterov momentum (default: False)
        block_size: Block size for quantization (default: 256)
    """
    _name = "SGD8bit"

    def __init__(self, params, lr: float, momentum: float = 0, dampening: float = 0, weight_decay: float = 0,
                 nesterov: bool = False, block_size: int = 256):
        check_hyper(lr=lr)
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum: {momentum}")
        check_hyper(weight_decay=weight_decay)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires momentum > 0 and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        block_size=block_size)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """Performs a single optimization step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, wd = group['lr'], group['weight_decay']
            momentum, dampening = group['momentum'], group['dampening']
            params = self._grads(group)
            if momentum == 0:
                for p in params:          # no state: the reference's two torch ops
                    grad = p.grad if wd == 0 else p.grad.add(p, alpha=wd)
                    p.add_(grad, alpha=-lr)
                continue
            block_size = self._block_size(group)
            items = []
            for p in params:
                state = self.state[p]
                if len(state) == 0:
                    state['momentum_int8'], state['momentum_absmax'] = new_state(p, block_size, signed=True)
                items.append((p, self._state_tensors(p, state, ('momentum_int8', 'momentum_absmax'), block_size), 0.0, 0.0))
            if not items:
                continue

            def scalars(pdt, gdt):
                return _optim_native.Scalars(f32(momentum), f32(1 - dampening), 0.0, 0.0, 0.0, in_dtype(wd, gdt), 0.0,
                                             in_dtype(-lr, pdt), _optim_native.WEIGHT_DECAY if wd != 0 else 0, 0)
            kind = _optim_native.SGD_NESTEROV if group['nesterov'] else _optim_native.SGD_MOMENTUM
            self._run(kind, block_size, items, scalars)
        return loss
