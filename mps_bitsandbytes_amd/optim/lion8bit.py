"""8-bit Lion (reference: mps_bitsandbytes/optim/lion8bit.py): one signed 8-bit momentum, one fused HIP step."""
from typing import Callable, Optional, Tuple

import torch

from .. import _optim_native
from ._base import Optimizer8bit, check_hyper, f32, in_dtype, new_state


class Lion8bit(Optimizer8bit):
    """
    8-bit Lion optimizer with blockwise quantization.

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (default: 1e-4)
        betas: Coefficients for computing running averages (default: (0.9, 0.99))
        weight_decay: Weight decay coefficient (default: 0)
        block_size: Block size for quantization (default: 256)
    """
    _name = "Lion8bit"

    def __init__(self, params, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.99), weight_decay: float = 0,
                 block_size: int = 256):
        check_hyper(lr=lr, betas=betas, weight_decay=weight_decay)
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay, block_size=block_size)
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
            items = []
            for p in self._grads(group):
                state = self.state[p]
                if len(state) == 0:
                    state['exp_avg_int8'], state['exp_avg_absmax'] = new_state(p, block_size, signed=True)
                items.append((p, self._state_tensors(p, state, ('exp_avg_int8', 'exp_avg_absmax'), block_size), 0.0, 0.0))
            if not items:
                continue

            def scalars(pdt, gdt):
                return _optim_native.Scalars(f32(beta1), f32(1 - beta1), f32(beta2), f32(1 - beta2), 0.0, 0.0,
                                             f32(1 - lr * wd), in_dtype(-lr, pdt), _optim_native.WEIGHT_DECAY if wd != 0 else 0, 0)
            self._run(_optim_native.LION, block_size, items, scalars)
        return loss
