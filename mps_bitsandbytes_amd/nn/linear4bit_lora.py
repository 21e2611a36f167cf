"""
Linear4bitLoRA / Linear4bitLoRAGroup — Linear4bit layers with un-merged LoRA adapters, alone or sharing their input.

No counterpart in the reference.  A LoRA trained over a 4-bit base cannot be merged into it without re-quantising, so the layer
that was trained is the layer that decodes: ``base(x) + scaling * (x @ lora_A^T) @ lora_B^T``.  The base stays an ordinary
Linear4bit submodule (its state-dict keys are its own under ``base.``); the forward is `functional.matmul_4bit_lora_grouped`: two
kernel launches for 1 to 16 rows of input under `no_grad` / `inference_mode` (the adapters are parameters), and the composed form --
`matmul_4bit` plus the adapter in torch ops, differentiable in the adapters and the input -- for everything else.
"""
import math
from typing import Sequence, Tuple

import torch
from torch import nn, Tensor

from .. import functional as F
from ._base import fold_leading
from .linear4bit import Linear4bit


def _forward(layers: Sequence['Linear4bitLoRA'], x: Tensor, in_features: int) -> Tuple[Tensor, ...]:
    for layer in layers:
        if layer.base.weight_quant_state is None:
            raise RuntimeError("Weight not quantized. Call from_linear() or load weights first.")
    compute_dtype = layers[0].base.compute_dtype
    rows, lead = fold_leading(x, in_features)
    if any(layer.base.compute_dtype != compute_dtype for layer in layers):
        ys = tuple(F.matmul_4bit_lora_grouped(rows, [(layer.base.weight, layer.base.weight_quant_state)], [layer.adapter()],
                                              [layer.base.bias], compute_dtype=layer.base.compute_dtype)[0] for layer in layers)
    else:
        ys = F.matmul_4bit_lora_grouped(rows, [(layer.base.weight, layer.base.weight_quant_state) for layer in layers],
                                        [layer.adapter() for layer in layers], [layer.base.bias for layer in layers],
                                        compute_dtype=compute_dtype)
    if x.dim() <= 2:
        return ys
    return tuple(y.reshape(*lead, layer.out_features) for y, layer in zip(ys, layers))


class Linear4bitLoRA(nn.Module):
    """`base`: the frozen Linear4bit; `lora_A` [r, in_features] (PEFT's Kaiming-uniform init) and `lora_B` [out_features, r] (zeros):
    parameters in the base's weight dtype; ``scaling = lora_alpha / r``."""

    def __init__(self, base: Linear4bit, r: int, lora_alpha: float = 1.0):
        super().__init__()
        if not isinstance(base, Linear4bit):
            raise TypeError(f"Linear4bitLoRA: base is a {type(base).__name__}, not a Linear4bit")
        if not isinstance(r, int) or r < 1:
            raise ValueError(f"Linear4bitLoRA: r must be a positive integer, got {r!r}")
        self.base = base
        self.in_features, self.out_features = base.in_features, base.out_features
        self.r, self.lora_alpha, self.scaling = r, lora_alpha, lora_alpha / r
        state = base.weight_quant_state
        dtype = base.compute_dtype if state is None else state.dtype
        a = torch.empty(r, self.in_features, dtype=torch.float32)
        nn.init.kaiming_uniform_(a, a=math.sqrt(5))       # PEFT's LoRA init: A Kaiming-uniform, B zeros, so the adapter starts at 0
        self.lora_A = nn.Parameter(a.to(device=base.weight.device, dtype=dtype))
        self.lora_B = nn.Parameter(torch.zeros(self.out_features, r, dtype=dtype, device=base.weight.device))

    def adapter(self) -> Tuple[Tensor, Tensor, float]:
        return self.lora_A, self.lora_B, self.scaling

    def forward(self, x: Tensor) -> Tensor:
        return _forward([self], x, self.in_features)[0]

    def extra_repr(self) -> str:
        return f'r={self.r}, lora_alpha={self.lora_alpha}'


class Linear4bitLoRAGroup(nn.Module):
    """`layers`: an nn.ModuleList of Linear4bitLoRA with equal `in_features` (state-dict keys under ``layers.<i>.``).
    ``forward(x)`` returns one output per member, each within the bounds of `functional.matmul_4bit_lora_grouped` around what
    ``member(x)`` defines."""

    def __init__(self, layers: Sequence[Linear4bitLoRA]):
        super().__init__()
        layers = list(layers)
        if not layers:
            raise ValueError("Linear4bitLoRAGroup needs at least one layer")
        for i, layer in enumerate(layers):
            if not isinstance(layer, Linear4bitLoRA):
                raise TypeError(f"Linear4bitLoRAGroup: layer {i} is a {type(layer).__name__}, not a Linear4bitLoRA")
            if layer.in_features != layers[0].in_features:
                raise ValueError(f"Linear4bitLoRAGroup: layer {i} has in_features={layer.in_features}, layer 0 has "
                                 f"in_features={layers[0].in_features}; the members share one input")
        self.in_features = layers[0].in_features
        self.layers = nn.ModuleList(layers)

    def forward(self, x: Tensor) -> Tuple[Tensor, ...]:
        return _forward(list(self.layers), x, self.in_features)

    def extra_repr(self) -> str:
        return f'in_features={self.in_features}, out_features={tuple(layer.out_features for layer in self.layers)}'
