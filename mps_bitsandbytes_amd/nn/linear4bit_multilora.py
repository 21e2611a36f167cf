"""
Linear4bitMultiLoRA / Linear4bitMultiLoRAGroup — Linear4bit layers with a BANK of un-merged LoRA adapters, one chosen per row.

No counterpart in the reference.  Continuous batching over one frozen 4-bit base serves requests that carry different adapters:
``base(x)[m] + scaling[s] * (x[m] @ lora_A[s]^T) @ lora_B[s]^T`` with ``s = adapter_ids[m]``; a row whose id is outside ``[0, S)``
(-1, say) gets ``base(x)[m]`` alone.  The base stays an ordinary Linear4bit submodule (its state-dict keys are its own under
``base.``); the forward is `functional.matmul_4bit_multilora_grouped`: two kernel launches for 2 to 16 rows of input under `no_grad` /
`inference_mode` (the banks are parameters), which read the ids on the device, and the composed form for everything else.
`load_adapter` writes a slot in place, so a captured graph serves the new adapter at its next replay.
"""
import math
from typing import Sequence, Tuple

import torch
from torch import nn, Tensor

from .. import functional as F
from ._base import fold_leading
from .linear4bit import Linear4bit


def _forward(layers: Sequence['Linear4bitMultiLoRA'], x: Tensor, adapter_ids: Tensor, in_features: int) -> Tuple[Tensor, ...]:
    for layer in layers:
        if layer.base.weight_quant_state is None:
            raise RuntimeError("Weight not quantized. Call from_linear() or load weights first.")
    if tuple(adapter_ids.shape) != tuple(x.shape[:-1]):
        raise ValueError(f"adapter_ids has shape {tuple(adapter_ids.shape)}, x has rows {tuple(x.shape[:-1])}")
    compute_dtype = layers[0].base.compute_dtype
    rows, lead = fold_leading(x, in_features)
    ids = adapter_ids if x.dim() == 2 else adapter_ids.reshape(-1)      # a view of a contiguous tensor: an int32 one is still passed as it is
    if any(layer.base.compute_dtype != compute_dtype for layer in layers):
        ys = tuple(F.matmul_4bit_multilora_grouped(rows, [(layer.base.weight, layer.base.weight_quant_state)], [layer.bank()], ids,
                                                   [layer.base.bias], compute_dtype=layer.base.compute_dtype)[0] for layer in layers)
    else:
        ys = F.matmul_4bit_multilora_grouped(rows, [(layer.base.weight, layer.base.weight_quant_state) for layer in layers],
                                             [layer.bank() for layer in layers], ids, [layer.base.bias for layer in layers],
                                             compute_dtype=compute_dtype)
    if x.dim() <= 2:
        return ys
    return tuple(y.reshape(*lead, layer.out_features) for y, layer in zip(ys, layers))


class Linear4bitMultiLoRA(nn.Module):
    """`base`: the frozen Linear4bit; `lora_A` [num_adapters, r, in_features] (PEFT's Kaiming-uniform init per slot) and `lora_B`
    [num_adapters, out_features, r] (zeros): parameters in the base's weight dtype; `scaling`: an f32 buffer [num_adapters], every
    slot ``lora_alpha / r`` until `load_adapter` says otherwise."""

    def __init__(self, base: Linear4bit, num_adapters: int, r: int, lora_alpha: float = 1.0):
        super().__init__()
        if not isinstance(base, Linear4bit):
            raise TypeError(f"Linear4bitMultiLoRA: base is a {type(base).__name__}, not a Linear4bit")
        if not isinstance(num_adapters, int) or num_adapters < 1:
            raise ValueError(f"Linear4bitMultiLoRA: num_adapters must be a positive integer, got {num_adapters!r}")
        if not isinstance(r, int) or r < 1:
            raise ValueError(f"Linear4bitMultiLoRA: r must be a positive integer, got {r!r}")
        self.base = base
        self.in_features, self.out_features = base.in_features, base.out_features
        self.num_adapters, self.r, self.lora_alpha = num_adapters, r, lora_alpha
        state = base.weight_quant_state
        dtype = base.compute_dtype if state is None else state.dtype
        device = base.weight.device
        a = torch.empty(num_adapters, r, self.in_features, dtype=torch.float32)
        for s in range(num_adapters):
            nn.init.kaiming_uniform_(a[s], a=math.sqrt(5))       # PEFT's LoRA init: A Kaiming-uniform, B zeros, so every adapter starts at 0
        self.lora_A = nn.Parameter(a.to(device=device, dtype=dtype))
        self.lora_B = nn.Parameter(torch.zeros(num_adapters, self.out_features, r, dtype=dtype, device=device))
        self.register_buffer('scaling', torch.full((num_adapters,), lora_alpha / r, dtype=torch.float32, device=device))

    def bank(self) -> Tuple[Tensor, Tensor, Tensor]:
        return self.lora_A, self.lora_B, self.scaling

    @torch.no_grad()
    def load_adapter(self, slot: int, lora_A: Tensor, lora_B: Tensor, scaling: float) -> None:
        """Copy an adapter (lora_A [r, in_features], lora_B [out_features, r]) into `slot` IN PLACE: the bank's tensors keep their
        addresses, so tables built from them and graphs captured over them stay valid."""
        if not 0 <= slot < self.num_adapters:
            raise IndexError(f"Linear4bitMultiLoRA: slot {slot} of {self.num_adapters}")
        if tuple(lora_A.shape) != (self.r, self.in_features) or tuple(lora_B.shape) != (self.out_features, self.r):
            raise ValueError(f"Linear4bitMultiLoRA: the adapter has shapes {tuple(lora_A.shape)} / {tuple(lora_B.shape)}, the bank's "
                             f"slots hold {(self.r, self.in_features)} / {(self.out_features, self.r)} (pad a smaller rank with zeros)")
        self.lora_A[slot].copy_(lora_A)
        self.lora_B[slot].copy_(lora_B)
        self.scaling[slot] = float(scaling)

    def forward(self, x: Tensor, adapter_ids: Tensor) -> Tensor:
        return _forward([self], x, adapter_ids, self.in_features)[0]

    def extra_repr(self) -> str:
        return f'num_adapters={self.num_adapters}, r={self.r}, lora_alpha={self.lora_alpha}'


class Linear4bitMultiLoRAGroup(nn.Module):
    """`layers`: an nn.ModuleList of Linear4bitMultiLoRA with equal `in_features` and `num_adapters` (state-dict keys under
    ``layers.<i>.``).  ``forward(x, adapter_ids)`` returns one output per member from ONE call to
    `functional.matmul_4bit_multilora_grouped`, each within its bounds around what ``member(x, adapter_ids)`` defines."""

    def __init__(self, layers: Sequence[Linear4bitMultiLoRA]):
        super().__init__()
        layers = list(layers)
        if not layers:
            raise ValueError("Linear4bitMultiLoRAGroup needs at least one layer")
        for i, layer in enumerate(layers):
            if not isinstance(layer, Linear4bitMultiLoRA):
                raise TypeError(f"Linear4bitMultiLoRAGroup: layer {i} is a {type(layer).__name__}, not a Linear4bitMultiLoRA")
            if layer.in_features != layers[0].in_features:
                raise ValueError(f"Linear4bitMultiLoRAGroup: layer {i} has in_features={layer.in_features}, layer 0 has "
                                 f"in_features={layers[0].in_features}; the members share one input")
            if layer.num_adapters != layers[0].num_adapters:
                raise ValueError(f"Linear4bitMultiLoRAGroup: layer {i} has num_adapters={layer.num_adapters}, layer 0 has "
                                 f"num_adapters={layers[0].num_adapters}; the members share the rows' adapter ids")
        self.in_features = layers[0].in_features
        self.layers = nn.ModuleList(layers)

    def forward(self, x: Tensor, adapter_ids: Tensor) -> Tuple[Tensor, ...]:
        return _forward(list(self.layers), x, adapter_ids, self.in_features)

    def extra_repr(self) -> str:
        return f'in_features={self.in_features}, out_features={tuple(layer.out_features for layer in self.layers)}'
