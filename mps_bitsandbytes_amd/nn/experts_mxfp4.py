"""
ExpertsMXFP4 — the E expert weights of one projection of a mixture-of-experts layer, in OCP MXFP4, on MI355X.

No counterpart in the reference.  Buffers `weight` uint8 [E, N, K / 2] (even k in the low nibble) and `weight_scales` uint8
[E, N, K / 32]: the bytes of the [E, N, K / 32, 16] blocks and [E, N, K / 32] scales MXFP4 checkpoints ship.  The forward is
`functional.matmul_mxfp4_experts`: one launch evaluates every (token, slot) pair against the expert `expert_ids[t, a]` names,
the ids read on the device.  The routed sum over the slots and the activation between two projections are the
caller's.  Inference only: an input or a bias that requires grad, with grad enabled, raises NotImplementedError.
"""
from typing import Optional

import torch
from torch import nn, Tensor

from .. import functional as F
from ._base import QuantizedModule, source_device

_BLOCK = 32


class ExpertsMXFP4(QuantizedModule):
    _anchor = 'weight'

    def __init__(self, num_experts: int, in_features: int, out_features: int, bias: bool = True, device=None,
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if num_experts <= 0 or out_features <= 0:
            raise ValueError(f"ExpertsMXFP4: num_experts ({num_experts}) and out_features ({out_features}) must be positive")
        if in_features <= 0 or in_features % _BLOCK:
            raise ValueError(f"ExpertsMXFP4: in_features ({in_features}) must be a positive multiple of the MX block, {_BLOCK}")
        self._init_linear(in_features, out_features, compute_dtype)
        self.num_experts = num_experts
        self.register_buffer('weight', torch.zeros(num_experts, out_features, in_features // 2, dtype=torch.uint8, device=device))
        self.register_buffer('weight_scales', torch.full((num_experts, out_features, in_features // _BLOCK), 127, dtype=torch.uint8, device=device))
        if bias:
            self.bias = nn.Parameter(torch.zeros(num_experts, out_features, dtype=compute_dtype, device=device))
        else:
            self.register_parameter('bias', None)

    def forward(self, x: Tensor, expert_ids: Tensor) -> Tensor:
        """x [T, K] (shared by a token's slots) or [T, A, K] (a row per slot), f16 / bf16; expert_ids [T, A] -> [T, A, N] in x's dtype."""
        return F.matmul_mxfp4_experts(x, self.weight, self.weight_scales, expert_ids, self.bias)

    @classmethod
    def from_weights(cls, weight: Tensor, bias: Optional[Tensor] = None, device=None,
                     compute_dtype: Optional[torch.dtype] = None) -> 'ExpertsMXFP4':
        """Quantise expert weights [E, N, K] (and copy a bias [E, N]) on `device` with the HIP quantiser, expert by expert row."""
        if weight.dim() != 3:
            raise ValueError(f"ExpertsMXFP4.from_weights: weight must be [E, N, K], got {tuple(weight.shape)}")
        E, N, K = weight.shape
        if bias is not None and tuple(bias.shape) != (E, N):
            raise ValueError(f"ExpertsMXFP4.from_weights: bias {tuple(bias.shape)} does not match [E, N] = {(E, N)}")
        device = source_device(weight, device)
        wdtype = weight.dtype
        cd = compute_dtype if compute_dtype is not None else (wdtype if wdtype in (torch.float16, torch.bfloat16) else torch.bfloat16)
        layer = cls(E, K, N, bias=bias is not None, device=device, compute_dtype=cd)
        codes, scales = F.quantize_mx(weight.detach().to(device).reshape(E * N, K), "fp4")
        layer.weight.copy_(codes.view(E, N, K // 2))
        layer.weight_scales.copy_(scales.view(E, N, K // _BLOCK))
        if bias is not None:
            layer.bias.data.copy_(bias.detach().to(cd).to(device))
        return layer

    def dequantize(self) -> Tensor:
        """The weights as [num_experts, out_features, in_features] in compute_dtype."""
        E, N, K = self.num_experts, self.out_features, self.in_features
        return F.dequantize_mx(self.weight.view(E * N, K // 2), self.weight_scales.view(E * N, K // _BLOCK), "fp4", self.compute_dtype).view(E, N, K)

    def extra_repr(self) -> str:
        return f'num_experts={self.num_experts}, {self._repr_core()}, quant_type=mxfp4'
