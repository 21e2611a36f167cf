"""
LinearMXFP4 — a linear layer whose weight is OCP MXFP4 (E2M1 codes, one E8M0 scale byte per 32 input features), on MI355X.

No counterpart in the reference.  Buffers `weight` uint8 [N, K / 2] (even k in the low nibble) and `weight_scales` uint8
[N, K / 32], both row-major: the tensors MXFP4 checkpoints ship.  The forward is `functional.matmul_mxfp4`: the
activation rows are quantised to `act_format` ("fp8": E4M3, "fp4": E2M1) and the product runs on gfx950's block-scaled MFMA.
`act_format="none"` is the weight-only form for token generation: the activation is not quantised, and one launch streams and
decodes the weight (bf16 calls of more than 16 rows run dequantise + the dense GEMM instead; the same sum in another order).
Inference only: an input or a bias that requires grad, with grad enabled, raises NotImplementedError.
"""
from typing import Optional

import torch
from torch import nn, Tensor

from .. import functional as F
from ._base import QuantizedModule, source_device

_BLOCK = 32


class LinearMXFP4(QuantizedModule):
    _anchor = 'weight'

    def __init__(self, in_features: int, out_features: int, bias: bool = True, act_format: str = "fp8", device=None,
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if in_features <= 0 or in_features % _BLOCK:
            raise ValueError(f"LinearMXFP4: in_features ({in_features}) must be a positive multiple of the MX block, {_BLOCK}")
        if act_format not in ("fp4", "fp8", "none"):
            raise ValueError(f"LinearMXFP4: unknown act_format {act_format!r} (supported: 'fp4', 'fp8', 'none')")
        self._init_linear(in_features, out_features, compute_dtype)
        self.act_format = act_format
        self.register_buffer('weight', torch.zeros(out_features, in_features // 2, dtype=torch.uint8, device=device))
        self.register_buffer('weight_scales', torch.full((out_features, in_features // _BLOCK), 127, dtype=torch.uint8, device=device))
        self._init_bias(bias, device)

    def forward(self, x: Tensor) -> Tensor:
        """In the input's dtype (f16 / bf16 / f32); any other input dtype computes in `compute_dtype`."""
        dtype = x.dtype if x.dtype in (torch.float16, torch.bfloat16, torch.float32) else self.compute_dtype
        return F.matmul_mxfp4(x, self.weight, self.weight_scales, self.bias, self.act_format, dtype)

    @classmethod
    def from_linear(cls, linear: nn.Linear, act_format: str = "fp8", device=None,
                    compute_dtype: Optional[torch.dtype] = None) -> 'LinearMXFP4':
        """Quantise an nn.Linear on `device` with the HIP quantiser; `act_format` as in the constructor ("none": weight-only)."""
        device = source_device(linear.weight, device)
        wdtype = linear.weight.dtype
        cd = compute_dtype if compute_dtype is not None else (wdtype if wdtype in (torch.float16, torch.bfloat16, torch.float32) else torch.bfloat16)
        layer = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, act_format=act_format, device=device,
                    compute_dtype=cd)
        codes, scales = F.quantize_mx(linear.weight.data.to(device), "fp4")
        layer.weight.copy_(codes)
        layer.weight_scales.copy_(scales)
        layer._copy_bias_from(linear, device)
        return layer

    def dequantize(self) -> Tensor:
        """The weight as [out_features, in_features] in compute_dtype."""
        return F.dequantize_mx(self.weight, self.weight_scales, "fp4", self.compute_dtype)

    def extra_repr(self) -> str:
        return f'{self._repr_core()}, quant_type=mxfp4, act_format={self.act_format}'
