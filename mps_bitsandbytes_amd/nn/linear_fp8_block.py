"""
LinearFP8Block — a linear layer over a block-scaled FP8 checkpoint weight (DeepSeek-V3 / R1, the Qwen3 -FP8 releases) on MI355X.

Buffers under the checkpoint's own keys: `weight` [N, K] uint8 (E4M3 codes; a float8_e4m3fn tensor in an incoming state dict is
viewed as uint8 on load), `weight_scale_inv` f32 [ceil(N / 128), ceil(K / 128)] and an optional `bias`.  The forward is
`functional.linear_fp8_block`: the activation quantised per row and 128-wide k group, both operands on the FP8 MFMA, every
128-k block folded into the f32 sum with its own scale product.  Inference only.

`act_format` (a class attribute, "fp8" by default: that forward) selects what becomes of the activation: "none" leaves it in its own
dtype and runs `functional.linear_fp8_block_weight_only` over the same buffers, the one-launch form for the 1 to 16 rows of a
token-generation step.
"""
import torch
from torch import nn, Tensor

from .. import functional as F
from ._base import QuantizedModule, source_device

_BLOCK = 128


class LinearFP8Block(QuantizedModule):
    _anchor = 'weight'
    act_format = "fp8"         # "none": the weight-only decode forward over the same buffers; set on the class or on an instance

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_linear(in_features, out_features, compute_dtype)
        self.register_buffer('weight', torch.zeros(out_features, in_features, dtype=torch.uint8, device=device))
        self.register_buffer('weight_scale_inv', torch.ones(-(-out_features // _BLOCK), -(-in_features // _BLOCK), dtype=torch.float32, device=device))
        self._init_bias(bias, device, as_parameter=False)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + 'weight')
        if w is not None and w.dtype == torch.float8_e4m3fn:
            state_dict[prefix + 'weight'] = w.view(torch.uint8)      # the codes as they lie in memory
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x: Tensor) -> Tensor:
        if self.act_format == "none":
            return F.linear_fp8_block_weight_only(x, self.weight, self.weight_scale_inv, self.bias)
        if self.act_format != "fp8":
            raise ValueError(f"LinearFP8Block: unknown act_format {self.act_format!r} (supported: 'fp8', 'none')")
        return F.linear_fp8_block(x, self.weight, self.weight_scale_inv, self.bias)

    @classmethod
    def from_linear(cls, linear: nn.Linear, device=None) -> 'LinearFP8Block':
        """Quantise an nn.Linear on `device` with `functional.quantize_fp8_blocks`."""
        device = source_device(linear.weight, device)
        dtype = linear.weight.dtype if linear.weight.dtype in (torch.float16, torch.bfloat16, torch.float32) else torch.bfloat16
        layer = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, device=device, compute_dtype=dtype)
        q, scales = F.quantize_fp8_blocks(linear.weight.data.to(device))
        layer.weight.copy_(q)
        layer.weight_scale_inv.copy_(scales)
        layer._copy_bias_from(linear, device)
        return layer

    def extra_repr(self) -> str:
        return f'{self._repr_core()}, quant_type=fp8_e4m3, weight_block_size=[{_BLOCK}, {_BLOCK}]'
