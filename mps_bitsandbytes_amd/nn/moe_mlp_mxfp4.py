"""
MoEMLPMXFP4 — the expert MLP of a mixture-of-experts block (gpt-oss) in OCP MXFP4, on MI355X.

No counterpart in the reference.  The buffers carry the checkpoint's names and layouts, so an `mlp.experts.*` state dict loads as
it is: `gate_up_proj_blocks` uint8 [E, 2I, H / 32, 16] with interleaved rows (row 2j is gate j, row 2j + 1 is up j),
`gate_up_proj_scales` uint8 [E, 2I, H / 32], `gate_up_proj_bias` [E, 2I], `down_proj_blocks` uint8 [E, H, I / 32, 16],
`down_proj_scales` uint8 [E, H, I / 32], `down_proj_bias` [E, H].  The forward is `functional.moe_mlp_mxfp4`: three launches, the
gated activation an epilogue of the gate / up launch, the routed sum over the slots on the device.  The router
stays the caller's.  Inference only.
"""
from typing import Optional

import torch
from torch import Tensor

from .. import functional as F
from ._base import QuantizedModule, source_device

_BLOCK = 32


class MoEMLPMXFP4(QuantizedModule):
    _anchor = 'gate_up_proj_blocks'

    def __init__(self, num_experts: int, hidden_size: int, intermediate_size: int, bias: bool = True, alpha: float = 1.702,
                 limit: float = 7.0, device=None, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if num_experts <= 0:
            raise ValueError(f"MoEMLPMXFP4: num_experts ({num_experts}) must be positive")
        for name, size in (("hidden_size", hidden_size), ("intermediate_size", intermediate_size)):
            if size <= 0 or size % _BLOCK:
                raise ValueError(f"MoEMLPMXFP4: {name} ({size}) must be a positive multiple of the MX block, {_BLOCK}")
        self._init_linear(hidden_size, hidden_size, compute_dtype)
        E, H, I = num_experts, hidden_size, intermediate_size
        self.num_experts, self.hidden_size, self.intermediate_size = E, H, I
        self.alpha, self.limit = float(alpha), float(limit)
        self.register_buffer('gate_up_proj_blocks', torch.zeros(E, 2 * I, H // _BLOCK, 16, dtype=torch.uint8, device=device))
        self.register_buffer('gate_up_proj_scales', torch.full((E, 2 * I, H // _BLOCK), 127, dtype=torch.uint8, device=device))
        self.register_buffer('gate_up_proj_bias', torch.zeros(E, 2 * I, dtype=compute_dtype, device=device) if bias else None)
        self.register_buffer('down_proj_blocks', torch.zeros(E, H, I // _BLOCK, 16, dtype=torch.uint8, device=device))
        self.register_buffer('down_proj_scales', torch.full((E, H, I // _BLOCK), 127, dtype=torch.uint8, device=device))
        self.register_buffer('down_proj_bias', torch.zeros(E, H, dtype=compute_dtype, device=device) if bias else None)

    def forward(self, x: Tensor, expert_ids: Tensor, routing_weights: Tensor) -> Tensor:
        """x [T, H], f16 / bf16; expert_ids and routing_weights [T, A] -> [T, H] in x's dtype."""
        return F.moe_mlp_mxfp4(x, self.gate_up_proj_blocks, self.gate_up_proj_scales, self.gate_up_proj_bias, self.down_proj_blocks,
                               self.down_proj_scales, self.down_proj_bias, expert_ids, routing_weights, self.alpha, self.limit)

    @classmethod
    def from_weights(cls, gate: Tensor, up: Tensor, down: Tensor, gate_bias: Optional[Tensor] = None, up_bias: Optional[Tensor] = None,
                     down_bias: Optional[Tensor] = None, alpha: float = 1.702, limit: float = 7.0, device=None,
                     compute_dtype: Optional[torch.dtype] = None) -> 'MoEMLPMXFP4':
        """Interleave gate and up [E, I, H] into the checkpoint's rows (row 2j gate j, row 2j + 1 up j), and quantise them and
        down [E, H, I] on `device` with the HIP quantiser; the biases ([E, I], [E, I], [E, H]: all three or none) are copied."""
        if gate.dim() != 3 or tuple(up.shape) != tuple(gate.shape):
            raise ValueError(f"MoEMLPMXFP4.from_weights: gate and up must both be [E, I, H], got {tuple(gate.shape)} and {tuple(up.shape)}")
        E, I, H = gate.shape
        if tuple(down.shape) != (E, H, I):
            raise ValueError(f"MoEMLPMXFP4.from_weights: down {tuple(down.shape)} does not match [E, H, I] = {(E, H, I)}")
        biases = (gate_bias, up_bias, down_bias)
        if any(b is None for b in biases) != all(b is None for b in biases):
            raise ValueError("MoEMLPMXFP4.from_weights: give gate_bias, up_bias and down_bias, or none of them")
        has_bias = gate_bias is not None
        if has_bias and (tuple(gate_bias.shape) != (E, I) or tuple(up_bias.shape) != (E, I) or tuple(down_bias.shape) != (E, H)):
            raise ValueError(f"MoEMLPMXFP4.from_weights: the biases must be [E, I], [E, I] and [E, H] = {(E, I)}, {(E, I)}, {(E, H)}")
        device = source_device(gate, device)
        cd = compute_dtype if compute_dtype is not None else (gate.dtype if gate.dtype in (torch.float16, torch.bfloat16) else torch.bfloat16)
        layer = cls(E, H, I, bias=has_bias, alpha=alpha, limit=limit, device=device, compute_dtype=cd)
        gate_up = torch.stack((gate.detach().to(device), up.detach().to(device)), dim=2)                  # [E, I, 2, H]: rows 2j, 2j + 1
        codes, scales = F.quantize_mx(gate_up.reshape(E * 2 * I, H), "fp4")
        layer.gate_up_proj_blocks.copy_(codes.view(E, 2 * I, H // _BLOCK, 16))
        layer.gate_up_proj_scales.copy_(scales.view(E, 2 * I, H // _BLOCK))
        codes, scales = F.quantize_mx(down.detach().to(device).reshape(E * H, I), "fp4")
        layer.down_proj_blocks.copy_(codes.view(E, H, I // _BLOCK, 16))
        layer.down_proj_scales.copy_(scales.view(E, H, I // _BLOCK))
        if has_bias:
            layer.gate_up_proj_bias.copy_(torch.stack((gate_bias.detach(), up_bias.detach()), dim=2).reshape(E, 2 * I).to(cd).to(device))
            layer.down_proj_bias.copy_(down_bias.detach().to(cd).to(device))
        return layer

    def dequantize(self):
        """(gate [E, I, H], up [E, I, H], down [E, H, I]) in compute_dtype."""
        E, H, I = self.num_experts, self.hidden_size, self.intermediate_size
        gate_up = F.dequantize_mx(self.gate_up_proj_blocks.view(E * 2 * I, H // 2), self.gate_up_proj_scales.view(E * 2 * I, H // _BLOCK), "fp4",
                                  self.compute_dtype).view(E, I, 2, H)
        down = F.dequantize_mx(self.down_proj_blocks.view(E * H, I // 2), self.down_proj_scales.view(E * H, I // _BLOCK), "fp4",
                               self.compute_dtype).view(E, H, I)
        return gate_up[:, :, 0], gate_up[:, :, 1], down

    def extra_repr(self) -> str:
        return (f'num_experts={self.num_experts}, hidden_size={self.hidden_size}, intermediate_size={self.intermediate_size}, '
                f'bias={self.gate_up_proj_bias is not None}, alpha={self.alpha}, limit={self.limit}, quant_type=mxfp4')
