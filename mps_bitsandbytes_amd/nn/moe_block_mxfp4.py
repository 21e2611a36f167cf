"""
MoERouterTopK and MoEBlockMXFP4 — the router of a mixture-of-experts block (gpt-oss) and the whole block, on MI355X.

No counterpart in the reference.  The buffers carry the checkpoint's names, so an `mlp.*` state dict loads as it is:
`router.weight` [E, H], `router.bias` [E] and `experts.*` (MoEMLPMXFP4).  The router's forward is `functional.moe_router_topk`:
one launch for the logits in f32, the top-k selection with ties to the lower expert, and the softmax over the selected logits
(DESIGN.md §30).  The block's forward is `experts(x, *router(x))`: four launches in three C calls, with no torch op, no
synchronisation and no host-side tensor between the hidden state and its output.  Inference only.
"""
import torch
from torch import Tensor, nn

from .. import functional as F
from ._base import source_device
from .moe_mlp_mxfp4 import MoEMLPMXFP4


class MoERouterTopK(nn.Module):
    def __init__(self, hidden_size: int, num_experts: int, top_k: int = 4, bias: bool = True, device=None,
                 dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if hidden_size <= 0 or hidden_size % 8:
            raise ValueError(f"MoERouterTopK: hidden_size ({hidden_size}) must be a positive multiple of 8")
        if num_experts <= 0:
            raise ValueError(f"MoERouterTopK: num_experts ({num_experts}) must be positive")
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"MoERouterTopK: top_k ({top_k}) must be from 1 to min(num_experts, 32) = {min(num_experts, 32)}")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"MoERouterTopK: dtype must be float16 or bfloat16, got {dtype}")
        self.hidden_size, self.num_experts, self.top_k = hidden_size, num_experts, top_k
        self.register_buffer('weight', torch.zeros(num_experts, hidden_size, dtype=dtype, device=device))
        self.register_buffer('bias', torch.zeros(num_experts, dtype=dtype, device=device) if bias else None)

    def forward(self, x: Tensor):
        """x [..., H] in the weight's dtype -> (expert_ids int32 [T, top_k], routing_weights f32 [T, top_k]), T the flattened tokens."""
        return F.moe_router_topk(x, self.weight, self.bias, self.top_k)

    @classmethod
    def from_linear(cls, linear: nn.Linear, top_k: int = 4, device=None, dtype: torch.dtype = None) -> 'MoERouterTopK':
        """Copy the weight [E, H] and the bias of an nn.Linear; `dtype` defaults to the linear's when that is 16-bit, else bfloat16."""
        w = linear.weight.detach()
        if dtype is None:
            dtype = w.dtype if w.dtype in (torch.float16, torch.bfloat16) else torch.bfloat16
        device = source_device(w, device)
        layer = cls(linear.in_features, linear.out_features, top_k=top_k, bias=linear.bias is not None, device=device, dtype=dtype)
        layer.weight.copy_(w.to(dtype).to(device))
        if linear.bias is not None:
            layer.bias.copy_(linear.bias.detach().to(dtype).to(device))
        return layer

    def extra_repr(self) -> str:
        return (f'hidden_size={self.hidden_size}, num_experts={self.num_experts}, top_k={self.top_k}, bias={self.bias is not None}, '
                f'dtype={self.weight.dtype}')


class MoEBlockMXFP4(nn.Module):
    def __init__(self, num_experts: int, hidden_size: int, intermediate_size: int, top_k: int = 4, bias: bool = True,
                 alpha: float = 1.702, limit: float = 7.0, device=None, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self.router = MoERouterTopK(hidden_size, num_experts, top_k=top_k, bias=bias, device=device, dtype=compute_dtype)
        self.experts = MoEMLPMXFP4(num_experts, hidden_size, intermediate_size, bias=bias, alpha=alpha, limit=limit, device=device,
                                   compute_dtype=compute_dtype)

    def forward(self, x: Tensor, return_routing: bool = False):
        """x [..., H], f16 / bf16 -> [..., H] in x's dtype; with return_routing also (expert_ids, routing_weights) [T, top_k]"""
        x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
        ids, rw = self.router(x2)
        out = self.experts(x2, ids, rw)
        out = out if x.dim() == 2 else out.reshape(*x.shape[:-1], out.shape[-1])
        return (out, (ids, rw)) if return_routing else out

    def extra_repr(self) -> str:
        return f'top_k={self.router.top_k}'
