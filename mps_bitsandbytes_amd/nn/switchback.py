"""
SwitchBackLinear: an int8 forward with a trained 16-bit master weight (reference: nn/switchback.py; arXiv 2304.13013).

Same surface as the reference: buffers `weight_int8` int8 [out, in] and `weight_scales` f32 [out] (the row absmax), parameters
`weight_fp` and `bias` in `compute_dtype`, `from_linear`, `sync_weights`, `_update_int8_pending`, and SwitchBackLinearCallback.
The forward runs `functional.switchback_linear` (libmbnb_train.so): the int8 weight decoded with the reference's rule
round_T(q * round_T(s / 127)), the dense MFMA GEMM, then the bias as a separate rounding.  The backward multiplies with `weight_fp`:
dX through the input-gradient kernels of the quantised linears, dW = dY^T . X through the weight-gradient GEMM.  Re-quantisation
(`sync_weights`) is the HIP quantize_rowwise, bit-exact against the reference.
"""
import torch
from torch import nn, Tensor

from .. import functional as F

SwitchBackFunction = F._SwitchBackFunction


class SwitchBackLinear(nn.Module):
    """Linear layer with an int8 forward and a 16-bit trainable weight (reference nn/switchback.py:97-241)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, compute_dtype=torch.float16, device=None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.compute_dtype = compute_dtype
        self.register_buffer('weight_int8', torch.zeros(out_features, in_features, dtype=torch.int8, device=device))
        self.register_buffer('weight_scales', torch.ones(out_features, dtype=torch.float32, device=device))
        self.weight_fp = nn.Parameter(torch.zeros(out_features, in_features, dtype=compute_dtype, device=device))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features, dtype=compute_dtype, device=device))
        else:
            self.register_parameter('bias', None)
        self._update_int8_pending = False

    def forward(self, x: Tensor) -> Tensor:
        # the reference re-quantises here only when training with an update pending; it never sets the flag itself
        if self.training and self._update_int8_pending:
            self._update_int8_weights()
            self._update_int8_pending = False
        return F.switchback_linear(x, self.weight_int8, self.weight_scales, self.weight_fp, self.bias)

    def _update_int8_weights(self):
        """Re-quantise the int8 weights from weight_fp (row-wise absmax)."""
        with torch.no_grad():
            weight_int8, weight_scales = F.quantize_rowwise(self.weight_fp.data)
            self.weight_int8.copy_(weight_int8)
            self.weight_scales.copy_(weight_scales)

    def sync_weights(self):
        """Re-quantise the int8 weights used by the forward from weight_fp; call it after optimizer.step()."""
        self._update_int8_weights()

    @classmethod
    def from_linear(cls, linear: nn.Linear, device=None) -> 'SwitchBackLinear':
        """Convert an nn.Linear: weight_fp and bias in the linear's dtype if that is f16 / bf16, else f16; the int8 codes and scales
        from the ORIGINAL-precision weight."""
        if device is None:
            device = linear.weight.device
        dtype = linear.weight.dtype
        if dtype not in (torch.float16, torch.bfloat16):
            dtype = torch.float16
        layer = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, compute_dtype=dtype, device=device)
        layer.weight_fp.data.copy_(linear.weight.data.to(dtype))
        weight_int8, weight_scales = F.quantize_rowwise(linear.weight.data.to(device))
        layer.weight_int8.copy_(weight_int8)
        layer.weight_scales.copy_(weight_scales)
        if linear.bias is not None:
            layer.bias.data.copy_(linear.bias.data.to(dtype))
        return layer

    def extra_repr(self) -> str:
        return f'in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}'


class SwitchBackLinearCallback:
    """Syncs the int8 weights of every SwitchBackLinear of a model (reference nn/switchback.py:244-268).

        callback = SwitchBackLinearCallback(model)
        loss.backward(); optimizer.step(); callback.sync()
    """

    def __init__(self, model: nn.Module):
        self.switchback_layers = []
        for module in model.modules():
            if isinstance(module, SwitchBackLinear):
                self.switchback_layers.append(module)

    def sync(self):
        """Sync all SwitchBackLinear layers."""
        for layer in self.switchback_layers:
            layer.sync_weights()
