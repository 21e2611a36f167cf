"""
Linear4bitGroup — several Linear4bit layers that are handed the same input (q / k / v, gate / up), run as one call.

No counterpart in the reference, whose layers run one at a time.  The members stay ordinary Linear4bit modules in an
nn.ModuleList, so their state-dict keys are their own under ``layers.<i>.``; the forward is
`functional.matmul_4bit_grouped`: one kernel launch for 1 to 16 rows of input (a decode step, alone or in a served batch), the
layers one by one for everything else, with each layer's own result bit for bit either way.
"""
from typing import Sequence, Tuple

from torch import nn, Tensor

from .. import functional as F
from ._base import fold_leading
from .linear4bit import Linear4bit


class Linear4bitGroup(nn.Module):
    """`layers`: the members, an nn.ModuleList of Linear4bit with equal `in_features`.  ``forward(x)`` returns one output per
    member, each what ``member(x)`` returns."""

    def __init__(self, layers: Sequence[Linear4bit]):
        super().__init__()
        layers = list(layers)
        if not layers:
            raise ValueError("Linear4bitGroup needs at least one layer")
        for i, layer in enumerate(layers):
            if not isinstance(layer, Linear4bit):
                raise TypeError(f"Linear4bitGroup: layer {i} is a {type(layer).__name__}, not a Linear4bit")
            if layer.in_features != layers[0].in_features:
                raise ValueError(f"Linear4bitGroup: layer {i} has in_features={layer.in_features}, layer 0 has "
                                 f"in_features={layers[0].in_features}; the members share one input")
        self.in_features = layers[0].in_features
        self.layers = nn.ModuleList(layers)

    @classmethod
    def from_linears(cls, linears: Sequence[nn.Linear], **from_linear_kwargs) -> 'Linear4bitGroup':
        """Quantize each nn.Linear with `Linear4bit.from_linear(linear, **from_linear_kwargs)`."""
        return cls([Linear4bit.from_linear(linear, **from_linear_kwargs) for linear in linears])

    def forward(self, x: Tensor) -> Tuple[Tensor, ...]:
        layers = list(self.layers)
        for layer in layers:
            if layer.weight_quant_state is None:
                raise RuntimeError("Weight not quantized. Call from_linear() or load weights first.")
        compute_dtype = layers[0].compute_dtype
        if any(layer.compute_dtype != compute_dtype for layer in layers):
            return tuple(layer(x) for layer in layers)
        rows, lead = fold_leading(x, self.in_features)
        ys = F.matmul_4bit_grouped(rows, [(layer.weight, layer.weight_quant_state) for layer in layers],
                                   [layer.bias for layer in layers], compute_dtype=compute_dtype)
        if x.dim() <= 2:
            return ys
        return tuple(y.reshape(*lead, layer.out_features) for y, layer in zip(ys, layers))

    def extra_repr(self) -> str:
        return f'in_features={self.in_features}, out_features={tuple(layer.out_features for layer in self.layers)}'
