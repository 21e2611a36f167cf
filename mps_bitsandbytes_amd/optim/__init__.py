"""
8-bit optimizers (reference: mps_bitsandbytes/optim): Adam8bit, AdamW8bit, Lion8bit, SGD8bit.

Their state is stored blockwise in 8 bits (the reference's layout, so state_dicts can be exchanged) and each step is
one fused HIP launch per 48 tensors of a parameter group and dtype pair (libmbnb_optim.so, include/mbnb_optim.h).  Parameters must be on
a ROCm ('cuda') device; there is no CPU path.  The reference's paged optimizers (PagedAdam, ...) are out of scope.
"""
from .adam8bit import (
    Adam8bit, AdamW8bit,
    quantize_state, dequantize_state,
    quantize_state_unsigned, dequantize_state_unsigned,
)
from .lion8bit import Lion8bit
from .sgd8bit import SGD8bit

__all__ = [
    'Adam8bit', 'AdamW8bit', 'Lion8bit', 'SGD8bit',
    'quantize_state', 'dequantize_state', 'quantize_state_unsigned', 'dequantize_state_unsigned',
]
