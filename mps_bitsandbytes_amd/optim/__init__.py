"""
Optimizers (reference: mps_bitsandbytes/optim): Adam8bit, AdamW8bit, Lion8bit, SGD8bit and PagedAdam, PagedAdamW, PagedLion.

Their state is stored blockwise in 8 bits (the reference's layout, so state_dicts can be exchanged) and each step is
one fused HIP launch per 48 tensors of a parameter group and dtype pair (libmbnb_optim.so, include/mbnb_optim.h).  Parameters must be on
a ROCm ('cuda') device; there is no CPU path.

The paged optimizers keep full-precision moments in the parameter's dtype, in pinned host memory (page_to_cpu=True: pages of them
stream through a fixed ring of device staging slots each step) or on the device (page_to_cpu=False), and step them with one fused
HIP kernel (libmbnb_paged.so, include/mbnb_paged.h; optim/paged.py).
"""
from .adam8bit import (
    Adam8bit, AdamW8bit,
    quantize_state, dequantize_state,
    quantize_state_unsigned, dequantize_state_unsigned,
)
from .lion8bit import Lion8bit
from .sgd8bit import SGD8bit
from .paged import PagedAdam, PagedAdamW, PagedLion

__all__ = [
    'Adam8bit', 'AdamW8bit', 'Lion8bit', 'SGD8bit', 'PagedAdam', 'PagedAdamW', 'PagedLion',
    'quantize_state', 'dequantize_state', 'quantize_state_unsigned', 'dequantize_state_unsigned',
]
