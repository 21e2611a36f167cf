"""
ctypes binding of the 8-bit optimizer library (include/mbnb_optim.h, libmbnb_optim.so).

A separate library from libmbnb_hip.so, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_optim.so")

ABI_VERSION = 1            # include/mbnb_optim.h MBNB_OPTIM_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_optim", "mps_bitsandbytes_amd.optim"
MAX_TENSORS = 48           # MBNB_OPTIM_MAX_TENSORS: descriptors per call (one kernel launch)
ADAM, ADAMW, LION, SGD_MOMENTUM, SGD_NESTEROV = 0, 1, 2, 3, 4
WEIGHT_DECAY = 1           # mbnb_optim_scalars.flags
FORCE_GENERIC = 1          # mbnb_optim_step flags


class Scalars(Structure):
    """mirror of ``struct mbnb_optim_scalars`` and of ``struct mbnb_paged_scalars`` (include/mbnb_paged.h), which has its layout"""
    _fields_ = [("beta1", c_float), ("one_minus_beta1", c_float), ("beta2", c_float), ("one_minus_beta2", c_float),
                ("eps", c_float), ("weight_decay", c_float), ("decay", c_float), ("neg_lr", c_float),
                ("flags", c_int32), ("pad_", c_int32)]


# the same layout as a numpy record: a whole table is built in one np.array call
DESC_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state1", "<u8"), ("absmax1", "<u8"), ("state2", "<u8"),
                       ("max2", "<u8"), ("numel", "<i8"), ("bc2_sqrt", "<f4"), ("neg_step_size", "<f4")])


class TensorDesc(Structure):
    """mirror of ``struct mbnb_optim_tensor``"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("state1", c_void_p), ("absmax1", c_void_p),
                ("state2", c_void_p), ("max2", c_void_p), ("numel", c_int64),
                ("bc2_sqrt", c_float), ("neg_step_size", c_float)]


_SIGNATURES = {
    "mbnb_optim_abi_version": (c_int, []),
    "mbnb_optim_last_error": (c_char_p, []),
    "mbnb_optim_step": (c_int, [c_int, c_int, c_int, c_int64, POINTER(Scalars), POINTER(TensorDesc), c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per mbnb_optim_step call (= one kernel launch) since the last reset_launch_log():
# (kind, param dtype, grad dtype, tensors in the call)
launch_log: List[Tuple[int, torch.dtype, torch.dtype, int]] = []


def reset_launch_log() -> None:
    launch_log.clear()


def available() -> bool:
    return _loader.loads(lib)


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it cannot be loaded."""
    if _lib is not None:
        return _lib
    return _loader.load(globals())


def check(status: int, what: str) -> None:
    if status != 0:
        raise _loader.failed(globals(), status, what)


def n_blocks(numel: int, block_size: int) -> int:
    return (numel + block_size - 1) // block_size


def plan(numels: Sequence[int], block_size: int, max_tensors: int = MAX_TENSORS) -> List[List[Tuple[int, int, int]]]:
    """How the library lays out one step: tensors in order, at most `max_tensors` per launch; in each launch tensor i
    owns global blocks [first, first + count) of its own, so no block (and no wave) ever covers two tensors.
    Returns, per launch, (tensor index, first block, block count) -- the same cumulative sums mbnb_optim_step forms."""
    chunks = []
    for c0 in range(0, len(numels), max_tensors):
        first, chunk = 0, []
        for i in range(c0, min(len(numels), c0 + max_tensors)):
            nb = n_blocks(int(numels[i]), block_size)
            chunk.append((i, first, nb))
            first += nb
        chunks.append(chunk)
    return chunks


def step(kind: int, param_dtype: torch.dtype, grad_dtype: torch.dtype, block_size: int, scalars: Scalars,
         descs: Sequence[tuple], stream: c_void_p, flags: int = 0) -> None:
    """Run one step over `descs` (any number of TensorDesc field tuples): one mbnb_optim_step call per launch of plan()."""
    handle = lib()
    for chunk in plan([d[6] for d in descs], block_size):
        part = np.array([descs[i] for i, _, _ in chunk], dtype=DESC_DTYPE)
        table = part.ctypes.data_as(POINTER(TensorDesc))
        check(handle.mbnb_optim_step(kind, DTYPE_CODE[param_dtype], DTYPE_CODE[grad_dtype], block_size, ctypes.byref(scalars),
                                     table, len(part), flags, stream), "step")
        launch_log.append((kind, param_dtype, grad_dtype, len(part)))
