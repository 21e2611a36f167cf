"""
ctypes binding of the fused full-precision optimizer step (include/mbnb_paged.h, libmbnb_paged.so).

A separate library from the other four, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too
from ._optim_native import Scalars          # struct mbnb_paged_scalars: the layout of mbnb_optim_scalars

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_paged.so")

ABI_VERSION = 1            # include/mbnb_paged.h MBNB_PAGED_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_paged", "mps_bitsandbytes_amd.optim.paged"
MAX_SEGMENTS = 48          # MBNB_PAGED_MAX_SEGMENTS: segments per call (one kernel launch)
ADAM, ADAMW, LION = 0, 1, 2
WEIGHT_DECAY = 1           # mbnb_paged_scalars.flags
FORCE_SCALAR = 1           # mbnb_paged_step flags


# the same layout as a numpy record: a whole table is built in one np.array call
SEG_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
                      ("bc2_sqrt", "<f4"), ("neg_step_size", "<f4")])


class Segment(Structure):
    """mirror of ``struct mbnb_paged_segment``"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("numel", c_int64), ("bc2_sqrt", c_float), ("neg_step_size", c_float)]


_SIGNATURES = {
    "mbnb_paged_abi_version": (c_int, []),
    "mbnb_paged_last_error": (c_char_p, []),
    "mbnb_paged_step": (c_int, [c_int, c_int, POINTER(Scalars), POINTER(Segment), c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per mbnb_paged_step call (= one kernel launch) since the last reset_launch_log(): (kind, dtype, segments in the call)
launch_log: List[Tuple[int, torch.dtype, int]] = []


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


def step(kind: int, dtype: torch.dtype, scalars: Scalars, segments: Sequence[tuple], stream: c_void_p, flags: int = 0) -> None:
    """Run one step over `segments` (any number of Segment field tuples): one mbnb_paged_step call per MAX_SEGMENTS of them."""
    handle = lib()
    for c0 in range(0, len(segments), MAX_SEGMENTS):
        part = np.array(segments[c0:c0 + MAX_SEGMENTS], dtype=SEG_DTYPE)
        table = part.ctypes.data_as(POINTER(Segment))
        check(handle.mbnb_paged_step(kind, DTYPE_CODE[dtype], ctypes.byref(scalars), table, len(part), flags, stream), "step")
        launch_log.append((kind, dtype, len(part)))
