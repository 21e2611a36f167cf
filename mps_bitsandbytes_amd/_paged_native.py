"""
ctypes binding of the fused full-precision optimizer step (include/mbnb_paged.h, libmbnb_paged.so).

A separate library from the other four, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_paged.so")

ABI_VERSION = 1            # include/mbnb_paged.h MBNB_PAGED_ABI_VERSION
MAX_SEGMENTS = 48          # MBNB_PAGED_MAX_SEGMENTS: segments per call (one kernel launch)
ADAM, ADAMW, LION = 0, 1, 2
F16, BF16, F32 = 0, 1, 2
DTYPE_CODE = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}
WEIGHT_DECAY = 1           # mbnb_paged_scalars.flags
FORCE_SCALAR = 1           # mbnb_paged_step flags


class Scalars(Structure):
    """mirror of ``struct mbnb_paged_scalars``"""
    _fields_ = [("beta1", c_float), ("one_minus_beta1", c_float), ("beta2", c_float), ("one_minus_beta2", c_float),
                ("eps", c_float), ("weight_decay", c_float), ("decay", c_float), ("neg_lr", c_float),
                ("flags", c_int32), ("pad_", c_int32)]


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
    try:
        lib()
        return True
    except RuntimeError:
        return False


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it cannot be loaded."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise RuntimeError(_load_error)
    if not os.path.exists(LIB_PATH):
        _load_error = (f"mps_bitsandbytes_amd.optim: native library {LIB_PATH} not found. Build it with "
                       f"`make -C {os.path.join(_HERE, 'csrc')}`. There is no Python fallback.")
        raise RuntimeError(_load_error)
    try:
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.mbnb_paged_abi_version() != ABI_VERSION:
            raise OSError(f"ABI version mismatch: library reports {handle.mbnb_paged_abi_version()}, binding expects {ABI_VERSION}")
    except (OSError, AttributeError) as e:
        _load_error = f"mps_bitsandbytes_amd.optim: cannot load {LIB_PATH}: {e}"
        raise RuntimeError(_load_error) from e
    _lib = handle
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().mbnb_paged_last_error().decode(errors="replace")
        raise RuntimeError(f"mps_bitsandbytes_amd.optim.paged.{what} failed (status {status}): {msg}")


def step(kind: int, dtype: torch.dtype, scalars: Scalars, segments: Sequence[tuple], stream: c_void_p, flags: int = 0) -> None:
    """Run one step over `segments` (any number of Segment field tuples): one mbnb_paged_step call per MAX_SEGMENTS of them."""
    handle = lib()
    for c0 in range(0, len(segments), MAX_SEGMENTS):
        part = np.array(segments[c0:c0 + MAX_SEGMENTS], dtype=SEG_DTYPE)
        table = part.ctypes.data_as(POINTER(Segment))
        check(handle.mbnb_paged_step(kind, DTYPE_CODE[dtype], ctypes.byref(scalars), table, len(part), flags, stream), "step")
        launch_log.append((kind, dtype, len(part)))
