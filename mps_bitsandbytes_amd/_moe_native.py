"""
ctypes binding of the MXFP4 expert linears (include/mbnb_moe.h, libmbnb_moe.so).

A separate library from the other ten, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_moe.so")

ABI_VERSION = 1            # include/mbnb_moe.h MBNB_MOE_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_moe", "mps_bitsandbytes_amd.moe"
ERR_ARG, ERR_SHAPE = -1, -2
BLOCK = 32                 # elements per scale byte
MAX_PAIRS = 1024           # MBNB_MOE_MAX_PAIRS: the most (token, slot) pairs of one launch
TILE_N = 16                # weight rows of one k_mx_experts workgroup
ROWS = 16                  # listed pairs per pass of its decode loop

_SIGNATURES = {
    "mbnb_moe_abi_version": (c_int, []),
    "mbnb_moe_last_error": (c_char_p, []),
    "mbnb_moe_last_launch": (c_char_p, []),
    "mbnb_moe_mxfp4_experts": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                       c_void_p, c_int, c_void_p, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None


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


def last_launch() -> str:
    return lib().mbnb_moe_last_launch().decode()
