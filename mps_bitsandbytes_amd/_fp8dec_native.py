"""
ctypes binding of the weight-only decode linear over a block-scaled FP8 weight (include/mbnb_fp8dec.h, libmbnb_fp8dec.so): one launch
for the 1 to 16 activation rows of a token-generation step, the activation left in its own dtype, the E4M3 weight decoded in registers.

A separate library from the other seventeen, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_fp8dec.so")

ABI_VERSION = 1            # include/mbnb_fp8dec.h MBNB_FP8DEC_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_fp8dec", "mps_bitsandbytes_amd.fp8dec"
ERR_ARG, ERR_SHAPE = -1, -2
BLOCK = 128                # MBNB_FP8DEC_BLOCK: the edge of a scale block
ROWS = 16                  # MBNB_FP8DEC_ROWS: weight rows, and activation rows of a chunk, of an MFMA workgroup

_SIGNATURES = {
    "mbnb_fp8dec_abi_version": (c_int, []),
    "mbnb_fp8dec_last_error": (c_char_p, []),
    "mbnb_fp8dec_last_launch": (c_char_p, []),
    "mbnb_fp8dec_linear_weight_only": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int,
                                               c_void_p]),
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
    return lib().mbnb_fp8dec_last_launch().decode()
