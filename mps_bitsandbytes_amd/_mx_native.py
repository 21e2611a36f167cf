"""
ctypes binding of the OCP MX quantiser and the MXFP4 linear (include/mbnb_mx.h, libmbnb_mx.so).

A separate library from the other nine, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_mx.so")

ABI_VERSION = 2            # include/mbnb_mx.h MBNB_MX_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_mx", "mps_bitsandbytes_amd.mx"
FP4, FP8 = 0, 1            # MBNB_MX_FP4 / MBNB_MX_FP8
ELEM_CODE = {"fp4": FP4, "fp8": FP8}
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
BLOCK = 32                 # elements per scale byte
TM, TN, KS = 128, 128, 128  # MBNB_MX_TILE_M / _TILE_N / _K_STEP: k_gemm_mx's workgroup tile and K-step
DECODE_ROWS = 16           # MBNB_MX_DECODE_ROWS: the most activation rows of one k_mx_decode workgroup pass
NAN_SCALE = 0xFF

_SIGNATURES = {
    "mbnb_mx_abi_version": (c_int, []),
    "mbnb_mx_last_error": (c_char_p, []),
    "mbnb_mx_last_launch": (c_char_p, []),
    "mbnb_mx_quantize": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mbnb_mx_dequantize": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "mbnb_mx_workspace_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "mbnb_mx_linear": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int,
                               c_void_p, c_int64, c_void_p]),
    "mbnb_mx_linear_weight_only": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int,
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
    return lib().mbnb_mx_last_launch().decode()


def workspace_bytes(M: int, K: int, act_elem: int) -> int:
    n = int(lib().mbnb_mx_workspace_bytes(M, K, act_elem))
    if n < 0:
        check(n, "workspace_bytes")
    return n
