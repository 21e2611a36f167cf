"""
ctypes binding of the grouped GEMM over MXFP4 experts on the block-scaled MFMA (include/mbnb_moemx.h, libmbnb_moemx.so).

A separate library from the other fourteen, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_moemx.so")

ABI_VERSION = 1            # include/mbnb_moemx.h MBNB_MOEMX_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_moemx", "mps_bitsandbytes_amd.moemx"
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
FP4, FP8 = 0, 1            # MBNB_MOEMX_FP4 / MBNB_MOEMX_FP8: the values of _mx_native.ELEM_CODE
BLOCK = 32                 # elements per scale byte
ROW_TILE = 64              # MBNB_MOEMX_ROW_TILE: the R of the plan it reads (_moegemm_native.ROW_TILE)
COL_TILE = 256             # MBNB_MOEMX_COL_TILE: weight rows of one k_mx_experts_scaled workgroup
K_STEP = 128               # MBNB_MOEMX_K_STEP
MAX_PAIRS = 1 << 20        # MBNB_MOEMX_MAX_PAIRS
MAX_EXPERTS = 1024         # MBNB_MOEMX_MAX_EXPERTS

_SIGNATURES = {
    "mbnb_moemx_abi_version": (c_int, []),
    "mbnb_moemx_last_error": (c_char_p, []),
    "mbnb_moemx_last_launch": (c_char_p, []),
    "mbnb_moemx_experts": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                   c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "mbnb_moemx_gate_up_glu": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                       c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "mbnb_moemx_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_moemx_down_sum": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                    c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(P: int, N: int) -> int:
    n = lib().mbnb_moemx_workspace_bytes(P, N)
    if n < 0:
        check(int(n), "workspace_bytes")
    return int(n)


def last_launch() -> str:
    return lib().mbnb_moemx_last_launch().decode()
