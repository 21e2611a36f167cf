"""
ctypes binding of the MXFP4 mixture-of-experts MLP (include/mbnb_moemlp.h, libmbnb_moemlp.so).

A separate library from the other eleven, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_moemlp.so")

ABI_VERSION = 1            # include/mbnb_moemlp.h MBNB_MOEMLP_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_moemlp", "mps_bitsandbytes_amd.moemlp"
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
BLOCK = 32                 # elements per scale byte
MAX_PAIRS = 1024           # MBNB_MOEMLP_MAX_PAIRS: the most (token, slot) pairs of one call
MAX_EXPERTS = 1024         # MBNB_MOEMLP_MAX_EXPERTS: a presence byte per expert in LDS
TILE_N = 16                # weight rows of one k_mx_experts_rt workgroup: 8 (gate, up) pairs of the gate / up launch
ROWS = 16                  # listed pairs per pass of its decode loop

_SIGNATURES = {
    "mbnb_moemlp_abi_version": (c_int, []),
    "mbnb_moemlp_last_error": (c_char_p, []),
    "mbnb_moemlp_last_launch": (c_char_p, []),
    "mbnb_moemlp_gate_up_glu": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                        c_void_p, c_int, c_float, c_float, c_void_p, c_int, c_void_p]),
    "mbnb_moemlp_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "mbnb_moemlp_down_sum": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                     c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(T: int, A: int, N: int) -> int:
    n = lib().mbnb_moemlp_workspace_bytes(T, A, N)
    if n < 0:
        check(int(n), "workspace_bytes")
    return int(n)


def last_launch() -> str:
    return lib().mbnb_moemlp_last_launch().decode()
