"""
ctypes binding of the prefill-sized grouped GEMM over MXFP4 experts (include/mbnb_moegemm.h, libmbnb_moegemm.so).

A separate library from the other thirteen, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_moegemm.so")

ABI_VERSION = 1            # include/mbnb_moegemm.h MBNB_MOEGEMM_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_moegemm", "mps_bitsandbytes_amd.moegemm"
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
BLOCK = 32                 # elements per scale byte
ROW_TILE = 64              # MBNB_MOEGEMM_ROW_TILE: the listed pairs of one expert that a workgroup takes
MAX_PAIRS = 1 << 20        # MBNB_MOEGEMM_MAX_PAIRS: the most (token, slot) pairs of one call
MAX_EXPERTS = 1024         # MBNB_MOEGEMM_MAX_EXPERTS
TILE_N = 48                # weight rows of one k_mx_experts_grouped workgroup: three B fragments

_SIGNATURES = {
    "mbnb_moegemm_abi_version": (c_int, []),
    "mbnb_moegemm_last_error": (c_char_p, []),
    "mbnb_moegemm_last_launch": (c_char_p, []),
    "mbnb_moegemm_plan_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_moegemm_plan": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "mbnb_moegemm_experts": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                     c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "mbnb_moegemm_gate_up_glu": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                         c_void_p, c_int, c_float, c_float, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "mbnb_moegemm_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_moegemm_down_sum": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
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


def max_tiles(P: int, E: int) -> int:
    """The bound on the tile table's entries that sizes the plan and the grid: it holds for every routing."""
    return min(E, P) + P // ROW_TILE


def plan_bytes(P: int, E: int) -> int:
    n = lib().mbnb_moegemm_plan_bytes(P, E)
    if n < 0:
        check(int(n), "plan_bytes")
    return int(n)


def workspace_bytes(P: int, N: int) -> int:
    n = lib().mbnb_moegemm_workspace_bytes(P, N)
    if n < 0:
        check(int(n), "workspace_bytes")
    return int(n)


def last_launch() -> str:
    return lib().mbnb_moegemm_last_launch().decode()
