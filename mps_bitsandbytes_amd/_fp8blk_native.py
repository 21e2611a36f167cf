"""
ctypes binding of the block-scaled FP8 linear (include/mbnb_fp8blk.h, libmbnb_fp8blk.so): the group and block quantisers to OCP
E4M3 and the GEMM over two E4M3 operands with 1 x 128 activation scales and 128 x 128 weight scales on the FP8 MFMA.

A separate library from the other sixteen, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_fp8blk.so")

ABI_VERSION = 1            # include/mbnb_fp8blk.h MBNB_FP8BLK_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_fp8blk", "mps_bitsandbytes_amd.fp8blk"
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
BLOCK = 128                # MBNB_FP8BLK_BLOCK: the edge of a scale block
TM, TN, KS = 128, 128, 128   # MBNB_FP8BLK_TILE_M / _TILE_N / _K_STEP
STEPS_IN_FLIGHT = 2        # MBNB_FP8BLK_STEPS_IN_FLIGHT: K-steps of LDS-DMA in flight
WIDTH = 16                 # K is a multiple of one 16-byte chunk of codes

_QUANT = (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p])
_SIGNATURES = {
    "mbnb_fp8blk_abi_version": (c_int, []),
    "mbnb_fp8blk_last_error": (c_char_p, []),
    "mbnb_fp8blk_last_launch": (c_char_p, []),
    "mbnb_fp8blk_quantize_groups": _QUANT,
    "mbnb_fp8blk_quantize_blocks": _QUANT,
    "mbnb_fp8blk_matmul": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p]),
    "mbnb_fp8blk_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_fp8blk_linear": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p, c_int64, c_void_p]),
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
    return lib().mbnb_fp8blk_last_launch().decode()


def blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def workspace_bytes(M: int, K: int) -> int:
    n = int(lib().mbnb_fp8blk_workspace_bytes(M, K))
    if n < 0:
        check(n, "workspace_bytes")
    return n
