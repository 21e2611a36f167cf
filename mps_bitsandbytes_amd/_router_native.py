"""
ctypes binding of the mixture-of-experts router (include/mbnb_router.h, libmbnb_router.so).

A separate library from the other twelve, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader
from ._native import BF16, DTYPE_CODE, F16, F32     # one definition; read from this module too

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_router.so")

ABI_VERSION = 1            # include/mbnb_router.h MBNB_ROUTER_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_router", "mps_bitsandbytes_amd.router"
ERR_ARG, ERR_SHAPE = -1, -2
MAX_EXPERTS = 1024         # MBNB_ROUTER_MAX_EXPERTS: an f32 logit per expert in LDS (libmbnb_moemlp.so's limit)
MAX_TOPK = 32              # MBNB_ROUTER_MAX_TOPK: slot a of a token is lane a of the selecting wave
MAX_K = 16384              # MBNB_ROUTER_MAX_K: one activation row in LDS, 32 KiB at this width
CHUNK = 8                  # elements per 16-byte chunk: K is a multiple of it

_SIGNATURES = {
    "mbnb_router_abi_version": (c_int, []),
    "mbnb_router_last_error": (c_char_p, []),
    "mbnb_router_last_launch": (c_char_p, []),
    "mbnb_router_topk_softmax": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p,
                                         c_void_p, c_int, c_void_p, c_void_p]),
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
    return lib().mbnb_router_last_launch().decode()
