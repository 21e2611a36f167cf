"""
ctypes binding of the trainable-weight library (include/mbnb_train.h, libmbnb_train.so): SwitchBackLinear's int8 forward and the
weight gradient dW = dY^T . X.

A separate library from libmbnb_hip.so (which it links against for mbnb_gemm_dense), with the same rule: there is NO Python/CPU
fallback behind it.  If the library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader, _native

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_train.so")

ABI_VERSION = 1            # include/mbnb_train.h MBNB_TRAIN_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_train", "mps_bitsandbytes_amd"
_REQUIRES = (_native,)     # libmbnb_hip.so first: the dependency this library resolves next to itself
PASS_ONLY = 1              # MBNB_TRAIN_PASS_ONLY: the first pass alone
FORCE_GENERIC = 2          # MBNB_TRAIN_FORCE_GENERIC: the generic kernel where the dense route would apply

_SIGNATURES = {
    "mbnb_train_abi_version": (c_int, []),
    "mbnb_train_last_error": (c_char_p, []),
    "mbnb_train_last_kernel": (c_char_p, []),
    "mbnb_train_padded_rows": (c_int64, [c_int64]),
    "mbnb_switchback_forward_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "mbnb_switchback_forward": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_int64, c_int, c_void_p]),
    "mbnb_linear_grad_weight_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "mbnb_linear_grad_weight": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int,
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


def last_kernel() -> str:
    """The kernel route the last call on this thread took (mbnb_train_last_kernel)."""
    return lib().mbnb_train_last_kernel().decode()


_last_kernel_addr = None


def last_variant() -> str:
    """The variant of the last call ("dq8x4 bias8", "dy1 x8"; "" where the launcher sets none): the second string of
    mbnb_train_last_kernel()'s buffer, right behind the name's terminating NUL (include/mbnb_train.h)."""
    global _last_kernel_addr
    if _last_kernel_addr is None:
        _last_kernel_addr = ctypes.CFUNCTYPE(c_void_p)(("mbnb_train_last_kernel", lib()))    # the same export, its pointer kept as an address
    addr = _last_kernel_addr()
    return ctypes.string_at(addr + len(ctypes.string_at(addr)) + 1).decode()


def padded_rows(M: int) -> int:
    """Mp of the weight gradient's transposed operands: M rounded up to a multiple of 64, at least 128."""
    return int(lib().mbnb_train_padded_rows(M))
