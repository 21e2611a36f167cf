"""
ctypes binding of the LLM.int8-decomposition library (include/mbnb_sparse.h, libmbnb_sparse.so): INT8 with column + row statistics and
the COO sparse operations.

A separate library from libmbnb_hip.so (which it links against for mbnb_gemm_dense), with the same rule: there is NO Python/CPU
fallback behind it.  If the library is missing or a call fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p
from typing import Optional

from . import _loader, _native

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_sparse.so")

ABI_VERSION = 1            # include/mbnb_sparse.h MBNB_SPARSE_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_sparse", "mps_bitsandbytes_amd"
_REQUIRES = (_native,)     # libmbnb_hip.so first: the dependency this library resolves next to itself
PASS_ONLY = 1              # MBNB_SPARSE_PASS_ONLY: matmul_colrow's dequantising pass alone
FORCE_GENERIC = 2          # MBNB_SPARSE_FORCE_GENERIC: the generic matmul kernel / the device-built CSR form
COO_VALUES, COO_INT8_SCALAR, COO_INT8_ENTRY = 0, 1, 2     # value_kind of mbnb_spmm_coo

_SIGNATURES = {
    "mbnb_sparse_abi_version": (c_int, []),
    "mbnb_sparse_last_error": (c_char_p, []),
    "mbnb_sparse_last_kernel": (c_char_p, []),
    "mbnb_colrow_quantize_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_colrow_quantize": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mbnb_colrow_dequantize": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "mbnb_colrow_matmul_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "mbnb_colrow_matmul": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_int, c_void_p]),
    "mbnb_coo_count": (c_int, [c_void_p, c_int, c_int64, c_int64, c_float, c_void_p, c_void_p]),
    "mbnb_coo_fill": (c_int, [c_void_p, c_int, c_int64, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mbnb_coo_quantize_workspace_bytes": (c_int64, []),
    "mbnb_coo_quantize": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mbnb_spmm_coo_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "mbnb_spmm_coo": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64,
                              c_void_p, c_void_p, c_int64, c_int, c_void_p]),
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
    """The kernel route the last call on this thread took (mbnb_sparse_last_kernel)."""
    return lib().mbnb_sparse_last_kernel().decode()


_last_kernel_addr = None


def last_variant() -> str:
    """The variant of the last call ("wt", "parts1024", "G16 x2"; "" where the launcher sets none): the second string of
    mbnb_sparse_last_kernel()'s buffer, right behind the name's terminating NUL (include/mbnb_sparse.h)."""
    global _last_kernel_addr
    if _last_kernel_addr is None:
        _last_kernel_addr = ctypes.CFUNCTYPE(c_void_p)(("mbnb_sparse_last_kernel", lib()))    # the same export, its pointer kept as an address
    addr = _last_kernel_addr()
    return ctypes.string_at(addr + len(ctypes.string_at(addr)) + 1).decode()
