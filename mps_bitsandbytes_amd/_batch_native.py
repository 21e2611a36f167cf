"""
ctypes binding of the grouped 4-bit decode launches for 2 to 16 activation rows (include/mbnb_batch.h, libmbnb_batch.so).

A separate library from the other seven, with the same rule: there is NO Python/CPU fallback behind it.  If the library is
missing or a call fails, the caller gets a RuntimeError.  MBNB_BATCH_NOT_APPLICABLE is not a failure: the library, which
alone knows the conditions of the fused launches, declined before launching anything, and the caller runs those members
through matmul_4bit (HIP kernels as well), or through the composed form where they carry adapters.
"""
from __future__ import annotations

import os
from ctypes import POINTER, c_char_p, c_int, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._group_native import MAX_MEMBERS, MEMBER_DTYPE, Member
from ._lora_native import ADAPTER_DTYPE, NO_ADAPTER, Adapter  # noqa: F401  (NO_ADAPTER: for the callers' tables)
from ._native import DTYPE_CODE, QUANT_CODE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_batch.so")

ABI_VERSION = 1            # include/mbnb_batch.h MBNB_BATCH_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_batch", "mps_bitsandbytes_amd.batch"
NOT_APPLICABLE = 65536     # MBNB_BATCH_NOT_APPLICABLE
MIN_M, MAX_M = 2, 16       # MBNB_BATCH_MIN_M / MBNB_BATCH_MAX_M: the rows for which functional asks this library at all

_SIGNATURES = {
    "mbnb_batch_abi_version": (c_int, []),
    "mbnb_batch_last_error": (c_char_p, []),
    "mbnb_batch_last_launch": (c_char_p, []),
    "mbnb_batch_gemm4": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, POINTER(Member), c_int, c_int, c_void_p]),
    "mbnb_batch_gemm4_lora": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, POINTER(Member), POINTER(Adapter), c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per call that launched since the last reset_launch_log(): (members in the call, M, K, dtype) for mbnb_batch_gemm4,
# (members in the call, the sum of their R, M, K, dtype) for mbnb_batch_gemm4_lora
launch_log: List[Tuple] = []


def reset_launch_log() -> None:
    launch_log.clear()


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
    """The form of this thread's last fused call ("skinny_group G3 M8", or
    "lora_down_rows G3 R48 M8 ku2/KU2 + skinny_group_lora G3 M8"; "" before the first)."""
    return lib().mbnb_batch_last_launch().decode()


def last_error() -> str:
    return lib().mbnb_batch_last_error().decode(errors="replace")


def gemm4(x: int, M: int, K: int, quant_type: str, dtype: torch.dtype, blocksize: int, members: Sequence[tuple], stream: c_void_p) -> List[bool]:
    """out_g[M, N_g] = x[M, K] . dequant(W_g)^T + bias_g for `members` (any number of Member field tuples; plain values, `x` an
    address): one mbnb_batch_gemm4 call, and so one kernel launch, per MAX_MEMBERS of them.  Returns one flag per call: True =
    launched, False = the library answered NOT_APPLICABLE for that chunk and wrote nothing (its reason: last_error())."""
    return _loader.call_chunks(globals(), "mbnb_batch_gemm4", "gemm4", (x, M, K, QUANT_CODE[quant_type], DTYPE_CODE[dtype], blocksize),
                               [(members, MEMBER_DTYPE, Member)], (), stream, (M, K, dtype))


def gemm4_lora(x: int, M: int, K: int, quant_type: str, dtype: torch.dtype, blocksize: int, members: Sequence[tuple],
               adapters: Sequence[tuple], stream: c_void_p) -> List[bool]:
    """gemm4 with the members' `adapters` (Adapter field tuples whose t is an f32 [M, R] workspace; NO_ADAPTER for a member without
    one): one mbnb_batch_gemm4_lora call, and so two kernel launches, per MAX_MEMBERS of them.  One flag per call, as gemm4."""
    if len(members) != len(adapters):
        raise ValueError(f"{len(members)} members but {len(adapters)} adapters")
    return _loader.call_chunks(globals(), "mbnb_batch_gemm4_lora", "gemm4_lora", (x, M, K, QUANT_CODE[quant_type], DTYPE_CODE[dtype], blocksize),
                               [(members, MEMBER_DTYPE, Member), (adapters, ADAPTER_DTYPE, Adapter)], (), stream, (M, K, dtype))
