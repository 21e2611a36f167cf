"""
ctypes binding of the grouped M = 1 decode GEMV (include/mbnb_group.h, libmbnb_group.so).

A separate library from the other five, with the same rule: there is NO Python/CPU fallback behind it.  If the
library is missing or a call fails, the caller gets a RuntimeError.  MBNB_GROUP_NOT_APPLICABLE is not a failure:
the library, which alone knows the conditions of the fused launch, declined before launching anything, and the
caller runs those members one by one through matmul_4bit (HIP kernels as well).
"""
from __future__ import annotations

import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._native import DTYPE_CODE, QUANT_CODE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_group.so")

ABI_VERSION = 1            # include/mbnb_group.h MBNB_GROUP_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_group", "mps_bitsandbytes_amd.group"
MAX_MEMBERS = 16           # MBNB_GROUP_MAX_MEMBERS: members per call (one kernel launch)
NOT_APPLICABLE = 65536     # MBNB_GROUP_NOT_APPLICABLE

# struct mbnb_group_member as a numpy record: a whole table is built in one np.array call
MEMBER_DTYPE = np.dtype([("packed", "<u8"), ("absmax_f32", "<u8"), ("absmax_i8", "<u8"), ("absmax2", "<u8"), ("bias", "<u8"),
                         ("out", "<u8"), ("N", "<i8"), ("blocksize2", "<i4"), ("pad_", "<i4")])


class Member(Structure):
    """mirror of ``struct mbnb_group_member``"""
    _fields_ = [("packed", c_void_p), ("absmax_f32", c_void_p), ("absmax_i8", c_void_p), ("absmax2", c_void_p), ("bias", c_void_p),
                ("out", c_void_p), ("N", c_int64), ("blocksize2", c_int32), ("pad_", c_int32)]


_SIGNATURES = {
    "mbnb_group_abi_version": (c_int, []),
    "mbnb_group_last_error": (c_char_p, []),
    "mbnb_group_last_launch": (c_char_p, []),
    "mbnb_group_gemv4": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, POINTER(Member), c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per mbnb_group_gemv4 call that launched since the last reset_launch_log(): (members in the call, K, dtype)
launch_log: List[Tuple[int, int, torch.dtype]] = []


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
    """The form of this thread's last fused launch ("gemv_group G3 ku2/KU2"; "" before the first)."""
    return lib().mbnb_group_last_launch().decode()


def last_error() -> str:
    return lib().mbnb_group_last_error().decode(errors="replace")


def gemv4(x: int, K: int, quant_type: str, dtype: torch.dtype, blocksize: int, members: Sequence[tuple], stream: c_void_p) -> List[bool]:
    """out_g = x . dequant(W_g)^T + bias_g for `members` (any number of Member field tuples; plain values, `x` an address): one
    mbnb_group_gemv4 call, and so one kernel launch, per MAX_MEMBERS of them.  Returns one flag per call: True = launched,
    False = the library answered NOT_APPLICABLE for that chunk and wrote nothing (its reason: last_error())."""
    return _loader.call_chunks(globals(), "mbnb_group_gemv4", "gemv4", (x, K, QUANT_CODE[quant_type], DTYPE_CODE[dtype], blocksize),
                               [(members, MEMBER_DTYPE, Member)], (), stream, (K, dtype))
