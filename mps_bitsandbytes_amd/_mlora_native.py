"""
ctypes binding of the grouped 4-bit decode launches for 2 to 16 activation rows with a different un-merged LoRA adapter per row
(include/mbnb_mlora.h, libmbnb_mlora.so).

A separate library from the other eight, with the same rule: there is NO Python/CPU fallback behind it.  If the library is
missing or a call fails, the caller gets a RuntimeError.  MBNB_MLORA_NOT_APPLICABLE is not a failure: the library, which
alone knows the conditions of the fused launches, declined before launching anything, and the caller runs those members
through the composed form (matmul_4bit's HIP kernels plus the adapters in torch ops).
"""
from __future__ import annotations

import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._group_native import MAX_MEMBERS, MEMBER_DTYPE, Member
from ._native import DTYPE_CODE, QUANT_CODE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_mlora.so")

ABI_VERSION = 1            # include/mbnb_mlora.h MBNB_MLORA_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_mlora", "mps_bitsandbytes_amd.mlora"
NOT_APPLICABLE = 65536     # MBNB_MLORA_NOT_APPLICABLE
MIN_M, MAX_M = 2, 16       # MBNB_MLORA_MIN_M / MBNB_MLORA_MAX_M: the rows for which functional asks this library at all
MAX_R = 64                 # MBNB_MLORA_MAX_R (the library's condition; functional asks it before it allocates)

# struct mbnb_mlora_bank as a numpy record: a whole table is built in one np.array call
BANK_DTYPE = np.dtype([("a", "<u8"), ("b", "<u8"), ("scaling", "<u8"), ("t", "<u8"), ("R", "<i4"), ("S", "<i4")])
NO_BANK = (0, 0, 0, 0, 0, 0)


class Bank(Structure):
    """mirror of ``struct mbnb_mlora_bank``"""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("scaling", c_void_p), ("t", c_void_p), ("R", c_int32), ("S", c_int32)]


_SIGNATURES = {
    "mbnb_mlora_abi_version": (c_int, []),
    "mbnb_mlora_last_error": (c_char_p, []),
    "mbnb_mlora_last_launch": (c_char_p, []),
    "mbnb_mlora_gemm4": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, POINTER(Member), POINTER(Bank), c_void_p, c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per mbnb_mlora_gemm4 call that launched since the last reset_launch_log(): (members in the call, the sum of their R, M, K, dtype)
launch_log: List[Tuple[int, int, int, int, torch.dtype]] = []


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
    """The form of this thread's last fused call ("lora_down_sel G3 R48 M8 ku2/KU2 + skinny_mlora G3 M8"; "" before the first)."""
    return lib().mbnb_mlora_last_launch().decode()


def last_error() -> str:
    return lib().mbnb_mlora_last_error().decode(errors="replace")


def gemm4(x: int, M: int, K: int, quant_type: str, dtype: torch.dtype, blocksize: int, members: Sequence[tuple], banks: Sequence[tuple],
          ids: int, stream: c_void_p) -> List[bool]:
    """out_g[m] = x[m] . dequant(W_g)^T + bias_g + scaling_g[s] B_{g,s} . (A_{g,s} . x[m]), s = ids[m], for `members` (Member field
    tuples) and their `banks` (Bank field tuples whose t is an f32 [M, R] workspace; NO_BANK for a member without one; plain values, `x`
    and `ids` device addresses -- the ids are never read here): one mbnb_mlora_gemm4 call, and so two kernel launches, per MAX_MEMBERS
    of them.  Returns one flag per call: True = launched, False = the library answered NOT_APPLICABLE for that chunk and wrote nothing
    (its reason: last_error())."""
    if len(members) != len(banks):
        raise ValueError(f"{len(members)} members but {len(banks)} banks")
    return _loader.call_chunks(globals(), "mbnb_mlora_gemm4", "gemm4", (x, M, K, QUANT_CODE[quant_type], DTYPE_CODE[dtype], blocksize),
                               [(members, MEMBER_DTYPE, Member), (banks, BANK_DTYPE, Bank)], (ids,), stream, (M, K, dtype))
