"""
ctypes binding of the grouped M = 1 decode GEMV with un-merged LoRA adapters (include/mbnb_lora.h, libmbnb_lora.so).

A separate library from the other six, with the same rule: there is NO Python/CPU fallback behind it.  If the library is
missing or a call fails, the caller gets a RuntimeError.  MBNB_LORA_NOT_APPLICABLE is not a failure: the library, which
alone knows the conditions of the fused launches, declined before launching anything, and the caller runs those members
through the composed form (matmul_4bit's HIP kernels plus the adapter in torch ops).
"""
from __future__ import annotations

import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _loader
from ._group_native import MAX_MEMBERS, MEMBER_DTYPE, Member
from ._native import DTYPE_CODE, QUANT_CODE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbnb_lora.so")

ABI_VERSION = 1            # include/mbnb_lora.h MBNB_LORA_ABI_VERSION
_PREFIX, _CHECK_PREFIX = "mbnb_lora", "mps_bitsandbytes_amd.lora"
NOT_APPLICABLE = 65536     # MBNB_LORA_NOT_APPLICABLE
MAX_R = 256                # MBNB_LORA_MAX_R (the library's condition; nothing here tests it)

# struct mbnb_lora_adapter as a numpy record: a whole table is built in one np.array call
ADAPTER_DTYPE = np.dtype([("a", "<u8"), ("b", "<u8"), ("t", "<u8"), ("R", "<i4"), ("scaling", "<f4")])
NO_ADAPTER = (0, 0, 0, 0, 0.0)


class Adapter(Structure):
    """mirror of ``struct mbnb_lora_adapter``"""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("t", c_void_p), ("R", c_int32), ("scaling", c_float)]


_SIGNATURES = {
    "mbnb_lora_abi_version": (c_int, []),
    "mbnb_lora_last_error": (c_char_p, []),
    "mbnb_lora_last_launch": (c_char_p, []),
    "mbnb_lora_gemv4": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, POINTER(Member), POINTER(Adapter), c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_load_error: Optional[str] = None

# one entry per mbnb_lora_gemv4 call that launched since the last reset_launch_log(): (members in the call, the sum of their R, K, dtype)
launch_log: List[Tuple[int, int, int, torch.dtype]] = []


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
    """The form of this thread's last fused call ("lora_down G3 R48 ku2/KU2 + gemv_lora G3 ku2/KU2"; "" before the first)."""
    return lib().mbnb_lora_last_launch().decode()


def last_error() -> str:
    return lib().mbnb_lora_last_error().decode(errors="replace")


def gemv4(x: int, K: int, quant_type: str, dtype: torch.dtype, blocksize: int, members: Sequence[tuple], adapters: Sequence[tuple],
          stream: c_void_p) -> List[bool]:
    """out_g = x . dequant(W_g)^T + bias_g + scaling_g B_g . (A_g . x) for `members` (Member field tuples) and their `adapters` (Adapter
    field tuples, NO_ADAPTER for a member without one; plain values, `x` an address): one mbnb_lora_gemv4 call, and so two kernel
    launches, per MAX_MEMBERS of them.  Returns one flag per call: True = launched, False = the library answered NOT_APPLICABLE for that
    chunk and wrote nothing (its reason: last_error())."""
    if len(members) != len(adapters):
        raise ValueError(f"{len(members)} members but {len(adapters)} adapters")
    return _loader.call_chunks(globals(), "mbnb_lora_gemv4", "gemv4", (x, K, QUANT_CODE[quant_type], DTYPE_CODE[dtype], blocksize),
                               [(members, MEMBER_DTYPE, Member), (adapters, ADAPTER_DTYPE, Adapter)], (), stream, (K, dtype))
