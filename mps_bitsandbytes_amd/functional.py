"""
Functional API of the MI355X quantized-linear backend.

Mirrors the reference's ``mps_bitsandbytes/functional.py`` for the quantized-linear hot path
(same names, argument order, defaults, return types and validation messages) so that user code
and tests written against the reference read the same here.  Every operation runs as a
hand-written HIP kernel on gfx950 through the C ABI in ``include/mbnb_hip.h``; tensors must
live on a ``cuda`` (ROCm) device.  There is no CPU / pure-torch fallback: a missing native
library or a non-GPU tensor raises.

Host-side work done here is plumbing only: argument validation, shape arithmetic, output
allocation, dtype casts of activations/bias (reference: functional.py:764-766), stream lookup.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _batch_native, _group_native, _lora_native, _mlora_native, _moe_native, _moegemm_native, _moemlp_native, _mx_native, _native, _router_native, _sparse_native, _train_native
from ._native import AbsmaxDesc, check, dtype_code, ptr, stream_ptr, on_device

# ============================================================================= codebooks
# reference: functional.py:21-32
NF4_CODEBOOK = torch.tensor([
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
    -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
    0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
    0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0
], dtype=torch.float32)

FP4_CODEBOOK = torch.tensor([
    0.0, 0.0625, 0.125, 0.25, 0.375, 0.5, 0.75, 1.0,
    -0.0, -0.0625, -0.125, -0.25, -0.375, -0.5, -0.75, -1.0
], dtype=torch.float32)


def create_normal_map(offset=0.9677083, use_extra_value=True):
    """NF4 codebook (bitsandbytes compatibility; reference functional.py:35-37)."""
    return NF4_CODEBOOK.clone()


def create_fp4_map(signed=True):
    """FP4 codebook (bitsandbytes compatibility; reference functional.py:40-42)."""
    return FP4_CODEBOOK.clone()


def _check_device(tensor: Tensor, operation: str = "operation"):
    """Device gate.  The reference accepts 'mps'/'cpu' (functional.py:76-83); this backend runs
    on ROCm GPUs only ('cuda' device type) and has no CPU path."""
    device_type = tensor.device.type
    if device_type != 'cuda':
        raise ValueError(
            f"mps-bitsandbytes-amd {operation} requires tensor on a 'cuda' (ROCm/HIP) device, "
            f"got '{device_type}'. Move tensor with .to('cuda')"
        )


_warned: set = set()


# matmul_4bit from 256 rows and 1.5 M outputs up: let the library dequantise the weight ONCE into a transient N x K scratch (in the weight dtype)
# and run a dense MFMA GEMM -- what the reference does for M > 512 (functional.py:753-767) -- instead of the fused kernels,
# which decode each weight tile once per 256 rows.  False keeps the fused kernels at every M (no N x K scratch) in matmul_4bit,
# linear_int8 and matmul_fp8_e4m3 alike (the FUSED_ONLY flag travels to all three entry points).  The scratch is transient:
# N x K_weight x 2 bytes per call from torch's caching allocator (32 MB for a 4096^2 layer, ~1 GB for a 128k x 4096 head).
DECODE_ONCE = True
MATMUL_FUSED_ONLY = 1   # include/mbnb_hip.h MBNB_MATMUL_FUSED_ONLY: the flags word of mbnb_matmul_4bit / mbnb_linear_int8 / mbnb_linear_fp8


def _as(t: Tensor, dtype: torch.dtype, device=None) -> Tensor:
    """`t.to(device, dtype).contiguous()` that dispatches nothing when `t` already is what is asked for"""
    if t.dtype != dtype or (device is not None and t.device != device):
        t = t.to(device=device if device is not None else t.device, dtype=dtype)
    return t if t.is_contiguous() else t.contiguous()


def _warn_once(key: str, message: str) -> None:
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(message, RuntimeWarning, stacklevel=3)


def _padded(n: int, blocksize: int) -> int:
    """K_padded rule, reference functional.py:219-221 / :260-262."""
    p = ((n + blocksize - 1) // blocksize) * blocksize
    if p % 2 != 0:
        p += blocksize
    return p


# ============================================================================= QuantState
@dataclass
class QuantState:
    """
    Quantization state for dequantization (reference: functional.py:90-156; field-for-field
    identical, including ``as_dict`` keys — this is the checkpoint wire format).
    """
    absmax: Tensor
    shape: torch.Size
    code: Optional[Tensor] = None
    blocksize: int = 64
    quant_type: str = "nf4"
    dtype: torch.dtype = torch.float16
    offset: Optional[Tensor] = None
    state2: Optional['QuantState'] = None

    def __post_init__(self):
        if self.code is None:
            self.code = NF4_CODEBOOK if self.quant_type == "nf4" else FP4_CODEBOOK

    def to(self, device):
        """Move state to device (in place, recursive)."""
        self.absmax = self.absmax.to(device)
        if self.code is not None:
            self.code = self.code.to(device)
        if self.offset is not None:
            self.offset = self.offset.to(device)
        if self.state2 is not None:
            self.state2 = self.state2.to(device)
        return self

    def as_dict(self, packed=False):
        return {
            'absmax': self.absmax,
            'shape': self.shape,
            'blocksize': self.blocksize,
            'quant_type': self.quant_type,
            'dtype': self.dtype,
            'state2': self.state2.as_dict() if self.state2 else None,
        }

    @classmethod
    def from_dict(cls, state_dict, device='cpu'):
        state2 = None
        if state_dict.get('state2') is not None:
            state2 = cls.from_dict(state_dict['state2'], device)
        return cls(
            absmax=state_dict['absmax'].to(device),
            shape=state_dict['shape'],
            blocksize=state_dict.get('blocksize', 64),
            quant_type=state_dict.get('quant_type', 'nf4'),
            dtype=state_dict.get('dtype', torch.float16),
            state2=state2,
        )


def _absmax_desc(absmax: Tensor, state2: Optional[QuantState], keep: list) -> AbsmaxDesc:
    """Build the C descriptor of an absmax tensor.  One level of int8 double-quant
    (QuantState.state2 as produced by quantize_4bit, functional.py:288-292) is decoded inside the
    consuming kernel; anything else is first brought to plain f32 by dequantize_blockwise.
    `keep` collects tensors that must stay alive until the launch has been enqueued."""
    if absmax.device.type != 'cuda':
        raise ValueError(f"absmax must live on a 'cuda' (ROCm/HIP) device before a kernel launch, got '{absmax.device}'")
    if state2 is not None:
        if (absmax.dtype == torch.int8 and state2.state2 is None and state2.dtype == torch.float32
                and state2.absmax.dtype == torch.float32):
            bs2 = int(state2.blocksize)
            q = absmax if absmax.is_contiguous() else absmax.contiguous()
            # the second-level absmax follows the first level's device (a QuantState built by from_dict() defaults to
            # 'cpu'; handing the kernel a host pointer would be a GPU fault where the reference raises a device mismatch)
            a2 = state2.absmax
            if a2.device != absmax.device:
                a2 = a2.to(device=absmax.device)
            if not a2.is_contiguous():
                a2 = a2.contiguous()
            need2 = (q.numel() + bs2 - 1) // bs2 if bs2 > 0 else -1
            if bs2 <= 0 or a2.numel() < need2:
                raise ValueError(f"state2.absmax has {a2.numel()} elements, expected {need2} "
                                 f"({q.numel()} absmax codes in blocks of {bs2})")
            keep += [q, a2]
            return AbsmaxDesc(None, q.data_ptr(), a2.data_ptr(), bs2)
        state2 = _state_on(state2, absmax.device)
        absmax = dequantize_blockwise(absmax, state2)
    a = absmax
    if a.dtype != torch.float32:
        a = a.to(torch.float32)
    if not a.is_contiguous():
        a = a.contiguous()
    keep.append(a)
    return AbsmaxDesc(a.data_ptr(), None, None, 0)


def _state_on(state: QuantState, device) -> QuantState:
    """A copy of `state` (recursively) whose tensors live on `device`; the caller's object is left untouched."""
    if state.absmax.device == device and (state.state2 is None or state.state2.absmax.device == device):
        return state
    return QuantState(absmax=state.absmax.to(device), shape=state.shape, code=state.code, blocksize=state.blocksize,
                      quant_type=state.quant_type, dtype=state.dtype, offset=state.offset,
                      state2=None if state.state2 is None else _state_on(state.state2, device))


def _check_absmax_count(absmax: Tensor, rows: int, cols_padded: int, blocksize: int, what: str) -> None:
    """The kernels index absmax as [rows, cols_padded / blocksize] and receive no length: a checkpoint whose blocksize or
    shape disagrees with its absmax must fail here (the reference's absmax.view(N, num_blocks_per_row) raises,
    functional.py:371-373), not read past the allocation."""
    need = rows * (cols_padded // blocksize)
    if absmax.numel() != need:
        raise ValueError(f"{what}: absmax has {absmax.numel()} elements, expected {need} "
                         f"({rows} rows x {cols_padded // blocksize} blocks of {blocksize})")


# ============================================================================= 4-bit
def quantize_4bit(
    A: Tensor,
    absmax: Optional[Tensor] = None,
    out: Optional[Tensor] = None,
    blocksize: int = 64,
    compress_statistics: bool = False,
    quant_type: str = "nf4",
    quant_storage: torch.dtype = torch.uint8,
) -> Tuple[Tensor, QuantState]:
    """
    Quantize tensor to 4-bit NF4 or FP4 (reference: functional.py:163-303, bit-exact).

    2-D tensors [N, K] are quantized row-wise (each row padded to a multiple of `blocksize`);
    other shapes over the flattened tensor.  Returns (packed uint8 flat tensor, QuantState).
    """
    if quant_type not in ("nf4", "fp4"):
        raise ValueError(f"quant_type must be 'nf4' or 'fp4', got {quant_type}")
    _check_device(A, "quantize_4bit")
    if blocksize <= 0:
        raise ValueError(f"blocksize must be positive, got {blocksize}")
    if blocksize > 65536:
        raise ValueError(f"blocksize too large ({blocksize}), max is 65536")
    if (blocksize & (blocksize - 1)) != 0:
        raise ValueError(f"blocksize must be a power of 2, got {blocksize}")
    max_safe_numel = 2**31 - 1
    if A.numel() > max_safe_numel:
        raise ValueError(f"Tensor too large ({A.numel()} elements), max is {max_safe_numel}")

    orig_shape = A.shape
    orig_dtype = A.dtype
    code = dtype_code(orig_dtype, "quantize_4bit")
    A = A.contiguous()
    if A.dim() == 2:
        rows, cols = A.shape
    else:
        rows, cols = 1, A.numel()
    cols_padded = _padded(cols, blocksize)
    nbytes = rows * cols_padded // 2
    nblocks = rows * cols_padded // blocksize

    user_out = out
    # the kernels store whole dwords: a caller's buffer off a 4-byte boundary (a contiguous view at an odd storage offset) is
    # filled by the copy below, as any other `out` that cannot be written directly
    if (out is not None and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == nbytes
            and out.device == A.device and out.data_ptr() % 4 == 0):
        packed = out.view(-1)
    else:
        packed = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    if blocksize == 1:
        packed.zero_()
    absmax_in = None
    if absmax is not None:
        absmax_in = absmax.to(device=A.device, dtype=torch.float32).contiguous().view(-1)
        if absmax_in.numel() != nblocks:
            raise ValueError(f"absmax has {absmax_in.numel()} elements, expected {nblocks}")
    # compress_statistics: the 256-block int8 quantisation of absmax (functional.py:288-292) is fused into the same launch
    # when the library supports the blocksize; the f32 absmax then never exists in memory
    fused_dq = compress_statistics and absmax_in is None and 8 <= blocksize <= 512 and nblocks > 0
    absmax_t = None
    state2 = None
    with on_device(A.device):
        if fused_dq:
            codes = torch.empty(nblocks, dtype=torch.int8, device=A.device)
            absmax2 = torch.empty((nblocks + 255) // 256, dtype=torch.float32, device=A.device)
            check(_native.lib().mbnb_quantize_4bit_dq(
                ptr(A), code, rows, cols, cols_padded, int(blocksize), _native.QUANT_CODE[quant_type], ptr(packed),
                ptr(codes), ptr(absmax2), stream_ptr(A.device)), "quantize_4bit")
            absmax_t = codes
            state2 = QuantState(absmax=absmax2, shape=torch.Size([nblocks]), blocksize=256, quant_type="int8",
                                dtype=torch.float32)     # = what quantize_blockwise(absmax, blocksize=256) returns
        else:
            absmax_out = torch.empty(nblocks, dtype=torch.float32, device=A.device)
            check(_native.lib().mbnb_quantize_4bit(
                ptr(A), code, rows, cols, cols_padded, int(blocksize), _native.QUANT_CODE[quant_type],
                ptr(absmax_in), ptr(packed), ptr(absmax_out), stream_ptr(A.device)), "quantize_4bit")
            absmax_t = absmax_out

    if user_out is not None and packed.data_ptr() != user_out.data_ptr():
        user_out.view(-1)[:] = packed.to(user_out.dtype)  # reference: out[:] = ... (functional.py:251)
        packed = user_out.flatten()
    elif quant_storage != torch.uint8:
        packed = packed.to(quant_storage)

    if compress_statistics and not fused_dq:
        absmax_t, state2 = quantize_blockwise(absmax_t, blocksize=256)

    quant_state = QuantState(
        absmax=absmax_t,
        shape=orig_shape,
        blocksize=blocksize,
        quant_type=quant_type,
        dtype=orig_dtype,
        state2=state2,
    )
    return packed, quant_state


def dequantize_4bit(
    A: Tensor,
    quant_state: Optional[QuantState] = None,
    absmax: Optional[Tensor] = None,
    out: Optional[Tensor] = None,
    blocksize: int = 64,
    quant_type: str = "nf4",
) -> Tensor:
    """Dequantize a 4-bit tensor (reference: functional.py:306-416, bit-exact)."""
    _check_device(A, "dequantize_4bit")
    state2 = None
    if quant_state is not None:
        absmax = quant_state.absmax
        blocksize = quant_state.blocksize
        quant_type = quant_state.quant_type
        shape = quant_state.shape
        dtype = quant_state.dtype
        state2 = quant_state.state2
    else:
        if absmax is None:
            raise ValueError("Either quant_state or absmax must be provided")
        shape = None
        dtype = torch.float16
    if quant_type not in ("nf4", "fp4"):
        raise ValueError(f"quant_type must be 'nf4' or 'fp4', got {quant_type}")

    A = A.contiguous()
    if A.dtype != torch.uint8:
        A = A.to(torch.uint8)
    if A.data_ptr() % 4 != 0:
        A = A.clone()       # the kernels read whole dwords: a contiguous view at an odd storage offset is copied to a fresh allocation
    if shape is not None and len(shape) == 2:
        rows, cols = int(shape[0]), int(shape[1])
        cols_padded = _padded(cols, blocksize)
        out_shape = (rows, cols)
    else:
        # flat layout: the number of blocks is what absmax says (functional.py:399-401)
        rows = 1
        cols_padded = absmax.numel() * blocksize
        if shape is not None:
            cols = int(torch.Size(shape).numel())
            out_shape = tuple(shape)
        elif out is not None:
            cols = out.numel()
            out_shape = tuple(out.shape)
        else:
            cols = cols_padded
            out_shape = (cols,)
    if A.numel() * 2 < rows * cols_padded or cols > cols_padded:
        raise ValueError(
            f"packed tensor has {A.numel()} bytes but absmax/shape describe {rows * cols_padded} 4-bit values")
    _check_absmax_count(absmax, rows, cols_padded, blocksize, "dequantize_4bit")

    keep: list = []
    desc = _absmax_desc(absmax.to(A.device), state2, keep)
    direct = (out is not None and out.dtype == dtype and out.is_contiguous() and out.numel() == rows * cols
              and out.device == A.device)
    result = out if direct else torch.empty(out_shape, dtype=dtype, device=A.device)
    with on_device(A.device):
        check(_native.lib().mbnb_dequantize_4bit(
            ptr(A), ctypes.byref(desc), rows, cols, cols_padded, int(blocksize), _native.QUANT_CODE[quant_type],
            dtype_code(dtype, "dequantize_4bit"), ptr(result), stream_ptr(A.device)), "dequantize_4bit")
    if out is not None and not direct:
        out[:] = result.view(out.shape).to(out.dtype)
        return out
    return result


def quantize_nf4(A: Tensor, absmax: Optional[Tensor] = None, out: Optional[Tensor] = None, blocksize: int = 64,
                 compress_statistics: bool = False, quant_storage: torch.dtype = torch.uint8):
    """Alias for quantize_4bit with quant_type='nf4' (reference functional.py:419-428)."""
    return quantize_4bit(A, absmax, out, blocksize, compress_statistics, "nf4", quant_storage)


def dequantize_nf4(A: Tensor, quant_state: Optional[QuantState] = None, absmax: Optional[Tensor] = None,
                   out: Optional[Tensor] = None, blocksize: int = 64) -> Tensor:
    """Alias for dequantize_4bit with quant_type='nf4' (reference functional.py:431-439)."""
    return dequantize_4bit(A, quant_state, absmax, out, blocksize, "nf4")


def quantize_fp4(A: Tensor, absmax: Optional[Tensor] = None, out: Optional[Tensor] = None, blocksize: int = 64,
                 compress_statistics: bool = False, quant_storage: torch.dtype = torch.uint8):
    """Alias for quantize_4bit with quant_type='fp4' (reference functional.py:442-451)."""
    return quantize_4bit(A, absmax, out, blocksize, compress_statistics, "fp4", quant_storage)


def dequantize_fp4(A: Tensor, quant_state: Optional[QuantState] = None, absmax: Optional[Tensor] = None,
                   out: Optional[Tensor] = None, blocksize: int = 64) -> Tensor:
    """Alias for dequantize_4bit with quant_type='fp4' (reference functional.py:454-462)."""
    return dequantize_4bit(A, quant_state, absmax, out, blocksize, "fp4")


# ============================================================================= blockwise int8
def quantize_blockwise(
    A: Tensor,
    code: Optional[Tensor] = None,
    absmax: Optional[Tensor] = None,
    out: Optional[Tensor] = None,
    blocksize: int = 4096,
    nested: bool = False,
) -> Tuple[Tensor, QuantState]:
    """INT8 blockwise absmax quantization (reference: functional.py:469-539, bit-exact)."""
    _check_device(A, "quantize_blockwise")
    if blocksize <= 0:
        raise ValueError(f"blocksize must be positive, got {blocksize}")
    if blocksize > 65536:
        raise ValueError(f"blocksize too large ({blocksize}), max is 65536")
    orig_shape = A.shape
    orig_dtype = A.dtype
    dcode = dtype_code(orig_dtype, "quantize_blockwise")
    A = A.contiguous()
    numel = A.numel()
    nblocks = (numel + blocksize - 1) // blocksize
    absmax_in = None
    if absmax is not None:
        absmax_in = absmax.to(device=A.device, dtype=torch.float32).contiguous().view(-1)
    q = torch.empty(numel, dtype=torch.int8, device=A.device)
    absmax_out = torch.empty(nblocks, dtype=torch.float32, device=A.device)
    with on_device(A.device):
        check(_native.lib().mbnb_quantize_blockwise(
            ptr(A), dcode, numel, int(blocksize), ptr(absmax_in), ptr(q), ptr(absmax_out),
            stream_ptr(A.device)), "quantize_blockwise")
    if out is not None:
        out.view(-1)[:numel] = q  # reference writes the blocked result into `out` (functional.py:522)
    q = q.view(orig_shape)

    absmax_t = absmax_out
    state2 = None
    if nested:
        absmax_t, state2 = quantize_blockwise(absmax_out, blocksize=256)
    quant_state = QuantState(
        absmax=absmax_t,
        shape=orig_shape,
        blocksize=blocksize,
        quant_type="int8",
        dtype=orig_dtype,
        state2=state2,
    )
    return q, quant_state


def dequantize_blockwise(
    A: Tensor,
    quant_state: Optional[QuantState] = None,
    absmax: Optional[Tensor] = None,
    code: Optional[Tensor] = None,
    out: Optional[Tensor] = None,
    blocksize: int = 4096,
    nested: bool = False,
) -> Tensor:
    """Dequantize blockwise INT8 (reference: functional.py:542-600, bit-exact)."""
    _check_device(A, "dequantize_blockwise")
    if quant_state is not None:
        absmax = quant_state.absmax
        blocksize = quant_state.blocksize
        shape = quant_state.shape
        dtype = quant_state.dtype
        if quant_state.state2 is not None:
            absmax = dequantize_blockwise(absmax, quant_state.state2)
    else:
        if absmax is None:
            raise ValueError("Either quant_state or absmax must be provided")
        shape = A.shape
        dtype = torch.float16
    q = A.contiguous()
    if q.dtype != torch.int8:
        q = q.to(torch.int8)
    numel = q.numel()
    am = absmax.to(device=A.device, dtype=torch.float32).contiguous()
    result = torch.empty(numel, dtype=dtype, device=A.device)
    with on_device(A.device):
        check(_native.lib().mbnb_dequantize_blockwise(
            ptr(q), numel, ptr(am), int(blocksize), dtype_code(dtype, "dequantize_blockwise"), ptr(result),
            stream_ptr(A.device)), "dequantize_blockwise")
    result = result.view(shape)
    if out is not None:
        out[:] = result
        return out
    return result


# ============================================================================= rowwise int8
def quantize_rowwise(tensor: Tensor) -> Tuple[Tensor, Tensor]:
    """Row-wise absmax INT8 quantization (reference: functional.py:607-625, bit-exact).
    Returns (int8 tensor of the same shape, scales f32 [rows]); scales hold the absmax itself."""
    _check_device(tensor, "quantize_rowwise")
    orig_shape = tensor.shape
    t = tensor.contiguous()
    cols = t.shape[-1]
    rows = t.numel() // cols if cols else 0
    q = torch.empty(t.shape, dtype=torch.int8, device=t.device)
    scales = torch.empty(rows, dtype=torch.float32, device=t.device)
    with on_device(t.device):
        check(_native.lib().mbnb_quantize_rowwise(
            ptr(t), dtype_code(t.dtype, "quantize_rowwise"), rows, cols, ptr(q), ptr(scales),
            stream_ptr(t.device)), "quantize_rowwise")
    return q.view(orig_shape), scales


def dequantize_rowwise(quantized: Tensor, scales: Tensor, dtype: torch.dtype = torch.float16) -> Tensor:
    """Dequantize row-wise INT8 (reference: functional.py:628-636, bit-exact)."""
    _check_device(quantized, "dequantize_rowwise")
    orig_shape = quantized.shape
    q = quantized.contiguous()
    cols = q.shape[-1]
    rows = q.numel() // cols if cols else 0
    s = scales.to(device=q.device, dtype=torch.float32).contiguous().view(-1)
    if s.numel() != rows:
        raise ValueError(f"scales has {s.numel()} elements, expected {rows}")
    out = torch.empty(q.shape, dtype=dtype, device=q.device)
    with on_device(q.device):
        check(_native.lib().mbnb_dequantize_rowwise(
            ptr(q), ptr(s), rows, cols, dtype_code(dtype, "dequantize_rowwise"), ptr(out),
            stream_ptr(q.device)), "dequantize_rowwise")
    return out.view(orig_shape)


# ============================================================================= matmuls
def matmul_4bit(
    A: Tensor,
    B: Tensor,
    quant_state: QuantState,
    bias: Optional[Tensor] = None,
    compute_dtype: Optional[torch.dtype] = None,
) -> Tensor:
    """
    Matrix multiplication with 4-bit quantized weights: ``A[..., K] @ dequant(B)[N, K]^T + bias``.

    Signature of the reference (functional.py:680-773).  Below 256 rows (1.5 M outputs) ONE fused HIP kernel decodes the
    packed weight inside the GEMV / MFMA GEMM (the reference fuses only on MPS and only for M <= 512); from there up the
    library does the reference's own two steps (functional.py:753-767) on a transient scratch: ``dequantize_4bit`` once, then
    a dense MFMA GEMM (``DECODE_ONCE = False`` keeps the fused kernels at every M).  Either way the decoded weight is
    rounded to ``quant_state.dtype`` exactly as ``dequantize_4bit`` would, the contraction runs in that dtype with f32
    accumulation, and the result is cast to ``compute_dtype`` (default ``A.dtype``) -- the numerics of the reference's CPU
    branch (functional.py:756-773).
    """
    if (A.requires_grad or (bias is not None and bias.requires_grad)) and torch.is_grad_enabled():
        return _MatMul4bitGrad.apply(A, B, quant_state, bias, compute_dtype)   # its forward is this function with grad mode off
    if compute_dtype is None:
        compute_dtype = A.dtype
    _check_device(A, "matmul_4bit")
    _check_device(B, "matmul_4bit")
    if len(quant_state.shape) != 2:
        raise ValueError(f"matmul_4bit needs a 2-D quantized weight, got shape {tuple(quant_state.shape)}")
    N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
    if A.shape[-1] != K:
        raise RuntimeError(
            f"mat1 and mat2 shapes cannot be multiplied ({A.numel() // max(A.shape[-1], 1)}x{A.shape[-1]} and {K}x{N})")
    blocksize = quant_state.blocksize
    K_weight = _padded(K, blocksize)
    w_dtype = quant_state.dtype
    w_code = dtype_code(w_dtype, "matmul_4bit")

    orig_shape = A.shape
    # reference: A.to(weight.dtype), functional.py:764.  (No-op conversions are skipped by hand: at M = 1 the kernel takes 5 us and every
    # dispatched torch call costs ~1 us of host time, tools/host_overhead.py.)
    A2 = A if A.dim() == 2 else A.reshape(-1, K)
    if A2.dtype != w_dtype:
        A2 = A2.to(w_dtype)
    if not A2.is_contiguous():
        A2 = A2.contiguous()
    M = A2.shape[0]
    bias_w = None
    if bias is not None:
        bias_w = bias   # functional.py:765-766
        if bias_w.dtype != w_dtype or bias_w.device != A.device:
            bias_w = bias_w.to(device=A.device, dtype=w_dtype)
        if not bias_w.is_contiguous():
            bias_w = bias_w.contiguous()
    packed = B if B.is_contiguous() else B.contiguous()
    if packed.dtype != torch.uint8:
        packed = packed.to(torch.uint8)
    if packed.numel() * 2 < N * K_weight:
        raise ValueError(f"packed weight has {packed.numel()} bytes, expected {N * K_weight // 2}")
    _check_absmax_count(quant_state.absmax, N, K_weight, blocksize, "matmul_4bit")

    if M * N * K >= (1 << 27) and ((w_dtype == torch.float32 and (K % 4 != 0 or not DECODE_ONCE)) or
                                   (w_dtype != torch.float32 and (blocksize < 32 or K % 8 != 0))):
        # the 16-bit MFMA / weight-streaming kernels need blocksize >= 32 and K % 8 == 0, the f32 decode-once path K % 4 == 0;
        # anything else runs on the generic one-wave-per-output-column kernel, orders of magnitude slower at this size
        _warn_once("matmul_4bit.generic",
                   f"matmul_4bit: weight dtype {w_dtype}, blocksize {blocksize}, K {K} takes the generic (non-MFMA) kernel; "
                   f"quantize a float16 / bfloat16 weight with blocksize >= 32 and K % 8 == 0 for the fast paths "
                   f"(e.g. Linear4bit.from_linear(linear.to(torch.bfloat16)))")
    out_dtype = compute_dtype if compute_dtype in _native.DTYPE_CODE else w_dtype
    out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    keep: list = []
    am = quant_state.absmax
    desc = _absmax_desc(am if am.device == A.device else am.to(A.device), quant_state.state2, keep)
    # The library's scratch (0 bytes = none needed for this shape): mid-sized M leaves too few output tiles for 256 CUs and
    # K is split over f32 partials; large M (>= 256 rows, >= 1.5 M outputs) decodes the weight ONCE into it (N x K_weight in the weight dtype) and
    # runs a dense MFMA GEMM instead of re-decoding every weight tile per 256 rows.  torch's caching allocator makes the
    # allocation a pointer bump; the memory goes back to the pool on return.
    flags = 0 if DECODE_ONCE else MATMUL_FUSED_ONLY
    ws_bytes = _matmul4_ws_bytes(M, N, K, K_weight, w_code, flags)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=A.device) if ws_bytes > 0 else None
    with on_device(A.device):
        check(_native.lib().mbnb_matmul_4bit(
            ptr(A2), M, K, ptr(packed), ctypes.byref(desc), N, K_weight, int(blocksize),
            _native.QUANT_CODE[quant_state.quant_type], w_code, ptr(bias_w), _native.DTYPE_CODE[out_dtype],
            ptr(out), ptr(ws), ws_bytes, flags, stream_ptr(A.device)), "matmul_4bit")
    if out_dtype != compute_dtype:
        out = out.to(compute_dtype)
    return out if len(orig_shape) == 2 else out.reshape(*orig_shape[:-1], N)


_WS_CACHE: dict = {}


def _matmul4_ws_bytes(M: int, N: int, K: int, K_weight: int, w_code: int, flags: int) -> int:
    """mbnb_matmul_4bit_workspace_bytes, memoised: a pure function of its arguments (a decode loop asks the same question for every token)."""
    key = (M, N, K, K_weight, w_code, flags)
    v = _WS_CACHE.get(key)
    if v is None:
        if len(_WS_CACHE) > 4096:
            _WS_CACHE.clear()
        v = _WS_CACHE[key] = int(_native.lib().mbnb_matmul_4bit_workspace_bytes(M, N, K, K_weight, w_code, flags))
    return v


def matmul_nf4(input: Tensor, weight_packed: Tensor, weight_state: QuantState,
               bias: Optional[Tensor] = None) -> Tensor:
    """Matrix multiplication with NF4-quantized weights (reference functional.py:776-779)."""
    return matmul_4bit(input, weight_packed, weight_state, bias)


def matmul_fp4(input: Tensor, weight_packed: Tensor, weight_state: QuantState,
               bias: Optional[Tensor] = None) -> Tensor:
    """Matrix multiplication with FP4-quantized weights (reference functional.py:782-785)."""
    return matmul_4bit(input, weight_packed, weight_state, bias)


def _group_rows(A: Tensor, weights, biases, compute_dtype: Optional[torch.dtype], max_rows: int = 1):
    """What the fused launch of matmul_4bit_grouped needs -- (K, quant_type, blocksize, w_dtype, [(packed, desc, bias, N), ...], keep) --
    or None where the call is not 1 ... `max_rows` rows times weights of one format (or where a member would not pass matmul_4bit's own
    checks: the member-by-member path then raises what matmul_4bit raises).  Whether the kernel takes the shapes is the library's decision."""
    if torch.is_grad_enabled() and (A.requires_grad or any(b is not None and b.requires_grad for b in biases)):
        return None
    if A.device.type != 'cuda' or A.dim() == 0 or A.shape[-1] == 0 or not 0 < A.numel() <= max_rows * A.shape[-1]:
        return None
    K = int(A.shape[-1])
    first = weights[0][1]
    qt, blocksize, w_dtype = first.quant_type, first.blocksize, first.dtype
    if (w_dtype not in _native.DTYPE_CODE or qt not in _native.QUANT_CODE or not isinstance(blocksize, int) or blocksize <= 0
            or (A.dtype if compute_dtype is None else compute_dtype) != w_dtype):
        return None
    K_weight = _padded(K, blocksize)
    rows, keep = [], []
    for (B, state), bias in zip(weights, biases):
        if (state.quant_type != qt or state.blocksize != blocksize or state.dtype != w_dtype or len(state.shape) != 2
                or int(state.shape[1]) != K or B.device != A.device or B.dtype != torch.uint8 or not B.is_contiguous()):
            return None
        N = int(state.shape[0])
        am = state.absmax
        if N <= 0 or B.numel() * 2 < N * K_weight or am.numel() != N * (K_weight // blocksize):
            return None
        try:
            desc = _absmax_desc(am if am.device == A.device else am.to(A.device), state.state2, keep)
        except ValueError:
            return None
        if bias is not None:
            bias = _as(bias, w_dtype, A.device)   # functional.py:765-766, as matmul_4bit
            keep.append(bias)
        rows.append((B, desc, bias, N))
    return K, qt, blocksize, w_dtype, rows, keep


def matmul_4bit_grouped(
    A: Tensor,
    weights: Sequence[Tuple[Tensor, QuantState]],
    biases: Optional[Sequence[Optional[Tensor]]] = None,
    compute_dtype: Optional[torch.dtype] = None,
) -> Tuple[Tensor, ...]:
    """
    ``tuple(matmul_4bit(A, packed, state, bias, compute_dtype) for (packed, state), bias in zip(weights, biases))`` -- the same
    values bit for bit, the same errors -- with ONE kernel launch per 16 members where A folds to 1 ... 16 rows (the decode step of a
    transformer block, alone or in a served batch: q / k / v share their input, and so do gate / up).

    `weights` is a sequence of ``(packed, QuantState)`` pairs, `biases` one Tensor or None per member (default: no bias).
    An empty sequence returns ``()``.

    The fused launches serve a call in which A folds to 1 ... 16 rows, no gradient is wanted, every member has the same quant_type,
    blocksize and weight dtype, and the output dtype equals the weight dtype; the library then decides on the shapes, and a chunk
    it declines runs member by member:

    - one row: libmbnb_group.so, k_gemv4_group -- the row body of matmul_4bit's own M = 1 kernel behind a member table (blocksize
      64, K a multiple of 64 in 1024 ... 16384, 16-bit dtype, aligned operands, all absmax plain or all double-quantised);
    - 2 ... 16 rows: libmbnb_batch.so, k_skinny4_group -- the workgroup of matmul_4bit's own weight-streaming MFMA kernel for these
      row counts behind the same table (blocksize a power of two >= 32, K a multiple of 128 and of the blocksize in 128 ... 16384,
      16-bit dtype, aligned operands, all absmax plain or all double-quantised).

    Everything else -- 17 rows or more, a gradient (differentiable through matmul_4bit's autograd function), mixed formats, f32
    weights, another compute_dtype -- is the member-by-member loop above.

    On the fused paths the outputs are VIEWS of one allocation of rows * sum(N) elements, each member's a dense [rows, N] block:
    writing to one in place never touches another, but each keeps the whole allocation alive.
    """
    weights = list(weights)
    biases = [None] * len(weights) if biases is None else list(biases)
    if len(biases) != len(weights):
        raise ValueError(f"matmul_4bit_grouped: {len(weights)} weights but {len(biases)} biases")
    if not weights:
        return ()
    def launch(x, M, K, qt, w_dtype, blocksize, table, _, stream):
        if M == 1:
            return _group_native.gemv4(x, K, qt, w_dtype, blocksize, table, stream)
        return _batch_native.gemm4(x, M, K, qt, w_dtype, blocksize, table, stream)

    return _grouped_launch(A, weights, biases, compute_dtype, _batch_native.MAX_M, launch,
                           lambda i: matmul_4bit(A, weights[i][0], weights[i][1], biases[i], compute_dtype))


def _grouped_launch(A: Tensor, weights, biases, compute_dtype: Optional[torch.dtype], max_rows: int, launch, fallback,
                    rank_check=None, rank_of=None, table_row=None):
    """What the three grouped functions do once their arguments are validated: the plan (_group_rows), the member table and the
    outputs (_group_table), the f32 workspace t laid out member by member, the launch, and `fallback(i)` for every member of a chunk
    the library declined -- or for every member, where there is no plan.

    `launch(x, M, K, quant_type, w_dtype, blocksize, table, side_table, stream)` returns one flag per call of the library.  The last
    three arguments belong to a function with adapters: `rank_check(K, w_dtype, rows, M)` gives one entry per member (None: no
    adapter) or None where the fused launch cannot take them, `rank_of(entry)` its R, and `table_row(entry, t)` the row of the side
    table for an entry whose f32 [M, R] block of the workspace starts at address `t`."""
    plan = _group_rows(A, weights, biases, compute_dtype, max_rows)
    M = 0 if plan is None else A.numel() // plan[0]
    ranks = None if plan is None else [] if rank_check is None else rank_check(plan[0], plan[3], plan[4], M)
    if ranks is None:
        return tuple(fallback(i) for i in range(len(weights)))
    K, qt, blocksize, w_dtype, rows, keep = plan
    x, table, outs = _group_table(A, K, w_dtype, rows, M)
    side = None
    if rank_check is not None:
        t = torch.empty(M * sum(rank_of(r) for r in ranks if r is not None), dtype=torch.float32, device=A.device)
        side, t0, o = [], t.data_ptr(), 0
        for r in ranks:
            side.append(table_row(r, t0 + 4 * o))      # t: the f32 [M, R] block of this member
            o += 0 if r is None else M * rank_of(r)
    with on_device(A.device):
        launched = launch(x.data_ptr(), M, K, qt, w_dtype, blocksize, table, side, stream_ptr(A.device))
    for c, ok in enumerate(launched):
        if not ok:    # the library declined this chunk before launching anything: its members through the fallback
            for i in range(c * _group_native.MAX_MEMBERS, min((c + 1) * _group_native.MAX_MEMBERS, len(rows))):
                outs[i] = fallback(i)
    return tuple(outs)


def _group_table(A: Tensor, K: int, w_dtype: torch.dtype, rows, M: int = 1):
    """(x, table, outs) of a fused grouped launch over _group_rows' `rows`: A prepared once for all members (matmul_4bit: A.to(weight
    dtype), contiguous [M, K]), the Member field tuples, and the outputs -- views of ONE allocation of M * sum(N) elements, member g's
    the dense [M, N_g] block."""
    x = _as(A.reshape(M, K), w_dtype)
    out = torch.empty(M * sum(r[3] for r in rows), dtype=w_dtype, device=A.device)
    table, outs, first = [], [], out.data_ptr()
    esize, o = out.element_size(), 0
    for B, desc, bias, N in rows:
        table.append((B.data_ptr(), desc.absmax_f32 or 0, desc.absmax_i8 or 0, desc.absmax2 or 0,
                      0 if bias is None else bias.data_ptr(), first + o * esize, N, desc.blocksize2, 0))
        outs.append(out[o:o + M * N].view(*A.shape[:-1], N))
        o += M * N
    return x, table, outs


def _lora_ranks(A: Tensor, K: int, w_dtype: torch.dtype, rows, adapters):
    """One (lora_A, lora_B, R, scaling) or None per member where the fused adapter launch can take the adapters as they are -- every
    tensor on A's device, in the weight dtype, contiguous, shaped [R, K] and [N, R], no gradient wanted -- else None.  Whether the
    kernels take the ranks and the alignment is the library's decision."""
    ranks = []
    for (_, _, _, N), adapter in zip(rows, adapters):
        if adapter is None:
            ranks.append(None)
            continue
        lora_A, lora_B, scaling = adapter
        R = int(lora_A.shape[0]) if lora_A.dim() == 2 else -1
        for t, shape in ((lora_A, (R, K)), (lora_B, (N, R))):
            if (t.device != A.device or t.dtype != w_dtype or tuple(t.shape) != shape or not t.is_contiguous()
                    or (t.requires_grad and torch.is_grad_enabled())):
                return None
        ranks.append((lora_A, lora_B, R, float(scaling)) if R > 0 else None)
    return ranks


def _lora_composed(A: Tensor, B: Tensor, state: QuantState, bias: Optional[Tensor], adapter, compute_dtype: Optional[torch.dtype]) -> Tensor:
    """One member of matmul_4bit_lora_grouped in its composed form: matmul_4bit (HIP kernels, differentiable in A and the bias) plus the
    adapter in torch ops (torch's GEMM; autograd gives lora_A, lora_B and A their gradients)."""
    y = matmul_4bit(A, B, state, bias, compute_dtype)
    if adapter is None:
        return y
    lora_A, lora_B, scaling = adapter
    x = A if A.dtype == state.dtype else A.to(state.dtype)        # the row as matmul_4bit feeds it
    if x.dtype != lora_A.dtype:
        x = x.to(lora_A.dtype)
    u = ((x @ lora_A.t()) @ lora_B.t()) * scaling
    return y + (u if u.dtype == y.dtype else u.to(y.dtype))


def matmul_4bit_lora_grouped(
    A: Tensor,
    weights: Sequence[Tuple[Tensor, QuantState]],
    adapters: Sequence[Optional[Tuple[Tensor, Tensor, float]]],
    biases: Optional[Sequence[Optional[Tensor]]] = None,
    compute_dtype: Optional[torch.dtype] = None,
) -> Tuple[Tensor, ...]:
    """
    `matmul_4bit_grouped` for layers that carry un-merged LoRA adapters (a LoRA trained over a 4-bit base cannot be merged into it):
    per member, ``A @ dequant(W)^T + bias + float32(scaling) * (A @ lora_A^T) @ lora_B^T``.

    `adapters` holds one entry per member: ``None`` or ``(lora_A [r, K], lora_B [N, r], scaling)``.  Returns a tuple of outputs, as
    `matmul_4bit_grouped` does.  With every adapter ``None`` the call IS `matmul_4bit_grouped`.

    What is promised is a BOUND, not bit-equality between the paths (unlike `matmul_4bit_grouped`): each element lies within the
    elementwise bounds of DESIGN.md 17 around the float64 value of the expression above, on whichever path computed it.  A member
    whose adapter is ``None`` equals `matmul_4bit` bit for bit on every path.

    The bound holds on three paths.  Two are fused and make TWO launches per 16 members, the down-projections t = A . lora_A^T in f32
    for every adapter row of every member, then the grouped base launch whose elements add ``scaling * lora_B[n, :] . t[m, :]`` to
    their f32 sum before the bias and the one rounding:

    - A folds to one row: libmbnb_lora.so, `k_lora_down` and `k_gemv4_group_lora`;
    - A folds to 2 ... 16 rows: libmbnb_batch.so, `k_lora_down_rows` and `k_skinny4_group` with its rank-r epilogue.  Every row of
      the batch uses the member's one adapter; a different adapter per row is not part of this function.  For these row counts
      the value's bits differ from the releases that ran the composed form here -- one rounding to the weight dtype instead of
      five -- which is inside the contract above, not outside it.

    They serve a call that `matmul_4bit_grouped` would fuse (1 ... 16 rows, no gradient wanted, one quant_type / blocksize / weight
    dtype, output dtype = weight dtype) in which every adapter tensor is on A's device, in the weight dtype, contiguous, shaped
    ``[r, K]`` / ``[N, r]`` and wants no gradient; the library then decides on the shapes (those of the grouped launch for that
    row count, and 1 <= r <= 256 with aligned operands), and a chunk it declines runs through the composed form.  The outputs are
    views of one allocation, the f32 workspaces slices of another.

    Everything else -- 17 rows or more, a wanted gradient, mixed formats, r > 256, another dtype -- runs ONE composed form per
    member: `matmul_4bit` (this library's HIP kernels, differentiable in A and the bias) plus
    ``((A.to(T) @ lora_A.t()) @ lora_B.t()) * scaling`` in torch ops.  That half is torch's GEMM, NOT a HIP kernel of this library;
    autograd gives lora_A, lora_B and A their gradients through it.  An efficient adapter path for prefill and training is not
    part of this function.
    """
    weights, adapters = list(weights), list(adapters)
    biases = [None] * len(weights) if biases is None else list(biases)
    if len(biases) != len(weights):
        raise ValueError(f"matmul_4bit_lora_grouped: {len(weights)} weights but {len(biases)} biases")
    if len(adapters) != len(weights):
        raise ValueError(f"matmul_4bit_lora_grouped: {len(weights)} weights but {len(adapters)} adapters")
    if all(adapter is None for adapter in adapters):
        return matmul_4bit_grouped(A, weights, biases, compute_dtype)

    def launch(x, M, K, qt, w_dtype, blocksize, table, rank_table, stream):
        if M == 1:
            return _lora_native.gemv4(x, K, qt, w_dtype, blocksize, table, rank_table, stream)
        return _batch_native.gemm4_lora(x, M, K, qt, w_dtype, blocksize, table, rank_table, stream)

    return _grouped_launch(A, weights, biases, compute_dtype, _batch_native.MAX_M, launch,
                           lambda i: _lora_composed(A, weights[i][0], weights[i][1], biases[i], adapters[i], compute_dtype),
                           lambda K, w_dtype, rows, M: _lora_ranks(A, K, w_dtype, rows, adapters),
                           lambda r: r[2],
                           lambda r, t: _lora_native.NO_ADAPTER if r is None else (r[0].data_ptr(), r[1].data_ptr(), t, r[2], r[3]))


def _multilora_ranks(A: Tensor, K: int, w_dtype: torch.dtype, rows, banks):
    """One (lora_A, lora_B, scaling, R, S) or None per member where the fused per-row adapter launch can take the banks as they are --
    every tensor on A's device and contiguous, lora_A [S, R, K] and lora_B [S, N, R] in the weight dtype, scaling f32 [S], R <= 64, no
    gradient wanted -- else None.  The alignment is the library's decision."""
    ranks = []
    for (_, _, _, N), bank in zip(rows, banks):
        if bank is None:
            ranks.append(None)
            continue
        lora_A, lora_B, scaling = bank
        S, R = (int(lora_A.shape[0]), int(lora_A.shape[1])) if lora_A.dim() == 3 else (-1, -1)
        for t, dtype, shape in ((lora_A, w_dtype, (S, R, K)), (lora_B, w_dtype, (S, N, R)), (scaling, torch.float32, (S,))):
            if (t.device != A.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                    or (t.requires_grad and torch.is_grad_enabled())):
                return None
        if R > _mlora_native.MAX_R:
            return None
        ranks.append((lora_A, lora_B, scaling, R, S) if R > 0 and S > 0 else None)
    return ranks


def _multilora_composed(A: Tensor, B: Tensor, state: QuantState, bias: Optional[Tensor], bank, ids: Tensor,
                        compute_dtype: Optional[torch.dtype]) -> Tensor:
    """One member of matmul_4bit_multilora_grouped in its composed form: matmul_4bit (HIP kernels, differentiable in A and the bias),
    then one slot after the other in torch ops, each selected by row with `where` -- a row without an adapter keeps matmul_4bit's
    bits, and what an unselected slot holds (a NaN included) never reaches a row.  The ids stay on the device."""
    y = matmul_4bit(A, B, state, bias, compute_dtype)
    if bank is None:
        return y
    lora_A, lora_B, scaling = bank
    x = A if A.dtype == state.dtype else A.to(state.dtype)        # the rows as matmul_4bit feeds them
    if x.dtype != lora_A.dtype:
        x = x.to(lora_A.dtype)
    for s in range(int(lora_A.shape[0])):
        u = ((x @ lora_A[s].t()) @ lora_B[s].t()) * scaling[s]        # a 0-dim f32 factor: u keeps its dtype
        y = torch.where((ids == s).unsqueeze(-1), y + (u if u.dtype == y.dtype else u.to(y.dtype)), y)
    return y


def matmul_4bit_multilora_grouped(
    A: Tensor,
    weights: Sequence[Tuple[Tensor, QuantState]],
    banks: Sequence[Optional[Tuple[Tensor, Tensor, Tensor]]],
    adapter_ids: Tensor,
    biases: Optional[Sequence[Optional[Tensor]]] = None,
    compute_dtype: Optional[torch.dtype] = None,
) -> Tuple[Tensor, ...]:
    """
    `matmul_4bit_lora_grouped` for a served batch whose rows carry DIFFERENT un-merged adapters (continuous batching over one frozen
    4-bit base): per member and row m, with ``s = adapter_ids[m]``,
    ``A[m] @ dequant(W)^T + bias + scaling[s] * (A[m] @ lora_A[s]^T) @ lora_B[s]^T``.

    `banks` holds one entry per member: ``None`` or ``(lora_A [S, r, K], lora_B [S, N, r], scaling)`` with `scaling` an f32 ``[S]``
    tensor on A's device; S must be equal across the banks.  `adapter_ids` is an integer tensor of shape ``A.shape[:-1]`` on A's
    device.  A row whose id lies outside ``[0, S)`` -- -1, S, anything else -- uses NO adapter: its values are `matmul_4bit`'s bit for
    bit on every path (out-of-range ids are skipped, as `spmm_coo` skips them: a check that raises would synchronise).  The ids are
    never read on the host.  An int32 contiguous tensor is passed to the kernels as it is, so a caller may overwrite it in place
    between the replays of a captured graph; anything else is converted once per call.  With every bank ``None`` the call IS
    `matmul_4bit_grouped`.

    What is promised is the BOUND of `matmul_4bit_lora_grouped` around the float64 value formed with each row's adapter.  Two paths:

    - A folds to 2 ... 16 rows in a call `matmul_4bit_grouped` would fuse, every bank tensor is in the weight dtype (the scaling in
      f32), contiguous, on A's device, r <= 64, and no gradient is wanted: libmbnb_mlora.so, TWO launches per 16 members --
      `k_lora_down_sel` (t[m] = lora_A[s] . A[m] in f32) and `k_skinny4_mlora`, the grouped base launch with a per-row rank-r
      epilogue.  Row m then equals, bit for bit, row m of `matmul_4bit_lora_grouped` on its 2 ... 16 row path with the adapters
      ``(lora_A[s], lora_B[s], float(scaling[s]))``.  The library decides on shapes and alignment; a chunk it declines runs composed.
    - Everything else -- 1 row, 17 rows or more, r > 64, a wanted gradient, mixed formats, an f32 bank -- runs the composed form per
      member: `matmul_4bit`, then per slot ``torch.where(ids == s, y + ((x @ lora_A[s].t()) @ lora_B[s].t()) * scaling[s], y)``:
      sync-free, differentiable in A, the bias and the bank, and S small torch GEMMs over all rows per member.
    """
    weights, banks = list(weights), list(banks)
    biases = [None] * len(weights) if biases is None else list(biases)
    if len(biases) != len(weights):
        raise ValueError(f"matmul_4bit_multilora_grouped: {len(weights)} weights but {len(biases)} biases")
    if len(banks) != len(weights):
        raise ValueError(f"matmul_4bit_multilora_grouped: {len(weights)} weights but {len(banks)} banks")
    if all(bank is None for bank in banks):
        return matmul_4bit_grouped(A, weights, biases, compute_dtype)
    slots = {int(bank[0].shape[0]) for bank in banks if bank is not None}
    if len(slots) != 1:
        raise ValueError(f"matmul_4bit_multilora_grouped: the banks hold {sorted(slots)} adapters; one S for all banks is needed")
    if tuple(adapter_ids.shape) != tuple(A.shape[:-1]):
        raise ValueError(f"matmul_4bit_multilora_grouped: adapter_ids has shape {tuple(adapter_ids.shape)}, A has rows {tuple(A.shape[:-1])}")
    if adapter_ids.dtype.is_floating_point or adapter_ids.dtype.is_complex or adapter_ids.dtype == torch.bool:
        raise TypeError(f"matmul_4bit_multilora_grouped: adapter_ids must be an integer tensor, got {adapter_ids.dtype}")

    ids = adapter_ids

    def rank_check(K, w_dtype, rows, M):
        nonlocal ids
        ranks = None if M < _mlora_native.MIN_M or adapter_ids.device != A.device else _multilora_ranks(A, K, w_dtype, rows, banks)
        if ranks is not None and not (ids.dtype == torch.int32 and ids.is_contiguous()):
            ids = ids.to(torch.int32).contiguous()      # once per call, before the outputs are allocated
        return ranks

    def launch(x, M, K, qt, w_dtype, blocksize, table, bank_table, stream):
        return _mlora_native.gemm4(x, M, K, qt, w_dtype, blocksize, table, bank_table, ids.data_ptr(), stream)

    return _grouped_launch(A, weights, biases, compute_dtype, _mlora_native.MAX_M, launch,
                           lambda i: _multilora_composed(A, weights[i][0], weights[i][1], biases[i], banks[i], adapter_ids, compute_dtype),
                           rank_check, lambda r: r[3],
                           lambda r, t: _mlora_native.NO_BANK if r is None else (r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), t, r[3], r[4]))


def matmul_int8(A: Tensor, B: Tensor, A_scales: Tensor, B_scales: Tensor,
                dtype: torch.dtype = torch.float16) -> Tensor:
    """
    INT8 matmul with fused dequantization (reference: functional.py:788-793).

    A int8 [M, K] with one scale per row; B int8 [K, N] with one scale per column.  Computed as
    ``int32(A·B) * (sA[m]/127) * (sB[n]/127)`` on the int8 MFMA (what the reference's Metal kernel
    mm:155-196 computes; equal to the reference CPU formulation within 4e-4 rel-err).
    """
    _check_device(A, "matmul_int8")
    _check_device(B, "matmul_int8")
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise RuntimeError(f"matmul_int8: shapes {tuple(A.shape)} and {tuple(B.shape)} cannot be multiplied")
    A = A.contiguous()
    B = B.contiguous()
    if A.dtype != torch.int8 or B.dtype != torch.int8:
        raise TypeError("matmul_int8: A and B must be int8")
    M, K = A.shape
    N = B.shape[1]
    sa = A_scales.to(device=A.device, dtype=torch.float32).contiguous().view(-1)
    sb = B_scales.to(device=A.device, dtype=torch.float32).contiguous().view(-1)
    if sa.numel() != M or sb.numel() != N:
        raise ValueError(f"matmul_int8: need {M} A_scales and {N} B_scales, got {sa.numel()} and {sb.numel()}")
    out_dtype = dtype if dtype in _native.DTYPE_CODE else torch.float32
    out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    # large aligned problems are read in place ([K, N] through a transposing LDS read); the rest need an N*K-byte scratch
    ws_bytes = int(_native.lib().mbnb_matmul_int8_workspace_bytes(M, N, K))
    if not DECODE_ONCE and K % 128 == 0 and N % 16 == 0 and ((M + 255) // 256) * ((N + 255) // 256) >= 96:
        ws_bytes = 0      # large aligned problems without scratch: B read in place as [K, N] (no transpose)
    workspace = torch.empty(ws_bytes, dtype=torch.int8, device=A.device) if ws_bytes > 0 else None
    with on_device(A.device):
        check(_native.lib().mbnb_matmul_int8(
            ptr(A), ptr(B), ptr(sa), ptr(sb), M, N, K, _native.DTYPE_CODE[out_dtype], ptr(out), ptr(workspace), ws_bytes,
            stream_ptr(A.device)), "matmul_int8")
    return out if out_dtype == dtype else out.to(dtype)


def linear_int8(input: Tensor, weight_int8: Tensor, weight_scales: Tensor, bias: Optional[Tensor] = None,
                dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    ``input[..., K] @ dequantize_rowwise(weight_int8[N, K], weight_scales, dtype)^T + bias`` in one
    kernel — the forward of Linear8bit (reference: nn/linear8bit.py:70-102; native binding
    `_C.linear_int8`, mm:1836-1886).
    """
    if (input.requires_grad or (bias is not None and bias.requires_grad)) and torch.is_grad_enabled():
        return _LinearInt8Grad.apply(input, weight_int8, weight_scales, bias, dtype)
    _check_device(input, "linear_int8")
    _check_device(weight_int8, "linear_int8")
    if dtype is None:
        dtype = input.dtype
    dcode = dtype_code(dtype, "linear_int8")
    N, K = weight_int8.shape
    if input.shape[-1] != K:
        raise RuntimeError(f"linear_int8: input width {input.shape[-1]} does not match weight {tuple(weight_int8.shape)}")
    x = _as(input if input.dim() == 2 else input.reshape(-1, K), dtype)      # (no-op conversions skipped: ~1 us of host time each)
    M = x.shape[0]
    w = weight_int8 if weight_int8.is_contiguous() else weight_int8.contiguous()
    s = _as(weight_scales, torch.float32, x.device)
    b = None if bias is None else _as(bias, dtype, x.device)
    out = torch.empty(M, N, dtype=dtype, device=x.device)
    flags = 0 if DECODE_ONCE else MATMUL_FUSED_ONLY
    ws_bytes = int(_native.lib().mbnb_linear_int8_workspace_bytes(M, N, K, flags)) if M > 16 else 0   # split-K partials / the dequantised weight
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
    with on_device(x.device):
        check(_native.lib().mbnb_linear_int8(ptr(x), dcode, M, K, ptr(w), ptr(s), N, ptr(b), ptr(out), ptr(ws), ws_bytes,
                                             flags, stream_ptr(x.device)), "linear_int8")
    return out if input.dim() == 2 else out.reshape(*input.shape[:-1], N)


def linear_dense(input: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """
    ``input[..., K] @ weight[N, K]^T + bias`` on an ALREADY dequantised 16-bit weight: the dense MFMA GEMM the decode-once
    paths run after their dequantise pass (csrc/gemm_dense.h), for callers that keep the dequantised weight -- Linear8bit's
    cache (reference nn/linear8bit.py:70-102: `F.linear(x, self._get_weight(), bias)`).  Same slice plan, hence the same bits,
    as ``linear_int8`` / ``matmul_4bit`` on the quantised weight at that shape.  K % 64 == 0, K >= 128.
    """
    if (input.requires_grad or (bias is not None and bias.requires_grad)) and torch.is_grad_enabled():
        return _LinearDenseGrad.apply(input, weight, bias)
    _check_device(input, "linear_dense")
    _check_device(weight, "linear_dense")
    dtype = weight.dtype
    dcode = dtype_code(dtype, "linear_dense")
    N, K = weight.shape
    if input.shape[-1] != K:
        raise RuntimeError(f"linear_dense: input width {input.shape[-1]} does not match weight {tuple(weight.shape)}")
    x = input.reshape(-1, K).to(dtype).contiguous()
    M = x.shape[0]
    w = weight.contiguous()
    b = None if bias is None else bias.to(device=x.device, dtype=dtype).contiguous()
    out = torch.empty(M, N, dtype=dtype, device=x.device)
    ws_bytes = int(_native.lib().mbnb_gemm_dense_workspace_bytes(M, N, K))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
    with on_device(x.device):
        check(_native.lib().mbnb_gemm_dense(ptr(x), ptr(w), dcode, ptr(b), dcode, ptr(out), M, N, K, K, ptr(ws), ws_bytes, 0,
                                            stream_ptr(x.device)), "linear_dense")
    return out.reshape(*input.shape[:-1], N)


def dense_path_applies(M: int, N: int, K: int) -> bool:
    """True where ``linear_int8`` / ``matmul_4bit`` take the decode-once path (dequantise into scratch + dense GEMM)."""
    return bool(_native.lib().mbnb_gemm_dense_applies(M, N, K, K))


# ============================================================================= FP8 E4M3 (the reference's own format)
def quantize_fp8_e4m3(tensor: Tensor) -> Tuple[Tensor, Tensor]:
    """
    Row-wise FP8 E4M3 quantization in the reference's format (functional.py:643-663, encoder :1086-1163), bit-exact:
    returns (uint8 [rows, cols], scales f32 [rows]) with scales = clamp(max|row| / 448, 1e-12).  The encoder is the
    reference's, not the OCP conversion (no mantissa carry, subnormals flushed, |v| >= 256 saturates to 240).
    """
    if tensor.dim() != 2:
        raise ValueError("Input must be 2D")
    _check_device(tensor, "quantize_fp8_e4m3")
    A = tensor if tensor.dtype in _native.DTYPE_CODE else tensor.float()
    A = A.contiguous()
    rows, cols = A.shape
    out = torch.empty(rows, cols, dtype=torch.uint8, device=A.device)
    scales = torch.empty(rows, dtype=torch.float32, device=A.device)
    with on_device(A.device):
        check(_native.lib().mbnb_quantize_fp8_e4m3(ptr(A), dtype_code(A.dtype, "quantize_fp8_e4m3"), rows, cols, ptr(out),
                                                   ptr(scales), stream_ptr(A.device)), "quantize_fp8_e4m3")
    return out, scales


def dequantize_fp8_e4m3(quantized: Tensor, scales: Tensor, dtype: torch.dtype = torch.float16) -> Tensor:
    """decode(byte) * scales[row] -> dtype (functional.py:666-673, decoder :1166-1215), bit-exact."""
    _check_device(quantized, "dequantize_fp8_e4m3")
    q = quantized.contiguous()
    rows, cols = q.shape
    s = scales.to(device=q.device, dtype=torch.float32).contiguous()
    out = torch.empty(rows, cols, dtype=dtype, device=q.device)
    with on_device(q.device):
        check(_native.lib().mbnb_dequantize_fp8_e4m3(ptr(q), ptr(s), rows, cols, dtype_code(dtype, "dequantize_fp8_e4m3"),
                                                     ptr(out), stream_ptr(q.device)), "dequantize_fp8_e4m3")
    return out


def matmul_fp8_e4m3(input: Tensor, weight: Tensor, weight_scales: Tensor, bias: Optional[Tensor] = None,
                    dtype: torch.dtype = torch.float16) -> Tensor:
    """
    ``input[..., K] @ dequantize_fp8_e4m3(weight[N, K], weight_scales, dtype)^T + bias`` (functional.py:796-807) in one
    kernel: the W8A16 GEMMs of linear_int8 with the FP8 byte decoder in the weight producer.
    """
    if (input.requires_grad or (bias is not None and bias.requires_grad)) and torch.is_grad_enabled():
        return _MatMulFP8Grad.apply(input, weight, weight_scales, bias, dtype)
    _check_device(input, "matmul_fp8_e4m3")
    _check_device(weight, "matmul_fp8_e4m3")
    dcode = dtype_code(dtype, "matmul_fp8_e4m3")
    N, K = weight.shape
    is_1d = input.dim() == 1
    x = (input.unsqueeze(0) if is_1d else input)
    if x.shape[-1] != K:
        raise RuntimeError(f"matmul_fp8_e4m3: input width {x.shape[-1]} does not match weight {tuple(weight.shape)}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K).to(dtype).contiguous()
    M = x2.shape[0]
    w = weight.contiguous()
    s = weight_scales.to(device=x2.device, dtype=torch.float32).contiguous()
    b = None if bias is None else bias.to(device=x2.device, dtype=dtype).contiguous()
    out = torch.empty(M, N, dtype=dtype, device=x2.device)
    flags = 0 if DECODE_ONCE else MATMUL_FUSED_ONLY
    ws_bytes = int(_native.lib().mbnb_linear_int8_workspace_bytes(M, N, K, flags)) if M > 16 else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x2.device) if ws_bytes > 0 else None
    with on_device(x2.device):
        check(_native.lib().mbnb_linear_fp8(ptr(x2), dcode, M, K, ptr(w), ptr(s), N, ptr(b), ptr(out), ptr(ws), ws_bytes,
                                            flags, stream_ptr(x2.device)), "matmul_fp8_e4m3")
    out = out.reshape(*lead, N)
    return out.squeeze(0) if is_1d else out


# ============================================================================= input gradients (QLoRA training)
# The reference's CPU path ends every quantised linear in F.linear on the dequantised weight (functional.py:767, :806,
# nn/linear8bit.py:102), so autograd gives it dX and bias.grad.  Here each forward above takes the autograd route only when grad mode
# is on and the input or the bias requires grad (otherwise nothing changes, not even a dispatch); the Function's forward is the plain
# forward (grad mode is off inside it) and its backward runs mbnb_linear_grad_input:
#   dX = cast(round_w(grad_out.to(w_dtype) @ dequant(W)), A.dtype),   bias.grad = grad_out.to(w_dtype) summed over rows in f32 -> w_dtype -> bias.dtype
# -- the gradients torch's autograd gives the reference's `F.linear(A.to(w_dtype), dequant(W), bias.to(w_dtype)).to(compute_dtype)`.
# Only references to the quantised weight and its state are kept for backward: never A, never a dequantised copy of the weight (the
# weight's transposed dequantised form lives in the backward call's transient workspace).  The weights are buffers: no weight gradient.
_FMT_INT8, _FMT_FP8, _FMT_DENSE = _native.W_INT8_ROWWISE, _native.W_FP8_E4M3, _native.W_DENSE


def _grad_input(dY: Tensor, fmt: int, W: Tensor, desc: Optional[AbsmaxDesc], scales: Optional[Tensor], K: int, K_weight: int,
                blocksize: int, w_dtype: torch.dtype, out_dtype: torch.dtype) -> Tensor:
    """dX [M, K] = dY [M, N] (contiguous, w_dtype) . dequant(W) [N, K], through mbnb_linear_grad_input."""
    M, N = dY.shape
    w_code = dtype_code(w_dtype, "linear_grad_input")
    if out_dtype not in _native.DTYPE_CODE:
        return _grad_input(dY, fmt, W, desc, scales, K, K_weight, blocksize, w_dtype, w_dtype).to(out_dtype)
    dX = torch.empty(M, K, dtype=out_dtype, device=dY.device)
    ws_bytes = int(_native.lib().mbnb_linear_grad_input_workspace_bytes(M, N, K, fmt, w_code))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dY.device) if ws_bytes > 0 else None
    with on_device(dY.device):
        check(_native.lib().mbnb_linear_grad_input(
            ptr(dY), M, N, fmt, ptr(W), None if desc is None else ctypes.byref(desc), ptr(scales), K, K_weight, int(blocksize), w_code,
            _native.DTYPE_CODE[out_dtype], ptr(dX), ptr(ws), ws_bytes, 0, stream_ptr(dY.device)), "linear_grad_input")
    return dX


def _backward(ctx, grad_out: Tensor, bias_index: int, fmt: int, W: Tensor, desc, scales) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(dA, dbias) of one quantised linear; `ctx` carries the shapes and dtypes its forward recorded."""
    g = grad_out if grad_out.dim() == 2 else grad_out.reshape(-1, grad_out.shape[-1])
    g = _as(g, ctx.w_dtype)      # an expanded (stride-0) or non-contiguous grad_out becomes a dense w_dtype matrix
    dA = dbias = None
    if ctx.needs_input_grad[0]:
        dA = _grad_input(g, fmt, W, desc, scales, ctx.K, ctx.K_weight, ctx.blocksize, ctx.w_dtype, ctx.a_dtype).reshape(ctx.a_shape)
    if ctx.needs_input_grad[bias_index]:
        dbias = g.sum(0, dtype=torch.float32).to(ctx.w_dtype).to(ctx.bias_dtype)
    return dA, dbias


def _record(ctx, A: Tensor, bias: Optional[Tensor], w_dtype: torch.dtype, K: int, K_weight: int, blocksize: int = 0) -> None:
    ctx.a_shape, ctx.a_dtype = A.shape, A.dtype
    ctx.bias_dtype = None if bias is None else bias.dtype
    ctx.w_dtype, ctx.K, ctx.K_weight, ctx.blocksize = w_dtype, K, K_weight, blocksize


class _MatMul4bitGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, quant_state, bias, compute_dtype):
        out = matmul_4bit(A, B, quant_state, bias, compute_dtype)
        K = int(quant_state.shape[1])
        _record(ctx, A, bias, quant_state.dtype, K, _padded(K, quant_state.blocksize), quant_state.blocksize)
        ctx.save_for_backward(B)
        ctx.quant_state = quant_state
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (B,) = ctx.saved_tensors
        st = ctx.quant_state
        packed = B if B.is_contiguous() else B.contiguous()
        if packed.dtype != torch.uint8:
            packed = packed.to(torch.uint8)
        keep: list = []
        desc = _absmax_desc(st.absmax if st.absmax.device == packed.device else st.absmax.to(packed.device), st.state2, keep)
        fmt = _native.QUANT_CODE[st.quant_type]
        dA, dbias = _backward(ctx, grad_out, 3, fmt, packed, desc, None)   # `keep` holds the absmax tensors until the launch
        return dA, None, None, dbias, None


class _LinearInt8Grad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight_int8, weight_scales, bias, dtype):
        out = linear_int8(input, weight_int8, weight_scales, bias, dtype)
        K = int(weight_int8.shape[1])
        _record(ctx, input, bias, out.dtype, K, K)
        ctx.save_for_backward(weight_int8, weight_scales)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        w, s = ctx.saved_tensors
        w = w if w.is_contiguous() else w.contiguous()
        s = _as(s, torch.float32, w.device)
        dA, dbias = _backward(ctx, grad_out, 3, _FMT_INT8, w, None, s)
        return dA, None, None, dbias, None


class _LinearDenseGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight, bias):
        out = linear_dense(input, weight, bias)
        K = int(weight.shape[1])
        _record(ctx, input, bias, weight.dtype, K, K)
        ctx.save_for_backward(weight)       # Linear8bit's cached dequantised weight: a reference, no copy
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (w,) = ctx.saved_tensors
        w = w if w.is_contiguous() else w.contiguous()
        dA, dbias = _backward(ctx, grad_out, 2, _FMT_DENSE, w, None, None)
        return dA, None, dbias


class _MatMulFP8Grad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight, weight_scales, bias, dtype):
        out = matmul_fp8_e4m3(input, weight, weight_scales, bias, dtype)
        K = int(weight.shape[1])
        _record(ctx, input, bias, dtype, K, K)
        ctx.save_for_backward(weight, weight_scales)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        w, s = ctx.saved_tensors
        w = w if w.is_contiguous() else w.contiguous()
        s = _as(s, torch.float32, w.device)
        dA, dbias = _backward(ctx, grad_out, 3, _FMT_FP8, w, None, s)
        return dA, None, None, dbias, None


def _dequantize_t(weight: Tensor, quant_state: Optional[QuantState] = None, scales: Optional[Tensor] = None, fmt: str = "4bit",
                  dtype: Optional[torch.dtype] = None) -> Tensor:
    """The transposed dequantise pass of the input gradient on its own: ``dequantize_*(weight).t()`` as a contiguous [K, N] tensor, the
    bits the backward's GEMM reads.  fmt "4bit" (packed weight + quant_state), "int8" / "fp8" (weight [N, K] + scales, `dtype`) or
    "dense" (a 16-bit [N, K] weight).  16-bit outputs only.  For tests and tools."""
    _check_device(weight, "_dequantize_t")
    keep: list = []
    desc, s = None, None
    if fmt == "4bit":
        N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
        blocksize, dtype = quant_state.blocksize, quant_state.dtype
        K_weight = _padded(K, blocksize)
        _check_absmax_count(quant_state.absmax, N, K_weight, blocksize, "_dequantize_t")
        W = _as(weight, torch.uint8)
        if W.numel() * 2 < N * K_weight:
            raise ValueError(f"packed weight has {W.numel()} bytes, expected {N * K_weight // 2}")
        desc = _absmax_desc(quant_state.absmax.to(W.device), quant_state.state2, keep)
        code = _native.QUANT_CODE[quant_state.quant_type]
    else:
        W = weight.contiguous()
        N, K = W.shape
        K_weight, blocksize = K, 0
        if fmt == "dense":
            dtype, code = W.dtype, _FMT_DENSE
        else:
            code = {"int8": _FMT_INT8, "fp8": _FMT_FP8}[fmt]
            s = _as(scales, torch.float32, W.device)
            if s.numel() != N:
                raise ValueError(f"scales has {s.numel()} elements, expected {N}")
    w_code = dtype_code(dtype, "_dequantize_t")
    out = torch.empty(K, N, dtype=dtype, device=W.device)
    with on_device(W.device):
        check(_native.lib().mbnb_linear_grad_input(
            None, 0, N, code, ptr(W), None if desc is None else ctypes.byref(desc), ptr(s), K, K_weight, int(blocksize), w_code, w_code,
            ptr(out), None, 0, _native.GRAD_TRANSPOSE_ONLY, stream_ptr(W.device)), "_dequantize_t")
    return out


# ============================================================================= SwitchBack (trainable int8 linear)
# SwitchBackLinear (reference nn/switchback.py) keeps an int8 copy of its weight for the forward and a 16-bit master weight `weight_fp`
# that receives the gradient.  The forward restates SwitchBackFunction.forward: Wd = round_T(q * round_T(s / 127)) -- not
# dequantize_rowwise, which rounds once -- then round_T(X . Wd^T), then `+ bias` as a separate op (libmbnb_train.so,
# include/mbnb_train.h).  The backward is the reference's three products on weight_fp: dX = dY . weight_fp through
# mbnb_linear_grad_input's dense format, dW = dY^T . X through mbnb_linear_grad_weight, db = dY summed over rows in f32.
def _switchback_forward(input: Tensor, weight_int8: Tensor, weight_scales: Tensor, bias: Optional[Tensor] = None, flags: int = 0) -> Tensor:
    """``input[..., K] . Wd^T (+ bias)`` with SwitchBack's weight rule, in the input's dtype.  A bias of another dtype is added the way the
    reference adds it (torch's `output + bias`, with type promotion).  `flags`: include/mbnb_train.h, for tests."""
    _check_device(input, "switchback_linear")
    _check_device(weight_int8, "switchback_linear")
    dtype = input.dtype
    dcode = dtype_code(dtype, "switchback_linear")
    N, K = weight_int8.shape
    if input.shape[-1] != K:
        raise RuntimeError(f"switchback_linear: input width {input.shape[-1]} does not match weight {tuple(weight_int8.shape)}")
    x = _as(input.reshape(-1, K), dtype)
    M = x.shape[0]
    w = _as(weight_int8, torch.int8)
    s = _as(weight_scales, torch.float32, x.device)
    if s.numel() != N:
        raise ValueError(f"weight_scales has {s.numel()} elements, expected {N}")
    b = late = None
    if bias is not None:
        if bias.dtype == dtype:
            b = _as(bias, dtype, x.device)
        else:
            late = bias
    out = torch.empty(M, N, dtype=dtype, device=x.device)
    handle = _train_native.lib()
    ws_bytes = int(handle.mbnb_switchback_forward_workspace_bytes(M, N, K, dcode))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
    with on_device(x.device):
        _train_native.check(handle.mbnb_switchback_forward(ptr(x), dcode, M, K, ptr(w), ptr(s), N, ptr(b), ptr(out), ptr(ws), ws_bytes,
                                                           int(flags), stream_ptr(x.device)), "switchback_linear")
    if late is not None:
        out = out + late.to(x.device)
    return out.reshape(*input.shape[:-1], N)


def _switchback_dequant(weight_int8: Tensor, weight_scales: Tensor, dtype: torch.dtype) -> Tensor:
    """The forward's first pass on its own: Wd [N, K] = round_T(q * round_T(s / 127)) in `dtype`, the bits its GEMM reads.  For tests
    and tools."""
    _check_device(weight_int8, "_switchback_dequant")
    w = _as(weight_int8, torch.int8)
    N, K = w.shape
    s = _as(weight_scales, torch.float32, w.device)
    dcode = dtype_code(dtype, "_switchback_dequant")
    out = torch.empty(N, K, dtype=dtype, device=w.device)
    with on_device(w.device):
        _train_native.check(_train_native.lib().mbnb_switchback_forward(None, dcode, 0, K, ptr(w), ptr(s), N, None, ptr(out), None, 0,
                                                                        _train_native.PASS_ONLY, stream_ptr(w.device)), "_switchback_dequant")
    return out


def _linear_grad_weight(grad_output: Tensor, input: Tensor, flags: int = 0) -> Tensor:
    _check_device(grad_output, "linear_grad_weight")
    _check_device(input, "linear_grad_weight")
    dtype = grad_output.dtype
    if input.dtype != dtype:
        raise RuntimeError(f"linear_grad_weight: expected grad_output and input to have the same dtype, but got: {dtype} != {input.dtype}")
    dcode = dtype_code(dtype, "linear_grad_weight")
    N, K = grad_output.shape[-1], input.shape[-1]
    g = _as(grad_output.reshape(-1, N), dtype)
    x = _as(input.reshape(-1, K), dtype, g.device)
    M = g.shape[0]
    if x.shape[0] != M:
        raise RuntimeError(f"linear_grad_weight: grad_output has {M} rows, input {x.shape[0]}")
    dW = torch.empty(N, K, dtype=dtype, device=g.device)
    handle = _train_native.lib()
    ws_bytes = int(handle.mbnb_linear_grad_weight_workspace_bytes(M, N, K, dcode))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device) if ws_bytes > 0 else None
    with on_device(g.device):
        _train_native.check(handle.mbnb_linear_grad_weight(ptr(g), ptr(x), M, N, K, dcode, ptr(dW), ptr(ws), ws_bytes, int(flags),
                                                           stream_ptr(g.device)), "linear_grad_weight")
    return dW


def linear_grad_weight(grad_output: Tensor, input: Tensor) -> Tensor:
    """The weight gradient of a linear: ``dW[N, K] = grad_output[..., N]^T . input[..., K]``, summed over every leading position, in the
    common dtype (f16 / bf16 / f32), f32 accumulation, one rounding -- torch.mm(grad_output_2d.t(), input_2d) of the reference's
    SwitchBackFunction.backward."""
    return _linear_grad_weight(grad_output, input)


def _transpose_pad(input: Tensor) -> Tensor:
    """The weight gradient's transposing pass on its own: a 16-bit [M, C] matrix as [C, Mp] with zero columns M .. Mp-1 (Mp: M rounded up
    to a multiple of 64, at least 128), the operand layout its GEMM reads.  For tests and tools."""
    _check_device(input, "_transpose_pad")
    x = input.contiguous()
    M, C = x.shape
    dcode = dtype_code(x.dtype, "_transpose_pad")
    out = torch.empty(C, _train_native.padded_rows(M), dtype=x.dtype, device=x.device)
    with on_device(x.device):
        _train_native.check(_train_native.lib().mbnb_linear_grad_weight(None, ptr(x), M, 0, C, dcode, ptr(out), None, 0, _train_native.PASS_ONLY,
                                                                        stream_ptr(x.device)), "_transpose_pad")
    return out


def _same_dtype(a: Tensor, b: Tensor) -> None:
    """torch.mm's check, where the reference's backward multiplies two tensors of different dtypes."""
    if a.dtype != b.dtype:
        raise RuntimeError(f"SwitchBackLinear backward: expected mat1 and mat2 to have the same dtype, but got: {a.dtype} != {b.dtype}")


class _SwitchBackFunction(torch.autograd.Function):
    """SwitchBackFunction of the reference: int8 forward, backward on the 16-bit master weight."""

    @staticmethod
    def forward(ctx, input, weight_int8, weight_scales, weight_fp, bias):
        ctx.save_for_backward(input, weight_fp, bias)
        return _switchback_forward(input, weight_int8, weight_scales, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, weight_fp, bias = ctx.saved_tensors
        N, K = weight_fp.shape
        g = grad_output.reshape(-1, grad_output.shape[-1])
        dX = dW = db = None
        if ctx.needs_input_grad[0]:
            _same_dtype(g, weight_fp)
            w = weight_fp if weight_fp.is_contiguous() else weight_fp.contiguous()
            dX = _grad_input(_as(g, w.dtype), _FMT_DENSE, w, None, None, K, K, 0, w.dtype, w.dtype).reshape(input.shape)
        if ctx.needs_input_grad[3]:
            _same_dtype(g, input)
            dW = _linear_grad_weight(g, input.reshape(-1, K))
        if bias is not None and ctx.needs_input_grad[4]:
            db = g.sum(0, dtype=torch.float32).to(g.dtype)
        return dX, None, None, dW, db


def switchback_linear(input: Tensor, weight_int8: Tensor, weight_scales: Tensor, weight_fp: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """SwitchBackLinear's product (reference SwitchBackFunction.apply): the forward on the int8 weight, the gradients on `weight_fp`.
    The same kernels run with or without grad mode, so the output bits do not depend on it."""
    return _SwitchBackFunction.apply(input, weight_int8, weight_scales, weight_fp, bias)


# ============================================================================= INT8 with column + row statistics (LLM.int8 style)
# reference functional.py:896-945, on libmbnb_sparse.so (include/mbnb_sparse.h).  The scale of element [i, j] is sqrt(row_absmax[i] *
# col_absmax[j]); every step of the reference's f32 chain is restated with correctly rounded operations.
def _f32_vector(t: Tensor, n: int, name: str, device) -> Tensor:
    v = _as(t, torch.float32, device).reshape(-1)
    if v.numel() != n:
        raise ValueError(f"{name} has {v.numel()} elements, expected {n}")
    return v


def quantize_colrow(tensor: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """
    Quantize a matrix to INT8 with both row-wise and column-wise statistics (reference: functional.py:896-924): the scale of
    element [i, j] is the geometric mean ``sqrt(row_absmax[i] * col_absmax[j])``.

    Returns (int8 [rows, cols], row_absmax f32 [rows], col_absmax f32 [cols]).  Bit-exact with the reference's chain evaluated with
    a correctly rounded sqrt; a NaN or Inf element makes its row's and column's statistic NaN / Inf and their codes 0.
    """
    if tensor.dim() != 2:
        raise ValueError("Input must be 2D")
    _check_device(tensor, "quantize_colrow")
    t = tensor if tensor.is_contiguous() else tensor.contiguous()
    R, C = t.shape
    dcode = dtype_code(t.dtype, "quantize_colrow")
    q = torch.empty((R, C), dtype=torch.int8, device=t.device)
    rs = torch.empty(R, dtype=torch.float32, device=t.device)
    cs = torch.empty(C, dtype=torch.float32, device=t.device)
    handle = _sparse_native.lib()
    ws_bytes = int(handle.mbnb_colrow_quantize_workspace_bytes(R, C))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=t.device) if ws_bytes > 0 else None
    with on_device(t.device):
        _sparse_native.check(handle.mbnb_colrow_quantize(ptr(t), dcode, R, C, ptr(q), ptr(rs), ptr(cs), ptr(ws), ws_bytes,
                                                         stream_ptr(t.device)), "quantize_colrow")
    return q, rs, cs


def dequantize_colrow(quantized: Tensor, row_scales: Tensor, col_scales: Tensor, dtype: torch.dtype = torch.float16) -> Tensor:
    """Dequantize INT8 with column + row statistics (reference: functional.py:927-932):
    ``(q.float() * (sqrt(row_scales[:, None] * col_scales[None, :]) / 127.0)).to(dtype)``."""
    if quantized.dim() != 2:
        raise ValueError("Input must be 2D")
    _check_device(quantized, "dequantize_colrow")
    q = _as(quantized, torch.int8)
    R, C = q.shape
    rs = _f32_vector(row_scales, R, "row_scales", q.device)
    cs = _f32_vector(col_scales, C, "col_scales", q.device)
    dcode = dtype_code(dtype, "dequantize_colrow")
    out = torch.empty((R, C), dtype=dtype, device=q.device)
    with on_device(q.device):
        _sparse_native.check(_sparse_native.lib().mbnb_colrow_dequantize(ptr(q), ptr(rs), ptr(cs), R, C, dcode, ptr(out), stream_ptr(q.device)),
                             "dequantize_colrow")
    return out


def _matmul_colrow(input: Tensor, weight_int8: Tensor, weight_row_scales: Tensor, weight_col_scales: Tensor, bias: Optional[Tensor],
                   dtype: torch.dtype, flags: int = 0) -> Tensor:
    _check_device(input, "matmul_colrow")
    _check_device(weight_int8, "matmul_colrow")
    if weight_int8.dim() != 2:
        raise ValueError("weight_int8 must be 2D")
    dcode = dtype_code(dtype, "matmul_colrow")
    N, K = weight_int8.shape
    if input.shape[-1] != K:
        raise RuntimeError(f"matmul_colrow: input width {input.shape[-1]} does not match weight {tuple(weight_int8.shape)}")
    x = _as(input.reshape(-1, K), dtype)
    M = x.shape[0]
    w = _as(weight_int8, torch.int8)
    rs = _f32_vector(weight_row_scales, N, "weight_row_scales", x.device)
    cs = _f32_vector(weight_col_scales, K, "weight_col_scales", x.device)
    b = None if bias is None else _as(bias, dtype, x.device)
    if b is not None and b.numel() != N:
        raise ValueError(f"bias has {b.numel()} elements, expected {N}")
    out = torch.empty(M, N, dtype=dtype, device=x.device)
    handle = _sparse_native.lib()
    ws_bytes = int(handle.mbnb_colrow_matmul_workspace_bytes(M, N, K, dcode))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
    with on_device(x.device):
        _sparse_native.check(handle.mbnb_colrow_matmul(ptr(x), dcode, M, K, ptr(w), ptr(rs), ptr(cs), N, ptr(b), ptr(out), ptr(ws), ws_bytes,
                                                       int(flags), stream_ptr(x.device)), "matmul_colrow")
    return out.reshape(*input.shape[:-1], N)


def _colrow_dequant_pass(weight_int8: Tensor, weight_row_scales: Tensor, weight_col_scales: Tensor, dtype: torch.dtype) -> Tensor:
    """matmul_colrow's first pass on its own, as its dense route runs it (write-through stores): Wd [N, K] in `dtype`, the bits its GEMM
    reads.  For tests and tools."""
    _check_device(weight_int8, "_colrow_dequant_pass")
    w = _as(weight_int8, torch.int8)
    N, K = w.shape
    rs = _f32_vector(weight_row_scales, N, "weight_row_scales", w.device)
    cs = _f32_vector(weight_col_scales, K, "weight_col_scales", w.device)
    dcode = dtype_code(dtype, "_colrow_dequant_pass")
    out = torch.empty(N, K, dtype=dtype, device=w.device)
    with on_device(w.device):
        _sparse_native.check(_sparse_native.lib().mbnb_colrow_matmul(None, dcode, 0, K, ptr(w), ptr(rs), ptr(cs), N, None, ptr(out), None, 0,
                                                                     _sparse_native.PASS_ONLY, stream_ptr(w.device)), "_colrow_dequant_pass")
    return out


def matmul_colrow(input: Tensor, weight_int8: Tensor, weight_row_scales: Tensor, weight_col_scales: Tensor,
                  bias: Optional[Tensor] = None, dtype: torch.dtype = torch.float16) -> Tensor:
    """
    ``input[..., K].to(dtype) @ dequantize_colrow(weight_int8[N, K], ..., dtype)^T + bias.to(dtype)`` (reference: functional.py:935-945):
    f32 accumulation and one rounding to `dtype` with the bias inside it, as ``linear_dense``.  Inputs of any leading dims, 1-D included.

    Inference only: the call records no autograd graph (the reference's gradient would flow through torch's F.linear on a weight that
    is rebuilt from the int8 codes on every call; nothing trains through it).
    """
    return _matmul_colrow(input, weight_int8, weight_row_scales, weight_col_scales, bias, dtype)


# ============================================================================= sparse COO (the outlier half of LLM.int8)
# reference functional.py:952-1037 and its native CSR kernels (csrc/mps_bitsandbytes.mm:1598-1650, host :2585-2720), on libmbnb_sparse.so.
_INDEX_BITS = {torch.int64: 64, torch.int32: 32}


def _coo_row_ptr(tensor: Tensor, threshold: float) -> Tuple[Tensor, float, Tensor]:
    """sparse_coo_from_dense's first launch pair: (the contiguous tensor, the threshold as the kernels take it, row_ptr int64 [rows + 1]) --
    the exclusive scan of the per-row counts of kept elements, row_ptr[rows] the total."""
    _check_device(tensor, "sparse_coo_from_dense")
    rows, cols = tensor.shape
    t = tensor if tensor.is_contiguous() else tensor.contiguous()
    dcode = dtype_code(t.dtype, "sparse_coo_from_dense")
    # `tensor.abs() >= threshold` compares in the tensor's dtype: the Python scalar is rounded to it first
    thr = float(torch.tensor(float(threshold), dtype=t.dtype)) if threshold > 0 else 0.0
    row_ptr = torch.empty(rows + 1, dtype=torch.int64, device=t.device)
    with on_device(t.device):
        _sparse_native.check(_sparse_native.lib().mbnb_coo_count(ptr(t), dcode, rows, cols, thr, ptr(row_ptr), stream_ptr(t.device)),
                             "sparse_coo_from_dense")
    return t, thr, row_ptr


def sparse_coo_from_dense(tensor: Tensor, threshold: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, int, int]:
    """
    Convert a dense matrix to COO (reference: functional.py:1005-1020): (row int64 [nnz], col int64 [nnz], values [nnz] in the tensor's
    dtype, rows, cols), entries in row-major order.  With ``threshold > 0`` elements with ``|x| < threshold`` are dropped, compared in
    the tensor's dtype as torch compares them.  -0.0 is dropped, Inf and NaN are kept.

    The size of the result depends on the data: one 8-byte read of the count between the two launches is the op's only host
    synchronisation (what ``torch.nonzero`` does too).
    """
    rows, cols = tensor.shape
    t, thr, row_ptr = _coo_row_ptr(tensor, threshold)
    handle = _sparse_native.lib()
    with on_device(t.device):
        nnz = int(row_ptr[rows].item())
        row = torch.empty(nnz, dtype=torch.int64, device=t.device)
        col = torch.empty(nnz, dtype=torch.int64, device=t.device)
        values = torch.empty(nnz, dtype=t.dtype, device=t.device)
        _sparse_native.check(handle.mbnb_coo_fill(ptr(t), dtype_code(t.dtype, "sparse_coo_from_dense"), rows, cols, thr, ptr(row_ptr), ptr(row),
                                                  ptr(col), ptr(values), nnz, stream_ptr(t.device)), "sparse_coo_from_dense")
    return row, col, values, rows, cols


def quantize_sparse_coo(row_indices: Tensor, col_indices: Tensor, values: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """
    Quantize COO values to INT8 with one absmax scale (reference: functional.py:1023-1037): ``scale = max(|v|).clamp(1e-8) / 127``,
    ``q = clamp(round(v / scale), -127, 127)``.  Returns (row_indices, col_indices, int8 [nnz], scale f32 [1]); the indices are
    returned as given.  The maximum never leaves the device.
    """
    _check_device(values, "quantize_sparse_coo")
    if values.numel() == 0:
        raise RuntimeError("quantize_sparse_coo: values is empty (nnz == 0): the maximum of no elements is undefined")
    v = values if values.is_contiguous() else values.contiguous()
    dcode = dtype_code(v.dtype, "quantize_sparse_coo")
    q = torch.empty(v.shape, dtype=torch.int8, device=v.device)
    scale = torch.empty(1, dtype=torch.float32, device=v.device)
    handle = _sparse_native.lib()
    ws_bytes = int(handle.mbnb_coo_quantize_workspace_bytes())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
    with on_device(v.device):
        _sparse_native.check(handle.mbnb_coo_quantize(ptr(v), dcode, v.numel(), ptr(q), ptr(scale), ptr(ws), ws_bytes, stream_ptr(v.device)),
                             "quantize_sparse_coo")
    return row_indices, col_indices, q, scale


def _spmm_coo(row_indices: Tensor, col_indices: Tensor, values: Tensor, kind: int, scale: Optional[Tensor], dense: Tensor, sparse_rows: int,
              sparse_cols: int, dtype: torch.dtype, what: str, flags: int = 0) -> Tensor:
    """Validation and the call of mbnb_spmm_coo.  `flags`: include/mbnb_sparse.h, for tests."""
    if row_indices.dim() != 1 or col_indices.dim() != 1 or values.dim() != 1:
        raise ValueError(f"{what}: row_indices, col_indices and values must be 1-D")
    nnz = values.numel()
    if row_indices.numel() != nnz or col_indices.numel() != nnz:
        raise ValueError(f"{what}: row_indices ({row_indices.numel()}), col_indices ({col_indices.numel()}) and values ({nnz}) differ in length")
    if row_indices.dtype not in _INDEX_BITS or col_indices.dtype not in _INDEX_BITS:
        raise ValueError(f"{what}: indices must be int64 or int32, got {row_indices.dtype} and {col_indices.dtype}")
    if dense.dim() != 2:
        raise ValueError(f"{what}: dense must be 2-D, got {dense.dim()}-D")
    sparse_rows, sparse_cols = int(sparse_rows), int(sparse_cols)
    if sparse_rows < 0 or sparse_cols < 0:
        raise ValueError(f"{what}: negative sparse shape ({sparse_rows}, {sparse_cols})")
    if dense.shape[0] != sparse_cols:
        raise ValueError(f"{what}: dense has {dense.shape[0]} rows, the sparse matrix {sparse_cols} columns")
    if dense.dtype != dtype:
        raise ValueError(f"{what}: dense is {dense.dtype}, the sparse values are {dtype}")
    _check_device(values, what)
    _check_device(dense, what)
    dev = dense.device
    dcode = dtype_code(dtype, what)
    r = row_indices.to(dev).contiguous()
    c = col_indices.to(dev).contiguous()
    v = values.to(dev).contiguous()
    d = dense if dense.is_contiguous() else dense.contiguous()
    N = d.shape[1]
    out = torch.empty(sparse_rows, N, dtype=dtype, device=dev)
    handle = _sparse_native.lib()
    ws_bytes = int(handle.mbnb_spmm_coo_workspace_bytes(nnz, sparse_rows))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    with on_device(dev):
        _sparse_native.check(handle.mbnb_spmm_coo(ptr(r), _INDEX_BITS[r.dtype], ptr(c), _INDEX_BITS[c.dtype], ptr(v), kind, ptr(scale), nnz, ptr(d),
                                                  dcode, sparse_rows, sparse_cols, N, ptr(out), ptr(ws), ws_bytes, int(flags), stream_ptr(dev)), what)
    return out


def spmm_coo(row_indices: Tensor, col_indices: Tensor, values: Tensor, dense: Tensor, sparse_rows: int, sparse_cols: int) -> Tensor:
    """
    ``sparse @ dense`` with the sparse matrix in COO form (reference: functional.py:952-979; native binding `_C.spmm_coo`): the result
    is [sparse_rows, N] in ``values.dtype``, each element one f32 sum rounded once.  Indices may be int64 or int32, in any order;
    duplicates add.  The same inputs give the same bits on every call.

    Unlike the reference, which raises, an entry whose row or column index is outside the sparse shape is skipped: a bounds check
    that raises would cost a device synchronisation.  Nothing outside any buffer is read or written.
    """
    return _spmm_coo(row_indices, col_indices, values, _sparse_native.COO_VALUES, None, dense, sparse_rows, sparse_cols, values.dtype, "spmm_coo")


def spmm_coo_int8(row_indices: Tensor, col_indices: Tensor, values_int8: Tensor, values_scale: Tensor, dense: Tensor, sparse_rows: int,
                  sparse_cols: int, dtype: torch.dtype = torch.float16) -> Tensor:
    """
    ``spmm_coo`` with INT8 values (reference: functional.py:982-1002; native binding `_C.spmm_coo_int8`): each value is
    ``values_int8.to(dtype) * scale`` with a one-element ``values_scale``, or ``values_int8.to(dtype) * values_scale.to(dtype)`` with one scale
    per entry; ``dense`` is cast to `dtype`.  Out-of-range indices are skipped as in ``spmm_coo``.
    """
    if values_int8.dtype != torch.int8:
        raise ValueError(f"spmm_coo_int8: values_int8 must be int8, got {values_int8.dtype}")
    nnz = values_int8.numel()
    if values_scale.numel() == 1:
        kind = _sparse_native.COO_INT8_SCALAR
    elif values_scale.numel() == nnz:
        kind = _sparse_native.COO_INT8_ENTRY
    else:
        raise ValueError(f"spmm_coo_int8: values_scale has {values_scale.numel()} elements, expected 1 or {nnz}")
    _check_device(dense, "spmm_coo_int8")
    dtype_code(dtype, "spmm_coo_int8")
    scale = _as(values_scale, torch.float32, dense.device).reshape(-1)
    return _spmm_coo(row_indices, col_indices, values_int8, kind, scale, _as(dense, dtype), sparse_rows, sparse_cols, dtype, "spmm_coo_int8")


# ============================================================================= quantized embedding lookups
def embedding_4bit(input: Tensor, weight_packed: Tensor, weight_absmax: Tensor, embedding_dim: int,
                   blocksize: int = 64, quant_type: str = 'nf4', padding_idx: Optional[int] = None,
                   dtype: torch.dtype = torch.float16) -> Tensor:
    """
    Gather + dequantize rows of a 4-bit embedding table in one kernel: the forward of Embedding4bit
    (reference: nn/embedding.py:83-138; native bindings `_C.embedding_4bit_nf4/_fp4`, mm:2309-2388).
    `weight_packed` u8 [num, dim/2], `weight_absmax` f32 [num, ceil(dim/blocksize)]; returns
    ``input.shape + [embedding_dim]`` in `dtype`, rows equal to `padding_idx` zeroed.  Bit-exact against the
    reference's Python path.  Indices are not range-checked on the host (no device synchronisation);
    out-of-range rows come back as zeros.
    """
    _check_device(weight_packed, "embedding_4bit")
    if quant_type not in _native.QUANT_CODE:
        raise ValueError(f"quant_type must be 'nf4' or 'fp4', got {quant_type}")
    dev = weight_packed.device
    idx = input.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    num = weight_packed.shape[0]
    out = torch.empty(idx.numel(), embedding_dim, dtype=dtype, device=dev)
    wp = weight_packed.contiguous()
    wa = weight_absmax.to(device=dev, dtype=torch.float32).contiguous()
    with on_device(dev):
        check(_native.lib().mbnb_embedding_4bit(ptr(idx), idx.numel(), ptr(wp), ptr(wa), num, int(embedding_dim),
                                                int(blocksize), _native.QUANT_CODE[quant_type], int(padding_idx is not None),
                                                int(padding_idx) if padding_idx is not None else 0,
                                                dtype_code(dtype, "embedding_4bit"), ptr(out), stream_ptr(dev)),
              "embedding_4bit")
    return out.reshape(*input.shape, embedding_dim)


def embedding_8bit(input: Tensor, weight_int8: Tensor, weight_scales: Tensor, padding_idx: Optional[int] = None,
                   dtype: torch.dtype = torch.float16) -> Tensor:
    """
    Gather + dequantize rows of an int8 embedding table: the forward of Embedding8bit
    (reference: nn/embedding.py:255-268; native binding `_C.embedding_8bit`, mm:2390-2427).  Bit-exact against the
    reference's Python path: ``q.to(dtype) * (scale / 127.0).to(dtype)``.
    """
    _check_device(weight_int8, "embedding_8bit")
    dev = weight_int8.device
    idx = input.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    num, dim = weight_int8.shape
    out = torch.empty(idx.numel(), dim, dtype=dtype, device=dev)
    w = weight_int8.contiguous()
    s = weight_scales.to(device=dev, dtype=torch.float32).contiguous()
    with on_device(dev):
        check(_native.lib().mbnb_embedding_8bit(ptr(idx), idx.numel(), ptr(w), ptr(s), num, dim,
                                                int(padding_idx is not None),
                                                int(padding_idx) if padding_idx is not None else 0,
                                                dtype_code(dtype, "embedding_8bit"), ptr(out), stream_ptr(dev)),
              "embedding_8bit")
    return out.reshape(*input.shape, dim)


# ============================================================================= outlier-aware INT8 linear
def outlier_linear(input: Tensor, weight_int8: Tensor, weight_scales: Tensor, outlier_indices: Tensor,
                   outlier_weights: Tensor, bias: Optional[Tensor] = None,
                   dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    The forward of OutlierAwareLinear (reference: nn/outlier_aware.py:84-146): row-wise INT8 quantisation of the
    non-outlier input columns, int8 x int8 contraction on the MFMA, the outlier columns in `dtype`, bias.
    The reference multiplies dtype-rounded dequantised operands; the exact integer contraction used here differs
    from it by <= 4e-4 (fp16) / 1.3e-3 (bf16) relative (Frobenius).
    An entry of `outlier_indices` outside ``[0, in_features)`` is not range-checked on the host (no device
    synchronisation): on every path it masks no column and its column of `outlier_weights` contributes zero.
    """
    _check_device(input, "outlier_linear")
    _check_device(weight_int8, "outlier_linear")
    if dtype is None:
        dtype = input.dtype
    dcode = dtype_code(dtype, "outlier_linear")
    N, K = weight_int8.shape
    if input.shape[-1] != K:
        raise RuntimeError(f"outlier_linear: input width {input.shape[-1]} does not match weight {tuple(weight_int8.shape)}")
    dev = input.device
    x = input.reshape(-1, K).to(dtype).contiguous()
    M = x.shape[0]
    w = weight_int8.contiguous()
    s = weight_scales.to(device=dev, dtype=torch.float32).contiguous()
    n_out = int(outlier_indices.numel())
    oi = outlier_indices.to(device=dev, dtype=torch.int64).contiguous() if n_out else None
    ow = outlier_weights.to(device=dev, dtype=dtype).contiguous() if n_out else None
    b = None if bias is None else bias.to(device=dev, dtype=dtype).contiguous()
    out = torch.empty(M, N, dtype=dtype, device=dev)
    ws_bytes = int(_native.lib().mbnb_outlier_linear_workspace_bytes(M, K, n_out))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with on_device(dev):
        check(_native.lib().mbnb_outlier_linear(ptr(x), dcode, M, K, ptr(w), ptr(s), N, ptr(oi), n_out, ptr(ow), ptr(b),
                                                   ptr(out), ptr(ws), ws_bytes, stream_ptr(dev)), "outlier_linear")
    return out.reshape(*input.shape[:-1], N)


# ============================================================================= double quant (LLM.int8 stats)
def double_quant(
    A: Tensor,
    col_stats: Optional[Tensor] = None,
    row_stats: Optional[Tensor] = None,
    out_col: Optional[Tensor] = None,
    out_row: Optional[Tensor] = None,
    threshold: float = 0.0,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """
    Row- and column-wise INT8 quantization with their absmax statistics
    (reference: functional.py:814-863, bit-exact).  Returns
    (col_quantized, row_quantized, col_stats, row_stats, None); `threshold` is ignored as in the
    reference, and caller-supplied out_col / out_row are returned untouched as there.
    """
    if A.dim() != 2:
        raise ValueError("Input must be 2D")
    _check_device(A, "double_quant")
    A = A.contiguous()
    rows, cols = A.shape
    dcode = dtype_code(A.dtype, "double_quant")
    cs = (torch.empty(cols, dtype=torch.float32, device=A.device) if col_stats is None
          else col_stats.to(device=A.device, dtype=torch.float32).contiguous().clone())
    rs = (torch.empty(rows, dtype=torch.float32, device=A.device) if row_stats is None
          else row_stats.to(device=A.device, dtype=torch.float32).contiguous().clone())
    oc = torch.empty(A.shape, dtype=torch.int8, device=A.device)
    orow = torch.empty(A.shape, dtype=torch.int8, device=A.device)
    with on_device(A.device):
        check(_native.lib().mbnb_double_quant(
            ptr(A), dcode, rows, cols, ptr(oc), ptr(orow), ptr(cs), ptr(rs), int(col_stats is not None),
            int(row_stats is not None), stream_ptr(A.device)), "double_quant")
    return (oc if out_col is None else out_col, orow if out_row is None else out_row,
            cs if col_stats is None else col_stats, rs if row_stats is None else row_stats, None)


def dequant_absmax(absmax_quant: Tensor, absmax_scales, blocksize: int = 256) -> Tensor:
    """Dequantize double-quantized absmax values (reference: functional.py:866-889).

    `absmax_scales` a QuantState: dequantize_blockwise (the live form, functional.py:870-871).  Otherwise the legacy
    form (functional.py:873-889): codes [rows, num_blocks] (or 1-D) with one scale per `blocksize` codes of a row;
    returns f32 ``codes.float() * scale``, zero where no scale block covers a code (the reference's zeros_like)."""
    if isinstance(absmax_scales, QuantState):
        return dequantize_blockwise(absmax_quant, absmax_scales)
    _check_device(absmax_quant, "dequant_absmax")
    q = absmax_quant.contiguous()
    rows = q.shape[0] if q.dim() > 1 else 1
    num_blocks = q.numel() // rows if rows > 0 else q.numel()
    scales = absmax_scales.to(device=q.device, dtype=torch.float32).contiguous()
    dq_blocks = scales.numel() // rows if rows > 0 else scales.numel()
    if blocksize <= 0:
        raise ValueError(f"blocksize must be positive, got {blocksize}")
    kind = 0 if q.dtype == torch.int8 else 1 if q.dtype == torch.uint8 else 2
    if kind == 2 and q.dtype != torch.float32:
        q = q.float()       # the reference's `.float()` of the codes
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    with on_device(q.device):
        check(_native.lib().mbnb_dequant_absmax(ptr(q), kind, rows, num_blocks, ptr(scales), dq_blocks, int(blocksize),
                                                ptr(out), stream_ptr(q.device)), "dequant_absmax")
    return out


# ============================================================================= OCP MX (MXFP4 weights, MXFP4 / MXFP8 activations)
# No counterpart in the reference: its FP4 table is not E2M1 and its scales are f32.  The format is DESIGN.md §25 and
# include/mbnb_mx.h: codes plus one E8M0 scale byte per 32 consecutive k, both row-major, so the tensors are the ones other MX
# tools read and write.  The linear runs gfx950's block-scaled MFMA over them as they lie in memory (libmbnb_mx.so).
def _mx_elem(elem: str, what: str) -> int:
    try:
        return _mx_native.ELEM_CODE[elem]
    except (KeyError, TypeError):
        raise ValueError(f"{what}: unknown MX element format {elem!r} (supported: 'fp4', 'fp8')") from None


def _mx_width(K: int, what: str) -> None:
    if K <= 0 or K % _mx_native.BLOCK:
        raise ValueError(f"{what}: the last dimension ({K}) must be a positive multiple of the MX block, {_mx_native.BLOCK}")


def _aligned16(t: Tensor) -> Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def quantize_mx(tensor: Tensor, elem: str = "fp4") -> Tuple[Tensor, Tensor]:
    """
    Quantise a 2-D tensor [rows, K] (K % 32 == 0) to OCP MX: returns (codes, scales) with `scales` uint8 [rows, K / 32]
    (E8M0, 0xFF = NaN block) and `codes` uint8 [rows, K / 2] for elem "fp4" (E2M1, even k in the low nibble) or
    [rows, K] for "fp8" (E4M3).  The rule is DESIGN.md §25.
    """
    code = _mx_elem(elem, "quantize_mx")
    _check_device(tensor, "quantize_mx")
    if tensor.dim() != 2:
        raise ValueError("quantize_mx: input must be 2D")
    rows, K = tensor.shape
    _mx_width(K, "quantize_mx")
    x = _aligned16(tensor if tensor.dtype in _native.DTYPE_CODE else tensor.float())
    codes = torch.empty(rows, K // 2 if code == _mx_native.FP4 else K, dtype=torch.uint8, device=x.device)
    scales = torch.empty(rows, K // _mx_native.BLOCK, dtype=torch.uint8, device=x.device)
    with on_device(x.device):
        _mx_native.check(_mx_native.lib().mbnb_mx_quantize(ptr(x), rows, K, dtype_code(x.dtype, "quantize_mx"), code, ptr(codes),
                                                           ptr(scales), stream_ptr(x.device)), "quantize_mx")
    return codes, scales


def dequantize_mx(codes: Tensor, scales: Tensor, elem: str = "fp4", dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """value(code) * 2^(scale byte - 127), formed exactly and rounded once to `dtype`; a 0xFF scale byte gives a NaN block."""
    code = _mx_elem(elem, "dequantize_mx")
    _check_device(codes, "dequantize_mx")
    if codes.dim() != 2 or scales.dim() != 2 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError("dequantize_mx: codes and scales must be 2D uint8 tensors")
    rows = codes.shape[0]
    K = codes.shape[1] * 2 if code == _mx_native.FP4 else codes.shape[1]
    _mx_width(K, "dequantize_mx")
    if tuple(scales.shape) != (rows, K // _mx_native.BLOCK):
        raise ValueError(f"dequantize_mx: scales {tuple(scales.shape)} do not match codes {tuple(codes.shape)}: expected {(rows, K // _mx_native.BLOCK)}")
    q = _aligned16(codes)
    s = scales.to(q.device).contiguous()
    out = torch.empty(rows, K, dtype=dtype, device=q.device)
    with on_device(q.device):
        _mx_native.check(_mx_native.lib().mbnb_mx_dequantize(ptr(q), ptr(s), rows, K, code, dtype_code(dtype, "dequantize_mx"), ptr(out),
                                                             stream_ptr(q.device)), "dequantize_mx")
    return out


def quantize_mxfp4(tensor: Tensor) -> Tuple[Tensor, Tensor]:
    """``quantize_mx(tensor, "fp4")``"""
    return quantize_mx(tensor, "fp4")


def dequantize_mxfp4(codes: Tensor, scales: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """``dequantize_mx(codes, scales, "fp4", dtype)``"""
    return dequantize_mx(codes, scales, "fp4", dtype)


def matmul_mxfp4(input: Tensor, weight: Tensor, weight_scales: Tensor, bias: Optional[Tensor] = None, act_format: str = "fp8",
                 dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    ``Q(input[..., K]) @ W^T + bias`` with W the MXFP4 weight (`weight` uint8 [N, K / 2], `weight_scales` uint8 [N, K / 32]) and Q
    the MX quantiser of the activation rows to `act_format` ("fp8": E4M3, "fp4": E2M1).  Two launches: the quantiser into a
    workspace, then the block-scaled MFMA GEMM: f32 accumulation, the bias added in f32, one rounding to `dtype` (default: the
    input's).  Inference only: no gradient is defined.

    ``act_format="none"`` is the weight-only form for decode steps: the activation is NOT quantised, it stays in
    its own dtype, and one launch of `k_mx_decode` streams the codes and scale bytes once and decodes them in registers (no
    workspace; f32 accumulation with the scale applied per block, the bias added in f32, one rounding).  Any number of rows
    takes that launch, with one exception: bf16 in and out (and bias) with more than 16 rows, ``K % 64 == 0`` and ``K >= 128`` run the
    composed form ``linear_dense(x, dequantize_mx(w, s, "fp4", torch.bfloat16), bias)``, i.e. a dequantise launch (exact in
    bf16 for every scale byte) and the dense bf16 GEMM.  The two routes differ in summation order only.
    """
    if torch.is_grad_enabled() and (input.requires_grad or (bias is not None and bias.requires_grad)):
        raise NotImplementedError("matmul_mxfp4 is inference-only: it defines no gradient for its input or bias "
                                  "(call it under torch.no_grad(), or detach them)")
    weight_only = isinstance(act_format, str) and act_format == "none"
    act = None if weight_only else _mx_elem(act_format, "matmul_mxfp4")
    _check_device(input, "matmul_mxfp4")
    _check_device(weight, "matmul_mxfp4")
    if weight.dim() != 2 or weight_scales.dim() != 2 or weight.dtype != torch.uint8 or weight_scales.dtype != torch.uint8:
        raise ValueError("matmul_mxfp4: weight and weight_scales must be 2D uint8 tensors")
    N, K = weight.shape[0], weight.shape[1] * 2
    _mx_width(K, "matmul_mxfp4")
    if tuple(weight_scales.shape) != (N, K // _mx_native.BLOCK):
        raise ValueError(f"matmul_mxfp4: weight_scales {tuple(weight_scales.shape)} do not match weight {tuple(weight.shape)}: "
                         f"expected {(N, K // _mx_native.BLOCK)}")
    out_dtype = input.dtype if dtype is None else dtype
    ocode = dtype_code(out_dtype, "matmul_mxfp4")
    is_1d = input.dim() == 1
    x = input.unsqueeze(0) if is_1d else input
    if x.shape[-1] != K:
        raise ValueError(f"matmul_mxfp4: input width {x.shape[-1]} does not match weight {tuple(weight.shape)} (K = {K})")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K)
    x2 = _aligned16(x2 if x2.dtype in _native.DTYPE_CODE else x2.float())
    M = x2.shape[0]
    w = _aligned16(weight)
    s = weight_scales.to(x2.device).contiguous()
    b = None if bias is None else bias.to(x2.device).contiguous()
    if b is not None and (b.dim() != 1 or b.shape[0] != N):
        raise ValueError(f"matmul_mxfp4: bias {tuple(b.shape)} does not match N = {N}")
    if b is not None and b.dtype not in _native.DTYPE_CODE:
        b = b.float()
    if (weight_only and M > _mx_native.DECODE_ROWS and x2.dtype == torch.bfloat16 and out_dtype == torch.bfloat16
            and K % 64 == 0 and K >= 128 and (b is None or b.dtype == torch.bfloat16)):
        # prefill-sized bf16 calls: dequantise (exact in bf16) + the dense GEMM; the same sum in another order
        out = linear_dense(x2, dequantize_mx(w, s, "fp4", torch.bfloat16), b)
        out = out.reshape(*lead, N)
        return out.squeeze(0) if is_1d else out
    out = torch.empty(M, N, dtype=out_dtype, device=x2.device)
    if M > 0 and weight_only:
        with on_device(x2.device):
            _mx_native.check(_mx_native.lib().mbnb_mx_linear_weight_only(
                ptr(x2), M, K, dtype_code(x2.dtype, "matmul_mxfp4"), ptr(w), ptr(s), N, ptr(b),
                0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out), ocode, stream_ptr(x2.device)), "matmul_mxfp4")
    elif M > 0:
        ws_bytes = _mx_native.workspace_bytes(M, K, act)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x2.device)
        with on_device(x2.device):
            _mx_native.check(_mx_native.lib().mbnb_mx_linear(
                ptr(x2), M, K, dtype_code(x2.dtype, "matmul_mxfp4"), ptr(w), ptr(s), N, act, ptr(b),
                0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out), ocode, ptr(ws), ws_bytes, stream_ptr(x2.device)), "matmul_mxfp4")
    out = out.reshape(*lead, N)
    return out.squeeze(0) if is_1d else out


# ============================================================================= MXFP4 expert linears (mixture of experts)
# The tensors MXFP4 checkpoints ship are expert weights: [E, N, K / 32, 16] blocks plus [E, N, K / 32] scale bytes, and a router
# picks `top_k` of the E experts per token.  One launch of libmbnb_moe.so serves a projection of every (token, slot) pair, the
# expert ids read on the device.  _expert_operands is the one check and preparation of an expert projection's
# operands, for this call and for the two of the MLP below.
def _expert_operands(what: str, native, input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, bias: Optional[Tensor],
                     per_slot: Optional[bool], dtype: Optional[torch.dtype], routing_weights: Optional[Tensor] = None):
    """The checks and the operand preparation of one expert projection -> (x, w, s, ids, b, rw, T, A, E, N, K, out dtype, its code).
    `native` is the binding whose library serves the call: its BLOCK and MAX_PAIRS hold, and its MAX_EXPERTS where it has one.
    `per_slot`: the input is [T, A, K] (True), [T, K] (False), or either (None)."""
    grads = (input, bias, routing_weights)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in grads):
        raise NotImplementedError(f"{what} is inference-only: it defines no gradient for its "
                                  f"{'input or bias' if routing_weights is None else 'input, bias or routing weights'} "
                                  "(call it under torch.no_grad(), or detach them)")
    if weight.dtype != torch.uint8 or weight_scales.dtype != torch.uint8 or weight.dim() not in (3, 4) or weight_scales.dim() != 3:
        raise ValueError(f"{what}: weight must be a uint8 tensor [E, N, K / 2] or [E, N, K / 32, 16] and weight_scales uint8 [E, N, K / 32]")
    if weight.dim() == 4:
        if weight.shape[3] != native.BLOCK // 2:
            raise ValueError(f"{what}: a 4-D weight is the blocks layout [E, N, K / 32, 16], got {tuple(weight.shape)}")
        weight = weight.reshape(weight.shape[0], weight.shape[1], -1)
    E, N, K = weight.shape[0], weight.shape[1], weight.shape[2] * 2
    _mx_width(K, what)
    if E <= 0 or N <= 0:
        raise ValueError(f"{what}: weight {tuple(weight.shape)} has no expert or no output feature")
    if E > getattr(native, "MAX_EXPERTS", E):
        raise ValueError(f"{what}: {E} experts exceed the {native.MAX_EXPERTS} of one launch")
    if tuple(weight_scales.shape) != (E, N, K // native.BLOCK):
        raise ValueError(f"{what}: weight_scales {tuple(weight_scales.shape)} do not match weight {tuple(weight.shape)}: "
                         f"expected {(E, N, K // native.BLOCK)}")
    if expert_ids.dim() != 2 or expert_ids.dtype.is_floating_point or expert_ids.dtype.is_complex or expert_ids.dtype == torch.bool:
        raise ValueError(f"{what}: expert_ids must be an integer tensor [T, A], got {expert_ids.dtype} {tuple(expert_ids.shape)}")
    T, A = expert_ids.shape
    if per_slot is None:
        if input.dim() not in (2, 3):
            raise ValueError(f"{what}: input must be [T, K] (shared by a token's slots) or [T, A, K] (a row per slot), got {tuple(input.shape)}")
        per_slot = input.dim() == 3
    want = (T, A, K) if per_slot else (T, K)
    if tuple(input.shape) != want:
        raise ValueError(f"{what}: input {tuple(input.shape)} does not match expert_ids {tuple(expert_ids.shape)} and K = {K}: "
                         f"expected {'[T, A, K]' if per_slot else '[T, K]'} = {want}")
    if input.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{what}: input must be float16 or bfloat16 (16-bit activations), got {input.dtype}")
    if bias is not None and tuple(bias.shape) != (E, N):
        raise ValueError(f"{what}: bias {tuple(bias.shape)} does not match [E, N] = {(E, N)}")
    if routing_weights is not None and (tuple(routing_weights.shape) != (T, A) or not routing_weights.dtype.is_floating_point):
        raise ValueError(f"{what}: routing_weights must be a floating-point tensor [T, A] = {(T, A)}, got {routing_weights.dtype} "
                         f"{tuple(routing_weights.shape)}")
    if A > native.MAX_PAIRS:
        raise ValueError(f"{what}: {A} slots per token exceed the {native.MAX_PAIRS} pairs of one launch")
    out_dtype = input.dtype if dtype is None else dtype
    ocode = dtype_code(out_dtype, what)
    for t in (input, weight, expert_ids):
        _check_device(t, what)
    x = _aligned16(input)
    w = _aligned16(weight)
    s = weight_scales.to(x.device).contiguous()
    ids = expert_ids.to(x.device)
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        ids = ids.to(torch.int32).contiguous()
    b = None if bias is None else bias.to(x.device).contiguous()
    if b is not None and b.dtype not in _native.DTYPE_CODE:
        b = b.float()
    rw = None if routing_weights is None else routing_weights.to(x.device)
    if rw is not None and (rw.dtype not in _native.DTYPE_CODE or not rw.is_contiguous()):
        rw = (rw if rw.dtype in _native.DTYPE_CODE else rw.float()).contiguous()
    return x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode


def matmul_mxfp4_experts(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, bias: Optional[Tensor] = None,
                         dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    ``out[t, a] = input_row(t, a) @ W[expert_ids[t, a]]^T + bias[expert_ids[t, a]]`` -> ``[T, A, N]``, over E MXFP4 weights:
    `weight` uint8 [E, N, K / 2] (or the checkpoint's blocks layout [E, N, K / 32, 16], the same bytes), `weight_scales` uint8
    [E, N, K / 32], `bias` [E, N] or None, `expert_ids` an integer tensor [T, A].  `input` is [T, K] (every slot of a token shares
    its row: a gate / up projection) or [T, A, K] (a row per slot: a down projection), f16 or bf16, not quantised.

    One launch of `k_mx_experts` for up to 1024 pairs (more are cut over the tokens into several launches): the ids are read on
    the device, so nothing synchronises and a captured graph serves a new routing once `expert_ids` is overwritten in place (an
    int32 contiguous `expert_ids` is passed as the caller's own tensor; other integer dtypes are converted).  f32 accumulation,
    the scale applied per block, the bias added in f32, one rounding to `dtype` (default: the input's); a pair's bits are those
    of ``matmul_mxfp4(row, W[e], s[e], bias[e], act_format="none")`` on 2 to 16 rows, whatever else is in the call.  A pair whose
    id is outside [0, E) (-1 pads) gets a row of +0.0.  Inference only: no gradient is defined.  The routed sum over the slots and
    the activation between two projections stay torch ops of the caller.  From `MOE_GROUPED_MIN_PAIRS` pairs up the call takes the
    grouped GEMM of `matmul_mxfp4_experts_grouped`: the same bits, another `last_launch()`.
    """
    what = "matmul_mxfp4_experts"
    x, w, s, ids, b, _, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moe_native, input, weight, weight_scales, expert_ids, bias, None,
                                                                          dtype)
    per_slot = x.dim() == 3
    if _takes_grouped(T * A, E):
        return _grouped_experts(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, None)
    out = torch.empty(T, A, N, dtype=out_dtype, device=x.device)
    if T * A == 0:
        return out
    step = max(1, _moe_native.MAX_PAIRS // A)                # tokens per launch
    fn = _moe_native.lib().mbnb_moe_mxfp4_experts
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            _moe_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, int(per_slot), K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, N,
                                 ptr(ids[t0:t1]), ptr(b), 0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out[t0:t1]), ocode, stream), what)
    return out


# ============================================================================= the MXFP4 mixture-of-experts MLP
# libmbnb_moemlp.so: the gate / up launch with the gated activation as its epilogue, the down launch into an f32
# workspace and the routed sum over a token's slots, the two expert launches on a grid sized by the routing.  Ids and routing
# weights are read on the device.
def matmul_mxfp4_experts_glu(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, bias: Optional[Tensor] = None,
                             alpha: float = 1.702, limit: float = 7.0, dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    The gate / up projection of a mixture-of-experts MLP with the gated activation as its epilogue -> ``[T, A, I]``.  `weight` uint8
    [E, 2I, K / 2] (or the blocks layout [E, 2I, K / 32, 16]) with the checkpoint's interleaved rows, row 2j gate j and row 2j + 1 up
    j; `weight_scales` uint8 [E, 2I, K / 32]; `bias` [E, 2I] or None, interleaved the same way; `input` [T, K], f16 or bf16, shared
    by a token's slots; `expert_ids` an integer tensor [T, A].  With ``pre = matmul_mxfp4_experts(..., dtype=float32)`` (the same bits),

        g = min(pre[..., 2j], limit);  u = clamp(pre[..., 2j + 1], -limit, limit)
        out[..., j] = (u + 1) * (g * (1 / (1 + exp(-alpha * g))))

    in f32, one rounding to `dtype` (default: the input's).  One launch for up to 1024 pairs (more are cut over the tokens) on a
    grid of ceil(2I / 16) x min(E, pairs) workgroups; the ids are read on the device, so nothing synchronises (an int32 contiguous
    `expert_ids` is passed as the caller's own tensor).  A pair whose id is outside [0, E) (-1 pads) gets a row of +0.0.  At most
    1024 experts.  `limit` may be ``inf``.  Inference only: no gradient is defined.  From `MOE_GROUPED_MIN_PAIRS` pairs up the call
    takes the grouped GEMM of `matmul_mxfp4_experts_grouped_glu`: the same bits, another `last_launch()`.
    """
    what = "matmul_mxfp4_experts_glu"
    alpha, limit = float(alpha), float(limit)
    if not math.isfinite(alpha) or not limit > 0:
        raise ValueError(f"{what}: alpha ({alpha}) must be finite and limit ({limit}) positive (inf: no clamp)")
    if weight.dim() in (3, 4) and weight.shape[1] % 2:
        raise ValueError(f"{what}: weight {tuple(weight.shape)} has {weight.shape[1]} rows: the interleaved gate / up rows come in pairs")
    x, w, s, ids, b, _, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moemlp_native, input, weight, weight_scales, expert_ids, bias, False, dtype)
    I = N // 2
    if _takes_grouped(T * A, E):
        return _grouped_glu(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, alpha, limit, None)
    out = torch.empty(T, A, I, dtype=out_dtype, device=x.device)
    if T * A == 0:
        return out
    step = max(1, _moemlp_native.MAX_PAIRS // A)             # tokens per launch
    fn = _moemlp_native.lib().mbnb_moemlp_gate_up_glu
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            _moemlp_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, I, ptr(ids[t0:t1]), ptr(b),
                                    0 if b is None else _native.DTYPE_CODE[b.dtype], alpha, limit, ptr(out[t0:t1]), ocode, stream), what)
    return out


def matmul_mxfp4_experts_sum(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, routing_weights: Tensor,
                             bias: Optional[Tensor] = None, dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    The down projection of a mixture-of-experts MLP and the routed, weighted sum over a token's slots -> ``[T, N]``:
    ``out[t] = sum_a routing_weights[t, a] * (input[t, a] @ W[expert_ids[t, a]]^T + bias[expert_ids[t, a]])``.  `input` [T, A, K],
    f16 or bf16; `weight` uint8 [E, N, K / 2] (or the blocks layout), `weight_scales` uint8 [E, N, K / 32], `bias` [E, N] or None;
    `routing_weights` [T, A], f32, f16 or bf16, read as f32.

    Two launches for up to 1024 pairs (more are cut over the tokens): the projection in f32, with the bits of
    ``matmul_mxfp4_experts(..., dtype=float32)``, into a workspace that is a ``torch.empty`` of this call, then one thread per output
    runs ``acc = fmaf(rw[t, a], y[t, a, n], acc)`` over the slots in their order from +0.0 and rounds once to `dtype` (default: the
    input's).  A slot whose id is outside [0, E) is skipped, its routing weight unread; a token without a slot in range gets +0.0.
    Ids and routing weights are read on the device (contiguous tensors of a supported dtype are passed as the caller's own), so a
    captured graph serves a new routing once both are overwritten in place.  At most 1024 experts.  Inference only.  From
    `MOE_GROUPED_MIN_PAIRS` pairs up the call takes the grouped GEMM of `matmul_mxfp4_experts_grouped_sum`: the same bits.
    """
    what = "matmul_mxfp4_experts_sum"
    x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moemlp_native, input, weight, weight_scales, expert_ids, bias, True, dtype,
                                                                           routing_weights)
    if T * A == 0:
        return torch.zeros(T, N, dtype=out_dtype, device=x.device)
    if _takes_grouped(T * A, E):
        return _grouped_sum(what, x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode, None)
    out = torch.empty(T, N, dtype=out_dtype, device=x.device)
    step = max(1, _moemlp_native.MAX_PAIRS // A)             # tokens per call
    ws_bytes = _moemlp_native.workspace_bytes(min(T, step), A, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    fn = _moemlp_native.lib().mbnb_moemlp_down_sum
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            _moemlp_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, N, ptr(ids[t0:t1]), ptr(b),
                                    0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(rw[t0:t1]), _native.DTYPE_CODE[rw.dtype],
                                    ptr(out[t0:t1]), ocode, ptr(ws), ws_bytes, stream), what)
    return out


def moe_mlp_mxfp4(input: Tensor, gate_up_weight: Tensor, gate_up_scales: Tensor, gate_up_bias: Optional[Tensor], down_weight: Tensor,
                  down_scales: Tensor, down_bias: Optional[Tensor], expert_ids: Tensor, routing_weights: Tensor, alpha: float = 1.702,
                  limit: float = 7.0, dtype: Optional[torch.dtype] = None) -> Tensor:
    """
    The expert MLP of a mixture-of-experts block (gpt-oss) for the tokens `input` [T, H] -> ``[T, H']``:
    ``matmul_mxfp4_experts_sum(matmul_mxfp4_experts_glu(input, gate_up..., expert_ids, alpha, limit), down..., expert_ids,
    routing_weights, dtype=dtype)`` and nothing more: three launches, the intermediate [T, A, I] in the input's dtype.  The router
    (`expert_ids`, `routing_weights`) stays the caller's.
    From `MOE_GROUPED_MIN_PAIRS` pairs up both projections run on the grouped GEMM and
    share one plan of the routing per cut of `MOE_GROUPED_MAX_PAIRS` pairs: the same bits.
    """
    if (expert_ids.dim() == 2 and expert_ids.is_cuda and not expert_ids.dtype.is_floating_point and gate_up_weight.dim() in (3, 4)
            and down_weight.dim() in (3, 4) and gate_up_weight.shape[0] == down_weight.shape[0]
            and _takes_grouped(expert_ids.numel(), gate_up_weight.shape[0])):
        # the prefill route: one plan per cut over the tokens serves both projections
        ids, plan = moe_grouped_plan(expert_ids, gate_up_weight.shape[0])
        h = matmul_mxfp4_experts_grouped_glu(input, gate_up_weight, gate_up_scales, ids, gate_up_bias, alpha, limit, plan=plan)
        return matmul_mxfp4_experts_grouped_sum(h, down_weight, down_scales, ids, routing_weights, down_bias, dtype, plan=plan)
    h = matmul_mxfp4_experts_glu(input, gate_up_weight, gate_up_scales, expert_ids, gate_up_bias, alpha, limit)
    return matmul_mxfp4_experts_sum(h, down_weight, down_scales, expert_ids, routing_weights, down_bias, dtype)


# ============================================================================= the prefill-sized grouped GEMM over MXFP4 experts
# libmbnb_moegemm.so: a plan of the routing built on the device (counts, a stable list of the pairs grouped by
# expert, a tile table), then one launch per projection for any number of pairs: a workgroup takes 64 listed pairs of one expert
# against one decode of its weight tile.  A pair's bits are those of the decode launches above, so the three functions of §28 /
# §29 take this route from MOE_GROUPED_MIN_PAIRS pairs up and only their speed and last_launch() change.
MOE_GROUPED_MAX_PAIRS = 16384      # pairs of one call: the f32 workspace and the intermediate stay below ~200 MB each at N = 2880
# The automatic route: matmul_mxfp4_experts, _glu and _sum (and so moe_mlp_mxfp4, moe_block_mxfp4 and the modules) take the grouped GEMM
# from this many pairs up; None: never.  Measured (profiles/moegemm_bench.jsonl): at 2048 pairs the grouped route takes
# 0.43x (E = 32) and 0.62x (E = 128) of the decode route's time; at 1024 pairs 0.62x and 1.19x, so 2048 is the smallest measured count
# from which it wins at both.
MOE_GROUPED_MIN_PAIRS: Optional[int] = 2048


def _takes_grouped(pairs: int, E: int) -> bool:
    return MOE_GROUPED_MIN_PAIRS is not None and pairs >= max(1, MOE_GROUPED_MIN_PAIRS) and E <= _moegemm_native.MAX_EXPERTS


def _grouped_cuts(T: int, A: int):
    step = max(1, MOE_GROUPED_MAX_PAIRS // max(1, A))        # tokens per call
    return [(t0, min(T, t0 + step)) for t0 in range(0, T, step)]


def moe_grouped_plan(expert_ids: Tensor, num_experts: int):
    """
    The plans of the grouped expert GEMM for `expert_ids` (an integer cuda tensor [T, A]) over `num_experts` experts ->
    ``(ids, plans)``: the ids as the int32 contiguous tensor the launches read (the caller's own when it is one already) and one
    plan per cut of at most `MOE_GROUPED_MAX_PAIRS` pairs over the tokens, built on the device in two small launches each.  Pass
    both on, as `expert_ids` and `plan=`, to the projections that share the routing.  A plan holds the routing it was built from:
    after `expert_ids` changes in place, build it again.
    """
    what = "moe_grouped_plan"
    if expert_ids.dim() != 2 or expert_ids.dtype.is_floating_point or expert_ids.dtype.is_complex or expert_ids.dtype == torch.bool:
        raise ValueError(f"{what}: expert_ids must be an integer tensor [T, A], got {expert_ids.dtype} {tuple(expert_ids.shape)}")
    E = int(num_experts)
    if not 0 < E <= _moegemm_native.MAX_EXPERTS:
        raise ValueError(f"{what}: {E} experts, between 1 and {_moegemm_native.MAX_EXPERTS}")
    _check_device(expert_ids, what)
    T, A = expert_ids.shape
    if A > _moegemm_native.MAX_PAIRS:
        raise ValueError(f"{what}: {A} slots per token exceed the {_moegemm_native.MAX_PAIRS} pairs of one launch")
    ids = expert_ids
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        ids = ids.to(torch.int32).contiguous()
    return ids, _grouped_plans(what, ids, T, A, E)


def _grouped_plans(what: str, ids: Tensor, T: int, A: int, E: int):
    plans = []
    fn = _moegemm_native.lib().mbnb_moegemm_plan
    with on_device(ids.device):
        stream = stream_ptr(ids.device)
        for t0, t1 in _grouped_cuts(T, A):
            nbytes = _moegemm_native.plan_bytes((t1 - t0) * A, E)
            plan = torch.empty(nbytes, dtype=torch.uint8, device=ids.device)
            if (t1 - t0) * A:
                _moegemm_native.check(fn(ptr(ids[t0:t1]), (t1 - t0) * A, E, ptr(plan), nbytes, stream), what)
            plans.append(plan)
    return plans


def _grouped_plans_of(what: str, plan, ids: Tensor, T: int, A: int, E: int):
    """The caller's plans, checked against the cuts of this call, or new ones."""
    if plan is None:
        return _grouped_plans(what, ids, T, A, E)
    cuts = _grouped_cuts(T, A)
    if not isinstance(plan, (list, tuple)) or len(plan) != len(cuts) or any(
            not isinstance(q, Tensor) or q.dtype != torch.uint8 or q.device != ids.device or not q.is_contiguous()
            or q.numel() < _moegemm_native.plan_bytes((t1 - t0) * A, E) for q, (t0, t1) in zip(plan, cuts)):
        raise ValueError(f"{what}: plan must be what moe_grouped_plan returned for these expert_ids and {E} experts: "
                         f"{len(cuts)} uint8 tensor(s) on {ids.device}")
    return list(plan)


def _grouped_experts(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, plan):
    per_slot = x.dim() == 3
    out = torch.empty(T, A, N, dtype=out_dtype, device=x.device)
    if T * A == 0:
        return out
    plans = _grouped_plans_of(what, plan, ids, T, A, E)
    fn = _moegemm_native.lib().mbnb_moegemm_experts
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for (t0, t1), q in zip(_grouped_cuts(T, A), plans):
            _moegemm_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, int(per_slot), K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, N,
                                     ptr(ids[t0:t1]), ptr(b), 0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out[t0:t1]), ocode,
                                     ptr(q), q.numel(), stream), what)
    return out


def _grouped_glu(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, alpha, limit, plan):
    I = N // 2
    out = torch.empty(T, A, I, dtype=out_dtype, device=x.device)
    if T * A == 0:
        return out
    plans = _grouped_plans_of(what, plan, ids, T, A, E)
    fn = _moegemm_native.lib().mbnb_moegemm_gate_up_glu
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for (t0, t1), q in zip(_grouped_cuts(T, A), plans):
            _moegemm_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, I, ptr(ids[t0:t1]), ptr(b),
                                     0 if b is None else _native.DTYPE_CODE[b.dtype], alpha, limit, ptr(out[t0:t1]), ocode, ptr(q), q.numel(),
                                     stream), what)
    return out


def _grouped_sum(what, x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode, plan):
    if T * A == 0:
        return torch.zeros(T, N, dtype=out_dtype, device=x.device)
    out = torch.empty(T, N, dtype=out_dtype, device=x.device)
    plans = _grouped_plans_of(what, plan, ids, T, A, E)
    cuts = _grouped_cuts(T, A)
    ws_bytes = _moegemm_native.workspace_bytes((cuts[0][1] - cuts[0][0]) * A, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    fn = _moegemm_native.lib().mbnb_moegemm_down_sum
    with on_device(x.device):
        stream = stream_ptr(x.device)
        for (t0, t1), q in zip(cuts, plans):
            _moegemm_native.check(fn(ptr(x[t0:t1]), t1 - t0, A, K, dtype_code(x.dtype, what), ptr(w), ptr(s), E, N, ptr(ids[t0:t1]), ptr(b),
                                     0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(rw[t0:t1]), _native.DTYPE_CODE[rw.dtype],
                                     ptr(out[t0:t1]), ocode, ptr(ws), ws_bytes, ptr(q), q.numel(), stream), what)
    return out


def matmul_mxfp4_experts_grouped(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, bias: Optional[Tensor] = None,
                                 dtype: Optional[torch.dtype] = None, plan=None) -> Tensor:
    """
    `matmul_mxfp4_experts` on the grouped GEMM of libmbnb_moegemm.so, at any number of pairs: the same operands, checks, errors and
    result BITS -> ``[T, A, N]``.  The routing is planned on the device (two small launches, no host round trip), then one launch
    of `k_mx_experts_grouped` serves up to `MOE_GROUPED_MAX_PAIRS` pairs (more are cut over the tokens): every expert's pairs are
    taken 64 at a time against one decode of the weight tile.  `plan`: what `moe_grouped_plan` returned for these ids, to share
    one plan between projections; None builds it here.  Ids are read on the device, so a captured graph serves a new routing once
    `expert_ids` is overwritten in place (the plan launches are part of the graph when they are captured with the call).  At
    most 1024 experts.  Inference only.
    """
    what = "matmul_mxfp4_experts_grouped"
    x, w, s, ids, b, _, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moegemm_native, input, weight, weight_scales, expert_ids, bias,
                                                                          None, dtype)
    return _grouped_experts(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, plan)


def matmul_mxfp4_experts_grouped_glu(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, bias: Optional[Tensor] = None,
                                     alpha: float = 1.702, limit: float = 7.0, dtype: Optional[torch.dtype] = None, plan=None) -> Tensor:
    """
    `matmul_mxfp4_experts_glu` on the grouped GEMM, at any number of pairs: the same operands, checks, errors and result bits ->
    ``[T, A, I]``; the gated activation is the epilogue of the one launch per cut.  `plan` as in `matmul_mxfp4_experts_grouped`.
    """
    what = "matmul_mxfp4_experts_grouped_glu"
    alpha, limit = float(alpha), float(limit)
    if not math.isfinite(alpha) or not limit > 0:
        raise ValueError(f"{what}: alpha ({alpha}) must be finite and limit ({limit}) positive (inf: no clamp)")
    if weight.dim() in (3, 4) and weight.shape[1] % 2:
        raise ValueError(f"{what}: weight {tuple(weight.shape)} has {weight.shape[1]} rows: the interleaved gate / up rows come in pairs")
    x, w, s, ids, b, _, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moegemm_native, input, weight, weight_scales, expert_ids, bias,
                                                                          False, dtype)
    return _grouped_glu(what, x, w, s, ids, b, T, A, E, N, K, out_dtype, ocode, alpha, limit, plan)


def matmul_mxfp4_experts_grouped_sum(input: Tensor, weight: Tensor, weight_scales: Tensor, expert_ids: Tensor, routing_weights: Tensor,
                                     bias: Optional[Tensor] = None, dtype: Optional[torch.dtype] = None, plan=None) -> Tensor:
    """
    `matmul_mxfp4_experts_sum` on the grouped GEMM, at any number of pairs: the same operands, checks, errors and result bits ->
    ``[T, N]``; the projection goes in f32 into a workspace that is a ``torch.empty`` of this call (at most `MOE_GROUPED_MAX_PAIRS`
    rows), the routed sum over the slots follows as a second launch.  `plan` as in `matmul_mxfp4_experts_grouped`.
    """
    what = "matmul_mxfp4_experts_grouped_sum"
    x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode = _expert_operands(what, _moegemm_native, input, weight, weight_scales, expert_ids, bias,
                                                                           True, dtype, routing_weights)
    return _grouped_sum(what, x, w, s, ids, b, rw, T, A, E, N, K, out_dtype, ocode, plan)


# ============================================================================= the router of the mixture-of-experts block
# libmbnb_router.so: the router's logits in f32, the top-k selection (ties to the lower expert) and the softmax over
# the selected logits in one launch; int32 ids and the routing weights, as the launches above read them.
_ROUTER_WEIGHT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def moe_router_topk(input: Tensor, weight: Tensor, bias: Optional[Tensor] = None, top_k: int = 4,
                    weights_dtype: torch.dtype = torch.float32, return_logits: bool = False):
    """
    The router of a mixture-of-experts block (gpt-oss): ``logits = input @ weight^T + bias`` in f32, the `top_k` largest per token
    and the softmax over those -> ``(expert_ids int32 [T, top_k], routing_weights [T, top_k])``, plus ``logits`` f32 [T, E] with
    ``return_logits=True``.  `input` [..., K], f16 or bf16, is flattened to [T, K]; `weight` [E, K] of the same dtype; `bias` [E] or
    None, read as f32.

    One launch of `k_router`, one workgroup per token.  The logits are accumulated in f32 from the exact products and are NOT
    rounded to 16 bits, as ``F.linear`` would round them: fewer ties.  The ids are in descending order of the logit; among equal
    logits (-0 equals +0) the lower expert index comes first, and a NaN logit ranks above everything, so the routing of a token
    does not depend on the batch it is in: its ids, weights and logits are bit-equal alone and in any batch.  With the selected
    logits v, ``w[a] = exp(v[a] - v[0]) / sum_a exp(v[a] - v[0])``, the sum in slot order, every operation in f32, one rounding
    to `weights_dtype` (float32, float16 or bfloat16).  The outputs are ``torch.empty`` tensors of this call and nothing
    synchronises, so the call can be captured in a graph.  At most 1024 experts, `top_k` at most ``min(E, 32)``, K a multiple of
    8 up to 16384.  Inference only: no gradient is defined.
    """
    what = "moe_router_topk"
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (input, weight, bias)):
        raise NotImplementedError(f"{what} is inference-only: it defines no gradient for its input, weight or bias "
                                  "(call it under torch.no_grad(), or detach them)")
    if weight.dim() != 2:
        raise ValueError(f"{what}: weight must be [E, K], got {tuple(weight.shape)}")
    E, K = weight.shape
    if E <= 0 or E > _router_native.MAX_EXPERTS:
        raise ValueError(f"{what}: {E} experts, 1 to {_router_native.MAX_EXPERTS} in one launch")
    if K <= 0 or K % _router_native.CHUNK or K > _router_native.MAX_K:
        raise ValueError(f"{what}: the last dimension ({K}) must be a positive multiple of {_router_native.CHUNK}, at most {_router_native.MAX_K}")
    if input.dim() < 1 or input.shape[-1] != K:
        raise ValueError(f"{what}: input {tuple(input.shape)} does not match weight {tuple(weight.shape)} (K = {K})")
    if input.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{what}: input must be float16 or bfloat16 (16-bit activations), got {input.dtype}")
    if weight.dtype != input.dtype:
        raise ValueError(f"{what}: weight ({weight.dtype}) must have the input's dtype ({input.dtype})")
    if bias is not None and (tuple(bias.shape) != (E,) or not bias.dtype.is_floating_point):
        raise ValueError(f"{what}: bias must be a floating-point tensor [E] = {(E,)}, got {bias.dtype} {tuple(bias.shape)}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1 or top_k > min(E, _router_native.MAX_TOPK):
        raise ValueError(f"{what}: top_k ({top_k!r}) must be an integer from 1 to min(E, {_router_native.MAX_TOPK}) = {min(E, _router_native.MAX_TOPK)}")
    if weights_dtype not in _ROUTER_WEIGHT_DTYPES:
        raise ValueError(f"{what}: weights_dtype must be float32, float16 or bfloat16, got {weights_dtype}")
    for t in (input, weight):
        _check_device(t, what)
    x = _aligned16(input.reshape(-1, K))
    w = _aligned16(weight.to(x.device))
    b = None if bias is None else bias.to(x.device).contiguous()
    if b is not None and b.dtype not in _native.DTYPE_CODE:
        b = b.float()
    T = x.shape[0]
    ids = torch.empty(T, top_k, dtype=torch.int32, device=x.device)
    rw = torch.empty(T, top_k, dtype=weights_dtype, device=x.device)
    logits = torch.empty(T, E, dtype=torch.float32, device=x.device) if return_logits else None
    if T > 0:
        with on_device(x.device):
            _router_native.check(_router_native.lib().mbnb_router_topk_softmax(
                ptr(x), T, K, dtype_code(x.dtype, what), ptr(w), E, ptr(b), 0 if b is None else _native.DTYPE_CODE[b.dtype], top_k,
                ptr(ids), ptr(rw), _native.DTYPE_CODE[weights_dtype], ptr(logits), stream_ptr(x.device)), what)
    return (ids, rw, logits) if return_logits else (ids, rw)


def moe_block_mxfp4(input: Tensor, router_weight: Tensor, router_bias: Optional[Tensor], gate_up_weight: Tensor, gate_up_scales: Tensor,
                    gate_up_bias: Optional[Tensor], down_weight: Tensor, down_scales: Tensor, down_bias: Optional[Tensor], top_k: int = 4,
                    alpha: float = 1.702, limit: float = 7.0, return_routing: bool = False):
    """
    The whole mixture-of-experts block (gpt-oss `mlp`) for `input` [..., H] -> ``[..., H]`` in the input's dtype:
    ``moe_mlp_mxfp4(x, experts..., *moe_router_topk(x, router_weight, router_bias, top_k))`` and nothing more: four launches in
    three C calls, no torch op, no synchronisation and no host-side tensor between the hidden state and its output.  With
    ``return_routing=True`` also ``(expert_ids, routing_weights)``, [T, top_k] over the flattened tokens.
    """
    x = input.reshape(-1, input.shape[-1]) if input.dim() != 2 else input
    ids, rw = moe_router_topk(x, router_weight, router_bias, top_k)
    out = moe_mlp_mxfp4(x, gate_up_weight, gate_up_scales, gate_up_bias, down_weight, down_scales, down_bias, ids, rw, alpha, limit)
    out = out.reshape(*input.shape[:-1], out.shape[-1])
    return (out, (ids, rw)) if return_routing else out
