"""CPU-side checks of the input-gradient entry points (mbnb_linear_grad_input and its workspace query): declared, bound and
exported; the query is pure host code with pinned values; argument errors come back through the status / last-error convention
without touching a device; and the autograd route keeps the device gate of the forwards."""
import ctypes
import os
import re

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd.functional import QuantState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mbnb_linear_grad_input", "mbnb_linear_grad_input_workspace_bytes")
NF4, FP4, INT8, FP8, DENSE = 0, 1, 2, 3, 4
F16, BF16, F32 = 0, 1, 2


def test_grad_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbnb_hip.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert (_native.W_INT8_ROWWISE, _native.W_FP8_E4M3, _native.W_DENSE) == (INT8, FP8, DENSE)
    assert re.search(r"MBNB_W_INT8_ROWWISE = 2, MBNB_W_FP8_E4M3 = 3, MBNB_W_DENSE = 4", header)


def test_grad_workspace_query_is_pure_host_code():
    """Dense path: the transposed weight Wt [K, N] (K x N x 2 bytes, 256-byte granules) plus the dense GEMM's own split-K share for
    the product dY [M, N] . Wt^T (output width K, reduction N); 0 where only the generic kernel applies."""
    lib = _native.lib()
    q, gemm = lib.mbnb_linear_grad_input_workspace_bytes, lib.mbnb_gemm_dense_workspace_bytes
    assert q(4096, 4096, 4096, NF4, BF16) == 4096 * 4096 * 2 == 33554432
    assert q(1024, 11008, 4096, NF4, BF16) == q(1024, 4096, 11008, FP4, F16) == 4096 * 11008 * 2
    assert q(512, 4096, 4096, FP4, F16) == 4096 * 4096 * 2
    # below the decode-once threshold the same two steps run; the GEMM's plan splits the long reduction of a skinny product
    assert q(1, 4096, 4096, NF4, BF16) == 4096 * 4096 * 2 + gemm(1, 4096, 4096) == 33554432 + 8 * 4096 * 4
    assert q(128, 4096, 4096, NF4, BF16) == 4096 * 4096 * 2 + gemm(128, 4096, 4096) == 50331648
    for M, N, K in ((4096, 4096, 4096), (7, 4160, 127), (300, 128, 1000)):
        wt = (K * N * 2 + 255) // 256 * 256
        assert q(M, N, K, NF4, BF16) == wt + gemm(M, K, N)
    assert q(64, 128, 96, INT8, F16) == q(64, 128, 96, FP8, BF16) == q(64, 128, 96, DENSE, F16) == 128 * 96 * 2
    # only the generic kernel: f32 weights, a reduction N that is not a multiple of 64 or below 128, K % 8 for the byte formats
    assert q(4096, 4096, 4096, NF4, F32) == 0
    for N in (63, 64, 127, 4100):
        assert q(256, N, 4096, NF4, BF16) == 0
    assert q(64, 128, 100, INT8, F16) == q(64, 128, 100, FP8, F16) == q(64, 128, 100, DENSE, F16) == 0
    assert q(64, 128, 100, NF4, F16) > 0           # the 4-bit pass reads the padded row: any K
    # not a problem
    assert q(0, 4096, 4096, NF4, BF16) == q(16, 0, 4096, NF4, BF16) == q(16, 4096, 0, NF4, BF16) == 0
    assert q(4096, 4096, 4096, 5, BF16) == q(4096, 4096, 4096, NF4, 7) == q(4096, 4096, 4096, -1, BF16) == 0


def test_grad_argument_errors_use_status_and_last_error():
    lib = _native.lib()
    one = ctypes.c_void_p(256)    # any non-NULL, aligned value: validation must fail before a dereference
    am = _native.AbsmaxDesc(256, None, None, 0)
    f = lib.mbnb_linear_grad_input

    def call(fmt=NF4, M=4, N=8, K=64, K_weight=64, bs=64, wd=F16, od=F16, absmax=am, scales=one, flags=0, ws_bytes=0):
        return f(one, M, N, fmt, one, None if absmax is None else ctypes.byref(absmax), scales, K, K_weight, bs, wd, od, one, None, ws_bytes,
                 flags, None)

    assert call(fmt=5) == -1 and b"w_format" in lib.mbnb_last_error()
    assert call(wd=7) == -1 and b"dtype" in lib.mbnb_last_error()
    assert call(od=3) == -1 and b"dtype" in lib.mbnb_last_error()
    assert call(flags=1) == -1 and b"flags" in lib.mbnb_last_error()
    assert call(bs=48) == -1 and b"blocksize" in lib.mbnb_last_error()
    assert call(K_weight=32) == -2 and b"K_weight" in lib.mbnb_last_error()
    assert call(K=64, K_weight=96) == -2                  # not a whole number of blocks
    assert call(fmt=INT8, K_weight=72) == -2 and b"K_weight" in lib.mbnb_last_error()
    assert call(M=-1) == -1 and b"negative" in lib.mbnb_last_error()
    assert call(ws_bytes=-5) == -1
    assert call(absmax=None) == -1 and b"absmax" in lib.mbnb_last_error()
    assert call(absmax=_native.AbsmaxDesc(None, 256, None, 256)) == -1 and b"absmax2" in lib.mbnb_last_error()
    assert call(fmt=INT8, scales=None) == -1 and b"scales" in lib.mbnb_last_error()
    assert call(fmt=FP8, scales=None) == -1
    assert call(flags=2, od=BF16) == -1 and b"transposed pass" in lib.mbnb_last_error()
    # empty problems are a no-op success
    assert call(M=0) == 0
    assert call(K=0, K_weight=0) == 0
    assert f(None, 0, 8, NF4, None, None, None, 64, 64, 64, F16, F16, None, None, 0, 0, None) == 0


def test_autograd_route_keeps_the_device_gate():
    """A CPU input that requires grad takes the autograd route and still meets the forwards' device gate (no CPU path)."""
    x = torch.zeros(2, 64, requires_grad=True)
    st = QuantState(absmax=torch.ones(2), shape=torch.Size([2, 64]), blocksize=64, quant_type="nf4", dtype=torch.float32)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.matmul_4bit(x, torch.zeros(64, dtype=torch.uint8), st)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.functional.linear_int8(x, torch.zeros(2, 64, dtype=torch.int8), torch.ones(2))
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.functional.linear_dense(x, torch.zeros(2, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.functional.matmul_fp8_e4m3(x, torch.zeros(2, 64, dtype=torch.uint8), torch.ones(2))
    bias = torch.zeros(2, requires_grad=True)     # only the bias requires grad: the same route, the same gate
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.matmul_4bit(torch.zeros(2, 64), torch.zeros(64, dtype=torch.uint8), st, bias)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        bnb.functional._dequantize_t(torch.zeros(64, dtype=torch.uint8), st)
