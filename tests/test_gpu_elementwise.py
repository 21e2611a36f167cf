"""
Every kernel the library can report, element by element against float64, on poisoned allocations.

The cases are the tables of tests/kernel_cases.py (one case at least per kernel name) and tests/gemm_variant_cases.py (one per variant
behind a name, per dispatch limit and per launch-grid limit; those also hold the variant the launcher reports).  Each runs through the public API (mbnb_gemm_dense through the C ABI) right
after a one-row embedding lookup whose kernel name is known, so a launch that sets no name shows up as that name instead of
passing on a stale one; it must dispatch to its named kernel, and every output element must lie within the bound of
tests/elementwise.py around a float64 product of the operands the op feeds the kernel -- the decoded weight taken from the CPU
oracle, and the library's own dequantise checked against it bit for bit.  Outputs and workspaces come from functional.py's
poisoned torch.empty (tests/poison.py), or are poisoned by hand where a test allocates them.  The largest err / bound ratio
of every case is printed (run with -s).
"""
import time

import numpy as np
import pytest
import torch

import oracle
from mps_bitsandbytes_amd import _native, synthetic
from mps_bitsandbytes_amd import functional as F
from tests import gemm_variant_cases, kernel_cases
from tests.elementwise import (UNIT, assert_bound_elementwise, assert_int8_elementwise, assert_linear_elementwise,
                               int8_reference)
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_SENTINEL = {}


def _poison(t):
    t.reshape(-1).view(torch.uint8).fill_(0xFF)
    return t


def _offset(t, n):
    """t's values in a slice that starts n elements into a larger buffer: an operand off its alignment by n elements."""
    buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    buf[n:] = t.reshape(-1)
    return buf[n:].view(t.shape)


def _sentinel(kernel):
    """Run a one-row embedding lookup (not the case's own kernel) and return its name."""
    if not _SENTINEL:
        _SENTINEL["q8"] = torch.ones(4, 64, dtype=torch.int8, device=DEV)
        _SENTINEL["s8"] = torch.ones(4, dtype=torch.float32, device=DEV)
        _SENTINEL["p4"] = torch.zeros(4, 32, dtype=torch.uint8, device=DEV)
        _SENTINEL["a4"] = torch.ones(4, 1, dtype=torch.float32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)
    if kernel == "embedding8":
        F.embedding_4bit(idx, _SENTINEL["p4"], _SENTINEL["a4"], 64)
        name = "embedding4"
    else:
        F.embedding_8bit(idx, _SENTINEL["q8"], _SENTINEL["s8"])
        name = "embedding8"
    assert _native.last_kernel() == name
    assert _native.last_variant() == "", "a call whose launcher sets no variant reports the previous call's"
    return name


def _check_name(got, c):
    want = c["kernel"]
    ok = got.startswith(want) if want.endswith(" ") else got == want
    assert ok, f"{kernel_cases.case_id(c)}: dispatched {got!r}, the case is for {want!r}"
    if "variant" in c:
        variant = _native.last_variant()
        assert variant == c["variant"], f"{kernel_cases.case_id(c)}: {got!r} took the variant {variant!r}, the case is for {c['variant']!r}"


def _same_bits(a, b):
    """Bit-equal wherever a value is a number, NaN in the same places (NaN payloads and signs may differ)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(torch.where(nan, 0, a).view(iv), torch.where(nan, 0, b).view(iv))


def _activation(c, K, dt, seed):
    """X as the op is fed it: rows scaled by 2^e, non-finite values planted, a row slice or a misaligned view if asked."""
    lead = tuple(c["lead"]) if "lead" in c else (c["M"],)
    rows = int(np.prod(lead))
    X = synthetic.normal_device((rows, K), dt, seed=seed)
    if "xexp" in c:
        lo, hi = c["xexp"]
        e = torch.linspace(lo, hi, rows, device=DEV).round().double()
        X = (X.double() * torch.exp2(e)[:, None]).to(dt)
    if "x" in c.get("bad", ""):
        X[1 % rows, 3] = float("nan")
        X[3 % rows, 5] = float("inf")
        X[4 % rows, 9] = float("-inf")
    if c.get("view") == "rows":
        big = synthetic.normal_device((rows + 4, K), dt, seed=seed + 1)
        big[3:3 + rows] = X
        X = big[3:3 + rows]
    elif c.get("view") == "misaligned":
        flat = torch.empty(rows * K + 1, dtype=dt, device=DEV)
        flat[1:] = X.reshape(-1)
        X = flat[1:].view(rows, K)
        assert X.data_ptr() % 16 == X.element_size()
    return X.reshape(*lead, K)


def _bias(c, N, dt, seed):
    return synthetic.normal_device((N,), dt, seed=seed) if c.get("bias") else None


def _quant_4bit(c, N, K, dt, seed):
    """The oracle's quantisation of the case's weight on the CPU: (packed, absmax, state2 or None)."""
    qt, bs, cs = c.get("qt", "nf4"), c.get("bs", 64), c.get("cs", False)
    W = synthetic.normal((N, K), dt, seed=seed)
    op, oa, ost2 = oracle.quantize_4bit(W, bs, qt, cs and "bs2" not in c)
    if "bs2" in c:                                  # the nested absmax at a second blocksize of the case's choosing
        oa, am2 = oracle.quantize_blockwise(oa, blocksize=c["bs2"])
        ost2 = (am2, c["bs2"])
    if "w" in c.get("bad", ""):
        assert not cs
        oa = oa.clone()
        oa[oa.numel() // 3] = float("nan")
    return op, oa, ost2


def _state_4bit(c, N, K, dt, op, oa, ost2):
    """(packed, QuantState) on the GPU of a quantisation and the oracle's decoded weight [N, K]."""
    qt, bs, cs = c.get("qt", "nf4"), c.get("bs", 64), c.get("cs", False)
    Wd = oracle.dequantize_4bit(op, oa, (N, K), bs, qt, dt, ost2)
    st2 = None
    if cs:
        st2 = F.QuantState(absmax=ost2[0].to(DEV), shape=torch.Size([oa.numel()]), blocksize=ost2[1], quant_type="int8", dtype=torch.float32)
    am = oa.to(DEV)
    st = F.QuantState(absmax=am, shape=torch.Size([N, K]), blocksize=bs, quant_type=qt, dtype=dt, state2=st2)
    packed = op.to(DEV)
    assert _same_bits(F.dequantize_4bit(packed, st), Wd), "dequantize_4bit differs from the oracle's decode"
    view = c.get("view")
    if view == "absmax+4":                          # the f32 absmax 4 bytes off 16-byte alignment
        assert not cs
        st.absmax = _offset(am, 1)
        assert st.absmax.data_ptr() % 16 == 4
    elif view == "codes+1":                         # the nested int8 absmax codes 1 byte off 4-byte alignment
        assert cs and am.dtype == torch.int8
        st.absmax = _offset(am, 1)
        assert st.absmax.data_ptr() % 4 == 1
    elif view in ("packed+4", "packed+2"):          # the packed nibbles off 16-byte / off 4-byte alignment
        packed = _offset(packed, int(view[-1]))
        assert packed.data_ptr() % 16 == int(view[-1])
    return packed, st, Wd


def _weight_4bit(c, N, K, dt, seed):
    """(packed, QuantState) on the GPU and the oracle's decoded weight [N, K] (a NaN absmax in one block for bad "w")."""
    return _state_4bit(c, N, K, dt, *_quant_4bit(c, N, K, dt, seed))


def _quant_8bit(c, N, K, dt, seed, fp8):
    """The oracle's row-wise int8 / FP8 quantisation of the case's weight on the CPU: (q, scales)."""
    W = synthetic.normal((N, K), dt, seed=seed, std=0.05)
    q, s = (oracle.quantize_fp8_e4m3 if fp8 else oracle.quantize_rowwise)(W)
    if "w" in c.get("bad", ""):
        if fp8:
            q = q.clone()
            q[N // 2, K // 3] = 0x7F
        else:
            s = s.clone()
            s[N // 2] = float("nan")
    return q, s


def _state_8bit(c, dt, fp8, q, s):
    """(q, scales) on the GPU of a quantisation and the oracle's decoded weight."""
    Wd = (oracle.dequantize_fp8_e4m3 if fp8 else oracle.dequantize_rowwise)(q, s, dt)
    qd, sd = q.to(DEV), s.to(DEV)
    mine = (F.dequantize_fp8_e4m3 if fp8 else F.dequantize_rowwise)(qd, sd, dt)
    assert _same_bits(mine, Wd), "the library's dequantise differs from the oracle's"
    if c.get("view") == "w+1":                      # the weight bytes 1 byte off 16-byte alignment
        qd = _offset(qd, 1)
        assert qd.data_ptr() % 16 == 1
    return qd, sd, Wd


def _weight_8bit(c, N, K, dt, seed, fp8):
    """(q, scales) on the GPU and the oracle's decoded weight (a NaN row scale / FP8 byte 0x7F for bad "w")."""
    return _state_8bit(c, dt, fp8, *_quant_8bit(c, N, K, dt, seed, fp8))


def _quantized(c, kind, N, K, dt, seed):
    """The CPU quantisation behind a quantised linear of `kind` ("4bit", "int8", "fp8"): what _forward takes."""
    return _quant_4bit(c, N, K, dt, seed) if kind == "4bit" else _quant_8bit(c, N, K, dt, seed, kind == "fp8")


def _forward(c, kind, N, K, dt, quant):
    """(Wd, fwd): the oracle's decode of a quantisation and fwd(X, bias, out_dtype) -> y through the public API."""
    if kind == "4bit":
        packed, st, Wd = _state_4bit(c, N, K, dt, *quant)
        return Wd, lambda X, b=None, out=None: F.matmul_4bit(X, packed, st, b, out)
    q, s, Wd = _state_8bit(c, dt, kind == "fp8", *quant)
    if kind == "int8":
        return Wd, lambda X, b=None, out=None: F.linear_int8(X, q, s, b)
    return Wd, lambda X, b=None, out=None: F.matmul_fp8_e4m3(X, q, s, b, dt)


KIND = {"matmul_4bit": "4bit", "linear_int8": "int8", "matmul_fp8": "fp8"}


def _launch(c, call):
    """call() right after the sentinel launch: (its result, the kernel name), the name and the variant checked against the case."""
    _sentinel(c["kernel"])
    y = call()
    kern = _native.last_kernel()
    _check_name(kern, c)
    return y, kern


def _run_linear(c, monkeypatch):
    op, N, K, dt = c["op"], c["N"], c["K"], DT[c["dt"]]
    if c.get("fused"):
        monkeypatch.setattr(F, "DECODE_ONCE", False)
    X = _activation(c, K, dt, seed=11)
    b = _bias(c, N, dt, seed=12)
    out = DT.get(c.get("out"))
    if op in KIND:
        Wd, fwd = _forward(c, KIND[op], N, K, dt, _quantized(c, KIND[op], N, K, dt, seed=13))
    else:
        Wd = synthetic.normal_device((N, K), dt, seed=13, std=0.05)
        fwd = lambda X, b=None, out=None: F.linear_dense(X, Wd, b)          # noqa: E731
    y, kern = _launch(c, lambda: fwd(X, b, out))
    return kern, assert_linear_elementwise(y, X, Wd, b, dt, out or dt, kern)


def _gemm_dense_operands(c):
    """(X, Wfull, bias, call) of a mbnb_gemm_dense case: call() poisons the output and the partials and launches on X as it is."""
    M, N, K, ldw, dt = c["M"], c["N"], c["K"], c["ldw"], DT[c["dt"]]
    odt = DT[c.get("out", c["dt"])]
    lib = _native.lib()
    X = _activation(c, K, dt, seed=21)
    Wfull = synthetic.normal_device((N, ldw), dt, seed=22, std=0.05)
    b = _bias(c, N, dt, seed=23)
    slices = c["slices"]
    code = _native.DTYPE_CODE[dt]

    def call():
        out = _poison(torch.empty(M, N, dtype=odt, device=DEV))
        ws = _poison(torch.empty(slices * M * N * 4, dtype=torch.uint8, device=DEV)) if slices > 1 else None
        rc = lib.mbnb_gemm_dense(X.data_ptr(), Wfull.data_ptr(), code, None if b is None else b.data_ptr(), _native.DTYPE_CODE[odt],
                                 out.data_ptr(), M, N, K, ldw, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                                 slices | (c["tile"] << 8), _native.stream_ptr(DEV))
        assert rc == 0, lib.mbnb_last_error()
        return out
    return X, Wfull, b, call


def _run_gemm_dense(c):
    K, dt = c["K"], DT[c["dt"]]
    X, Wfull, b, call = _gemm_dense_operands(c)
    out, kern = _launch(c, call)
    return kern, assert_linear_elementwise(out, X, Wfull[:, :K], b, dt, DT[c.get("out", c["dt"])], kern)


def _run_matmul_int8(c, plant=None):
    """plant(sa, sb), if given, changes the row and column scales in place before the launch."""
    M, N, K = c["M"], c["N"], c["K"]
    odt = DT[c["out"]]
    A = synthetic.int8_tensor((M, K), seed=31).to(DEV)
    B = synthetic.int8_tensor((K, N), seed=32).to(DEV)
    sa = (synthetic.normal((M,), torch.float32, seed=33).abs() + 0.5).to(DEV)
    sb = (synthetic.normal((N,), torch.float32, seed=34).abs() + 0.5).to(DEV)
    if "w" in c.get("bad", ""):
        sb[N // 2] = float("nan")
    if plant is not None:
        plant(sa, sb)
    if c.get("view") == "a+1":
        A = _offset(A, 1)
    elif c.get("view") == "b+1":
        B = _offset(B, 1)
    _sentinel(c["kernel"])
    y = F.matmul_int8(A, B, sa, sb, odt)
    kern = _native.last_kernel()
    _check_name(kern, c)
    return kern, assert_int8_elementwise(y, int8_reference(A, B, sa, sb), odt, kern)


def _backward(c, fwd, x, dY):
    """(x.grad, the kernel name) of y = fwd(x) under y.backward(dY), the name taken right after the op's backward."""
    x = x.detach().requires_grad_(True)
    seen = []
    y = fwd(x)
    # both hooks run on autograd's device thread, whose last-kernel record is its own: the sentinel just before the backward
    # of the op, the name just after it
    y.register_hook(lambda g: seen.append(_sentinel(c["kernel"])) and None)
    x.register_hook(lambda g: seen.append(_native.last_kernel()) and None)
    y.backward(dY)
    assert len(seen) == 2, seen
    kern = seen[1]
    _check_name(kern, c)
    return x.grad, kern


def _run_grad(c):
    """dX = cast(round_w(dY.to(w_dtype) . dequant(W)), x.dtype): the contraction runs over N."""
    M, N, K, dt, fmt = c["M"], c["N"], c["K"], DT[c["dt"]], c["fmt"]
    Wd, fwd = _forward(c, fmt, N, K, dt, _quantized(c, fmt, N, K, dt, seed=41))
    x = synthetic.normal_device((M, K), dt, seed=42)
    dY = _activation(dict(c, M=M), N, dt, seed=43)
    dx, kern = _backward(c, fwd, x, dY)
    return kern, assert_linear_elementwise(dx, dY, Wd.t().contiguous().to(DEV), None, dt, dt, kern)


def _run_grad_t(c):
    """The transposed dequantise pass alone: bit for bit the oracle's decode, transposed."""
    N, K, dt, fmt = c["N"], c["K"], DT[c["dt"]], c["fmt"]
    if fmt == "4bit":
        packed, st, Wd = _weight_4bit(c, N, K, dt, seed=51)
        _sentinel(c["kernel"])
        Wt = F._dequantize_t(packed, st)
    else:
        q, s, Wd = _weight_8bit(c, N, K, dt, seed=51, fp8=fmt == "fp8")
        _sentinel(c["kernel"])
        Wt = F._dequantize_t(q, scales=s, fmt=fmt, dtype=dt)
    kern = _native.last_kernel()
    _check_name(kern, c)
    assert _same_bits(Wt, Wd.t().contiguous()), f"{kern}: the transposed pass differs from the oracle's decode"
    return kern, 0.0


def _run_outlier(c):
    """OutlierAwareLinear against oracle.outlier_linear on every element.  Both quantise the non-outlier columns of x row-wise
    to int8 the same way; the kernel contracts the integers exactly where the oracle multiplies the decoded operands rounded to
    the compute dtype (the reference's numerics), so the bound is 2 ulps of |ref| (the two final roundings), 3 u + g over the
    decomposition S = (|x| + max|x_row| / 127) . |Wd|^T + |b| (the two operand roundings and the accumulation), and one int8 step
    of x on one element of the row (a tie quantised the other way)."""
    M, N, K, dt, n_out = c["M"], c["N"], c["K"], DT[c["dt"]], c["n_out"]
    W = synthetic.normal((N, K), torch.float32, seed=61, std=0.05)
    oidx = torch.from_numpy(np.sort((synthetic.uniform_u64(4 * n_out + 1, seed=62) % np.uint64(K)).astype(np.int64))).unique()[:n_out]
    W[:, oidx] *= 30.0
    W = W.to(dt)
    W0 = W.clone()
    W0[:, oidx] = 0
    q, s = oracle.quantize_rowwise(W0)
    ow = W[:, oidx].contiguous()
    b = synthetic.normal((N,), dt, seed=63) if c.get("bias") else None
    x = synthetic.normal((M, K), dt, seed=64)
    if "xexp" in c:                                  # rows over many binades, as _activation scales them
        lo, hi = c["xexp"]
        x = (x.double() * torch.exp2(torch.linspace(lo, hi, M).round().double())[:, None]).to(dt)
    _sentinel(c["kernel"])
    y = F.outlier_linear(x.to(DEV), q.to(DEV), s.to(DEV), oidx.to(DEV), ow.to(DEV), None if b is None else b.to(DEV), dt)
    kern = _native.last_kernel()
    _check_name(kern, c)
    ref = oracle.outlier_linear(x, q, s, oidx, ow, b).to(DEV).double()
    Wfull = oracle.dequantize_rowwise(q, s, dt).to(DEV).double()
    Wfull[:, oidx.to(DEV)] = ow.to(DEV).double()
    xd = x.to(DEV).double()
    step = xd.abs().amax(1, keepdim=True) / 127.0
    S = (xd.abs() + step) @ Wfull.abs().t() + (0 if b is None else b.to(DEV).double().abs())
    u = UNIT[dt]
    g = (K + 2) * 2.0 ** -23
    bound = 4 * u * ref.abs() + (3 * u + g) * S + step * Wfull.abs().amax(1)[None, :] + (2.0 ** -24 if dt == torch.float16 else 0.0)
    return kern, assert_bound_elementwise(y, ref, bound, kern, "outlier_linear")


def outlier_masked_bound(x, Wd, pos, ow, b, ref, dt):
    """The per-element bound of tests/test_gpu_nn_forms.py around oracle.outlier_linear: _run_outlier's terms, with the quantisation
    step taken from the row maximum over the KEPT columns and the outlier columns entering S through `ow` without a step.

    x [M, K] in dt, Wd [N, K] the oracle's decode of the int8 weight, pos the outlier columns, ow [N, len(pos)], b [N] or None, ref
    [M, N]; all on one device, the result float64.  With kept = the columns outside pos, m_i = max(max_kept |x_ik|, 1e-8) and
    step_i = m_i / 127 (quantize_rowwise's scale of the masked row: an outlier column neither sets it nor is quantised),

        S_in = sum_kept (|x_ik| + step_i) |Wd_nk| + sum_pos |x_ij| |ow_nj| + |b_n|

    bounds the magnitude of every partial result on either side: a kept activation is replaced by its code times step_i, at most step_i
    away; an outlier activation is used as it is.  Both sides quantise alike; the kernel contracts the integers exactly and scales once in
    f32, the oracle multiplies the two decoded operands rounded to dt and accumulates in f32.  So: the two operand roundings cost 2 u S,
    the accumulation and the f32 scaling g S with g = (K + 2) 2^-23, and the roundings of the two partial sums (the int8 product and the
    outlier term), done on both sides over values that differ by no more than the above, one more u S; the two last roundings (the sum of
    the partial sums, then the bias) act on values within that of ref: 2 u |ref| on each side.  One int8 step of x on one element of the
    row (a tie quantised the other way) adds step_i max_kept |Wd_nk|; half of f16's smallest subnormal covers a result rounded there.
    With the step taken over the full row instead, the x64 outlier columns would loosen the first and the last term 64-fold."""
    K = x.shape[1]
    dev = x.device
    keep = torch.ones(K, dtype=torch.bool, device=dev)
    keep[torch.as_tensor(pos, dtype=torch.int64, device=dev)] = False
    xd, Wk = x.double(), Wd.double().abs() * keep.double()[None, :]
    step = (xd.abs() * keep.double()[None, :]).amax(1, keepdim=True).clamp_min(1e-8) / 127.0
    S = ((xd.abs() + step) * keep.double()[None, :]) @ Wk.t()
    if len(pos):
        S = S + xd[:, torch.as_tensor(pos, dtype=torch.int64, device=dev)].abs() @ ow.double().abs().t()
    if b is not None:
        S = S + b.double().abs()[None, :]
    u = UNIT[dt]
    g = (K + 2) * 2.0 ** -23
    return 4 * u * ref.double().abs() + (3 * u + g) * S + step * Wk.amax(1)[None, :] + (2.0 ** -24 if dt == torch.float16 else 0.0)


def _run_embedding(c):
    M, dim, num, dt = c["M"], c["N"], c["K"], DT[c["dt"]]
    idx = torch.from_numpy((synthetic.uniform_u64(M, seed=71) % np.uint64(num)).astype(np.int64))
    if c["op"] == "embedding_4bit":
        W = synthetic.normal((num, dim), dt, seed=72)
        op, oa, _ = oracle.quantize_4bit(W, c["bs"], c["qt"])
        packed, absmax = op.view(num, dim // 2), oa.view(num, -1)
        ref = oracle.embedding_4bit(idx, packed, absmax, dim, c["bs"], c["qt"], None, dt)
        _sentinel(c["kernel"])
        y = F.embedding_4bit(idx.to(DEV), packed.to(DEV), absmax.to(DEV), dim, c["bs"], c["qt"], None, dt)
    else:
        W = synthetic.normal((num, dim), dt, seed=72)
        q, s = oracle.quantize_rowwise(W)
        ref = oracle.embedding_8bit(idx, q, s, None, dt)
        _sentinel(c["kernel"])
        y = F.embedding_8bit(idx.to(DEV), q.to(DEV), s.to(DEV), None, dt)
    kern = _native.last_kernel()
    _check_name(kern, c)
    assert _same_bits(y, ref), f"{kern} differs from the oracle"
    return kern, 0.0


ALL_CASES = kernel_cases.CASES + gemm_variant_cases.CASES


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.xfail(strict=True, reason=c["xfail"])) if "xfail" in c else c
                                  for c in ALL_CASES], ids=[kernel_cases.case_id(c) for c in ALL_CASES])
def test_kernel_case_elementwise(case, monkeypatch, poisoned_alloc):
    op = case["op"]
    t0 = time.perf_counter()
    if op in ("matmul_4bit", "linear_int8", "matmul_fp8", "linear_dense"):
        kern, ratio = _run_linear(case, monkeypatch)
    elif op == "gemm_dense":
        kern, ratio = _run_gemm_dense(case)
    elif op == "matmul_int8":
        kern, ratio = _run_matmul_int8(case)
    elif op == "grad":
        kern, ratio = _run_grad(case)
    elif op == "grad_t":
        kern, ratio = _run_grad_t(case)
    elif op == "outlier_linear":
        kern, ratio = _run_outlier(case)
    else:
        kern, ratio = _run_embedding(case)
    assert poisoned_alloc.poisoned > 0
    torch.cuda.synchronize()
    print(f"\nelementwise {kern} [{_native.last_variant() if op not in ('grad', 'grad_t') else ''}]: max err / bound {ratio:.3g} "
          f"({kernel_cases.case_id(case)}) {time.perf_counter() - t0:.2f} s")


def test_matmul_int8_transpose_path_at_the_offset_limit(poisoned_alloc):
    """K * N = 2^31 (M = 256, N = 65536, K = 32768): past the in-place kernel's 32-bit offsets (gemm_i8_inplace.hip), B -- a
    2 GiB int8 matrix -- is transposed into the workspace and multiplied by the dense pipeline.  Every element against the exact
    integer product, computed in column chunks (no float64 copy of B)."""
    M, N, K = 256, 65536, 32768
    g = torch.Generator(device=DEV).manual_seed(20261016)
    A = torch.randint(-127, 128, (M, K), generator=g, device=DEV, dtype=torch.int8)
    B = torch.randint(-127, 128, (K, N), generator=g, device=DEV, dtype=torch.int8)
    sa = torch.rand(M, generator=g, device=DEV) + 0.5
    sb = torch.rand(N, generator=g, device=DEV) + 0.5
    _sentinel("i8_transpose+dense")
    y = F.matmul_int8(A, B, sa, sb, torch.bfloat16)
    kern = _native.last_kernel()
    assert kern == "i8_transpose+dense", kern
    ref = int8_reference(A, B, sa, sb, chunk=4096)
    del B
    ratio = assert_int8_elementwise(y, ref, torch.bfloat16, kern)
    assert poisoned_alloc.poisoned > 0
    print(f"\nelementwise {kern}: max err / bound {ratio:.3g} (M={M} N={N} K={K})")
