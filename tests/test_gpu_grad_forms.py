"""
Every form and limit of the input-gradient path (mbnb_linear_grad_input: k_dequant_t, k_grad_generic, the dense path) on guarded buffers.

Each case of tests/grad_cases.py runs three times: on poisoned allocations, then under tests/guard.py's proxy with each of its two fills,
dY, W, the absmax of both levels, the scales and -- through the C ABI -- dX and the workspace placed inside guard bands at the case's
offsets (dX and the workspace of the autograd route are functional.py's own torch.empty calls, carved by the proxy's plan).  Per run:

- the library's name and variant after a sentinel call equal the case's and tests.grad_cases.model(case) (taken in hooks on autograd's
  device thread for the autograd route);
- the transposed pass is bit-equal to the CPU oracle's decode, transposed (NaN payloads apart);
- every element of dX lies within tests/elementwise.py's bound, contraction length N, around the float64 product of dY.to(w_dtype) and
  the oracle's decoded weight, non-finite elements where expected_nonfinite predicts them;
- on the dense path dX is bit-equal to linear_dense(dY, Wt) with Wt from _dequantize_t (a one-slice mbnb_gemm_dense where a short
  workspace costs the split);
- a bias gradient lies within UNIT[w_dtype] relative of the float64 column sum plus (M + 2) 2^-23 sum|dY|;
- dX has the same bits in all three runs (an element never written would hold the fill), and every band is intact.

The worst err / bound per kernel name is printed at the end of the module (run with -s).  Measured on an MI355X: grad_generic 0.996 (the
rounding of a bf16 dX at half an ulp, the bound's u_T |r| term), grad_t+dense 0.951, grad_t+dense_splitk 0.181, grad_t exact; the module's 553
tests take 5.3 s, the slowest 0.8 s.
"""
import ctypes

import pytest
import torch

import mps_bitsandbytes_amd as bnb
import oracle
from mps_bitsandbytes_amd import _native, synthetic
from mps_bitsandbytes_amd import functional as F
from tests import forms, grad_cases, guard
from tests.elementwise import UNIT, assert_bound_elementwise, expected_nonfinite, linear_bound
from tests.forms import memo as _memo
from tests.guard import guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
FMT_CODE = {"int8": _native.W_INT8_ROWWISE, "fp8": _native.W_FP8_E4M3, "dense": _native.W_DENSE}
WORST = {}
_SENTINEL = {}


def _sentinel():
    """A one-row embedding lookup: another entry point of the library, whose launcher sets no variant."""
    if not _SENTINEL:
        _SENTINEL["q8"] = torch.ones(4, 64, dtype=torch.int8, device=DEV)
        _SENTINEL["s8"] = torch.ones(4, dtype=torch.float32, device=DEV)
        _SENTINEL["idx"] = torch.zeros(1, dtype=torch.int64, device=DEV)
    F.embedding_8bit(_SENTINEL["idx"], _SENTINEL["q8"], _SENTINEL["s8"])
    assert (_native.last_kernel(), _native.last_variant()) == ("embedding8", "")


def _record():
    return _native.last_kernel(), _native.last_variant()


def _bits(t):
    """The values as integers on the CPU, every NaN as the dtype's default NaN (the contract says where a NaN is, not which one)."""
    t = t.detach()
    t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _key(c, *drop):
    return tuple(sorted((k, repr(v)) for k, v in c.items() if k not in ("op", "kernel", "variant", "off", "ws") + drop))


# ----------------------------------------------------------------------------------------------- operands
def _weight(c):
    """CPU, shared between the runs of a case: the weight as the library is given it and the oracle's decode [N, K]."""
    N, K, T, fmt, bad = c["N"], c["K"], DT[c["dt"]], c["fmt"], "w" in c.get("bad", "")
    if fmt == "4bit":
        bs, qt, cs = c.get("bs", 64), c.get("qt", "nf4"), bool(c.get("cs"))
        packed, am, st2 = oracle.quantize_4bit(synthetic.normal((N, K), T, seed=41), bs, qt, cs)
        if bad:
            assert not cs
            am = am.clone()
            am[am.numel() // 3] = float("nan")
        Wd = oracle.dequantize_4bit(packed, am, (N, K), bs, qt, T, st2)
        return dict(w=packed, absmax=am, absmax2=None if st2 is None else st2[0], bs2=0 if st2 is None else st2[1], scales=None, Wd=Wd)
    if fmt == "dense":
        Wd = synthetic.normal((N, K), T, seed=41, std=0.05)
        return dict(w=Wd, absmax=None, absmax2=None, scales=None, Wd=Wd)
    fp8 = fmt == "fp8"
    q, s = (oracle.quantize_fp8_e4m3 if fp8 else oracle.quantize_rowwise)(synthetic.normal((N, K), T, seed=41, std=0.05))
    if bad and fp8:
        q = q.clone()
        q[N // 2, K // 3], q[N // 3, K // 2] = 0x7F, 0xFF
    elif bad:
        s = s.clone()
        s[N // 2] = float("nan")
    return dict(w=q, absmax=None, absmax2=None, scales=s, Wd=(oracle.dequantize_fp8_e4m3 if fp8 else oracle.dequantize_rowwise)(q, s, T))


def _dy(c):
    """dY [M, N] in the weight dtype on the device: rows over binades, a NaN, a +Inf and a -Inf row where the case asks."""
    M, N, T = c["M"], c["N"], DT[c["dt"]]
    X = synthetic.normal_device((M, N), T, seed=43)
    if "xexp" in c:
        lo, hi = c["xexp"]
        X = (X.double() * torch.exp2(torch.linspace(lo, hi, M, device=DEV).round().double())[:, None]).to(T)
    if "x" in c.get("bad", ""):
        X[1 % M, 3], X[3 % M, 5], X[4 % M, 9] = float("nan"), float("inf"), float("-inf")
    return X


class _Put:
    """Where a run's operands go: an offset copy, or a guarded buffer of the proxy."""

    def __init__(self, c, proxy):
        self.c, self.proxy = c, proxy

    def __call__(self, name, t):
        if t is None:
            return None
        off = grad_cases.offset(self.c, name)
        t = t.to(DEV)
        return self.proxy.place(name, t, off) if self.proxy is not None else forms.at(t, off)

    def empty(self, name, shape, dtype):
        off = grad_cases.offset(self.c, name)
        if self.proxy is not None:
            return self.proxy.place_empty(name, shape, dtype, DEV, off)
        n = 1
        for v in shape:
            n *= v
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        buf = torch.empty(nbytes + 32, dtype=torch.uint8, device=DEV).fill_(0xFF)
        assert buf.data_ptr() % 256 == 0
        return buf[off:off + nbytes].view(dtype).view(shape)


def _placed(c, put):
    w = _memo(("w", _key(c, "M", "xdt", "bias", "xexp", "bad") + (("bad", "w" in c.get("bad", "")),)), lambda: _weight(c))
    return dict(w=put("w", w["w"]), absmax=put("absmax", w["absmax"]), absmax2=put("absmax2", w["absmax2"]), scales=put("scales", w["scales"]),
                bs2=w.get("bs2", 0), Wd=w["Wd"])


def _quant_state(c, ops):
    st2 = None
    if ops["absmax2"] is not None:
        st2 = F.QuantState(absmax=ops["absmax2"], shape=torch.Size([ops["absmax"].numel()]), blocksize=ops["bs2"], quant_type="int8", dtype=torch.float32)
    return F.QuantState(absmax=ops["absmax"], shape=torch.Size([c["N"], c["K"]]), blocksize=c.get("bs", 64), quant_type=c.get("qt", "nf4"),
                        dtype=DT[c["dt"]], state2=st2)


def _abi(c, ops, dY, dX, ws, nbytes, M=None):
    """mbnb_linear_grad_input through ctypes; returns the status."""
    four = c["fmt"] == "4bit"
    desc = None
    if four:
        nested = ops["absmax2"] is not None
        desc = _native.AbsmaxDesc(None if nested else ops["absmax"].data_ptr(), ops["absmax"].data_ptr() if nested else None,
                                  ops["absmax2"].data_ptr() if nested else None, ops["bs2"] if nested else 1)
    code = _native.QUANT_CODE[c["qt"] if "qt" in c else "nf4"] if four else FMT_CODE[c["fmt"]]
    return _native.lib().mbnb_linear_grad_input(
        _native.ptr(dY), c["M"] if M is None else M, c["N"], code, _native.ptr(ops["w"]), None if desc is None else ctypes.byref(desc),
        _native.ptr(ops["scales"]), c["K"], grad_cases.k_weight(c), c.get("bs", 64) if four else 0, _native.DTYPE_CODE[DT[c["dt"]]],
        _native.DTYPE_CODE[dX.dtype], _native.ptr(dX), _native.ptr(ws), nbytes, 0, _native.stream_ptr(DEV))


def _transposed(c, ops):
    if c["fmt"] == "4bit":
        return F._dequantize_t(ops["w"], _quant_state(c, ops))
    if c["fmt"] == "dense":
        return F._dequantize_t(ops["w"], fmt="dense")
    return F._dequantize_t(ops["w"], scales=ops["scales"], fmt=c["fmt"], dtype=DT[c["dt"]])


# ----------------------------------------------------------------------------------------------- the checks
def _reference(c, dYw, Wd):
    """(ref with NaN / +-Inf where expected, bound) in float64 on the device, shared between the runs of a case."""
    def make():
        T, O = DT[c["dt"]], DT[c.get("xdt", c["dt"])]
        Wt = Wd.t().contiguous().to(DEV)                              # [K, N]: the "weight" of dX = dY . Wt^T, contraction length N
        r, bound = linear_bound(dYw, Wt, None, T, O)
        nan, pos, neg = expected_nonfinite(dYw, Wt)
        r = torch.where(nan, torch.full_like(r, float("nan")), torch.where(pos, torch.full_like(r, float("inf")),
                                                                           torch.where(neg, torch.full_like(r, float("-inf")), r)))
        return r, bound
    return _memo(("ref", _key(c, "bias")), make)


def _check_dx(c, dX, dYw, Wd, name, run):
    O = DT[c.get("xdt", c["dt"])]
    assert dX.shape == (c["M"], c["K"]) and dX.dtype == O, (dX.shape, dX.dtype)
    ref, bound = _reference(c, dYw, Wd)
    ratio = assert_bound_elementwise(dX, ref, bound, name, "dX = dY . dequant(W)")
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    first = _memo(("dx", grad_cases.case_id(c)), lambda: _bits(dX))
    assert torch.equal(first, _bits(dX)), f"{grad_cases.case_id(c)} ({run}): dX differs from the first run's: an element was not written"
    return ratio


def _check_dense_bits(c, ops, dY, dX):
    """The dense path against the forward's machinery: the same GEMM on the transposed pass's output."""
    T = DT[c["dt"]]
    Wt = _transposed(c, ops)
    if c.get("ws") == "nosplit":                                      # one slice by the workspace: the plan's tile, not its split
        M, N, K = c["M"], c["N"], c["K"]
        want = torch.empty(M, K, dtype=T, device=DEV).fill_(float("nan"))
        code = _native.DTYPE_CODE[T]
        rc = _native.lib().mbnb_gemm_dense(dY.data_ptr(), Wt.data_ptr(), code, None, code, want.data_ptr(), M, K, N, N, None, 0, 1, _native.stream_ptr(DEV))
        assert rc == 0, _native.lib().mbnb_last_error()
    else:
        want = F.linear_dense(dY, Wt)
    assert torch.equal(_bits(dX), _bits(want.to(dX.dtype))), f"{grad_cases.case_id(c)}: dX differs from linear_dense(dY, Wt)"


def _check_bias(c, b, dYw):
    T = DT[c["dt"]]
    yd = dYw.double()
    ref = yd.sum(0)
    fin = torch.where(torch.isfinite(yd), yd, torch.zeros_like(yd))
    bound = UNIT[T] * torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref)).abs() + (c["M"] + 2) * 2.0 ** -23 * fin.abs().sum(0)
    assert b.grad is not None and b.grad.dtype == T
    assert_bound_elementwise(b.grad.reshape(1, -1), ref.reshape(1, -1), bound.reshape(1, -1), "bias", "bias.grad = sum of dY over rows")


# ----------------------------------------------------------------------------------------------- one run of a case
def _run_grad_t(c, proxy, fill, run):
    put = _Put(c, proxy)
    _sentinel()
    if proxy is not None:
        proxy.begin(fill, [(n, grad_cases.offset(c, n)) for n in grad_cases.PLAN_OPERANDS["grad_t"]], grad_cases.case_id(c))
    ops = _placed(c, put)
    if c["kernel"] == "unsupported":
        with pytest.raises(RuntimeError):
            _transposed(c, ops)
        assert b"transposed pass alone" in _native.lib().mbnb_last_error()
        assert grad_cases.model(c) == ("unsupported", "")
        return
    Wt = _transposed(c, ops)
    got = _record()
    assert got == (c["kernel"], c["variant"]) == grad_cases.model(c), f"{grad_cases.case_id(c)}: the library reports {got}, the model {grad_cases.model(c)}"
    assert Wt.data_ptr() % 16 == (grad_cases.offset(c, "out") if proxy is not None else 0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(Wt), _bits(ops["Wd"].t().contiguous())), f"{grad_cases.case_id(c)} ({run}): the transposed pass differs from the oracle's decode"
    WORST.setdefault("grad_t", 0.0)
    if proxy is not None:
        proxy.check()


def _run_abi(c, proxy, fill, run):
    T, O = DT[c["dt"]], DT[c.get("xdt", c["dt"])]
    put = _Put(c, proxy)
    if proxy is not None:
        proxy.begin(fill, (), grad_cases.case_id(c))
    ops = _placed(c, put)
    dYw = _dy(c)
    dY = put("dy", dYw)
    dX = put.empty("dx", (c["M"], c["K"]), O)
    nbytes = grad_cases.ws_bytes(c)
    if "ws" not in c:
        assert (nbytes or 0) == _native.lib().mbnb_linear_grad_input_workspace_bytes(c["M"], c["N"], c["K"], 0 if c["fmt"] == "4bit" else FMT_CODE[c["fmt"]],
                                                                                   _native.DTYPE_CODE[T]), "the restated workspace query"
    ws = None if nbytes is None else put.empty("ws", (nbytes,), torch.uint8)
    if ws is not None:
        assert ws.data_ptr() % 256 == grad_cases.offset(c, "ws")
    for name, t in (("dy", dY), ("dx", dX), ("w", ops["w"])):
        assert t.data_ptr() % 16 == grad_cases.offset(c, name) % 16, name
    _sentinel()
    n_alloc = None if proxy is None else len(proxy.allocs)
    rc = _abi(c, ops, dY, dX, ws, nbytes or 0)
    assert rc == 0, _native.lib().mbnb_last_error()
    got = _record()
    assert got == (c["kernel"], c["variant"]) == grad_cases.model(c), f"{grad_cases.case_id(c)}: the library reports {got}, the model {grad_cases.model(c)}"
    torch.cuda.synchronize()
    ratio = _check_dx(c, dX, dYw, ops["Wd"], got[0], run)
    if got[0].startswith("grad_t+dense"):
        _check_dense_bits(c, ops, dY, dX)
    if proxy is not None:
        assert n_alloc >= 3
        torch.cuda.synchronize()
        proxy.check()
    return ratio


def _run_autograd(c, proxy, fill, run):
    T, O, fmt = DT[c["dt"]], DT[c.get("xdt", c["dt"])], c["fmt"]
    M, N, K = c["M"], c["N"], c["K"]
    put = _Put(c, proxy)
    if proxy is not None:
        proxy.begin(fill, (), grad_cases.case_id(c))
    ops = _placed(c, put)
    dYw = _dy(c)
    dY = put("dy", dYw)
    placed = None if proxy is None else list(proxy.allocs)
    x = synthetic.normal_device((M, K), O, seed=42).requires_grad_(True)
    b = synthetic.normal_device((N,), T, seed=44).requires_grad_(True) if c.get("bias") else None
    if fmt == "4bit":
        y = F.matmul_4bit(x, ops["w"], _quant_state(c, ops), b, T)
    elif fmt == "int8":
        y = F.linear_int8(x, ops["w"], ops["scales"], b, T)
    else:
        y = F.matmul_fp8_e4m3(x, ops["w"], ops["scales"], b, T)
    assert y.dtype == T
    plan = [(n, grad_cases.offset(c, n)) for n in grad_cases.PLAN_OPERANDS["grad"]]
    seen = []

    def before(g):
        # on autograd's device thread, whose record is its own: the sentinel, then the plan for the backward's own allocations (dX, the
        # workspace); the forward's and the sentinel's allocations are none of this test's business
        _sentinel()
        if proxy is not None:
            proxy.allocs, proxy.plan = list(placed), list(plan)

    y.register_hook(before)
    x.register_hook(lambda g: seen.append(_record()) and None)
    y.backward(dY)
    assert len(seen) == 1, seen
    got = seen[0]
    assert got == (c["kernel"], c["variant"]) == grad_cases.model(c), f"{grad_cases.case_id(c)}: the library reports {got}, the model {grad_cases.model(c)}"
    torch.cuda.synchronize()
    if proxy is not None:
        names = [g.name for g in proxy.allocs[len(placed):]]
        assert names == ["dx", "ws"][:len(names)] and names, names
        assert (len(names) == 2) == (grad_cases.ws_query(c) > 0), (names, got)      # (the query knows no blocksize: 16 gets a workspace it leaves alone)
    ratio = _check_dx(c, x.grad, dYw, ops["Wd"], got[0], run)
    if got[0].startswith("grad_t+dense"):
        _check_dense_bits(c, ops, dY, x.grad)
    if b is not None:
        _check_bias(c, b, dYw)
    if M == 262144:           # past grid.y: the last four rows against the same rows run alone
        alone = torch.empty(4, K, dtype=O, device=DEV).fill_(float("nan"))
        assert _abi(c, ops, dY[-4:].contiguous(), alone, None, 0, M=4) == 0, _native.lib().mbnb_last_error()
        assert torch.equal(_bits(x.grad[-4:]), _bits(alone))
    if proxy is not None:
        torch.cuda.synchronize()
        proxy.check()
    return ratio


def _run(c, proxy=None, fill=None):
    run = "poisoned" if proxy is None else f"guarded, fill 0x{fill:02X}"
    return {"grad_t": _run_grad_t, "grad_abi": _run_abi, "grad": _run_autograd}[c["op"]](c, proxy, fill, run)


@pytest.mark.parametrize("case", [c for c in grad_cases.CASES if not grad_cases.needs_plan(c)], ids=grad_cases.case_id)
def test_case_poisoned(case, poisoned_alloc):
    _run(case)
    assert poisoned_alloc.poisoned > 0


@pytest.mark.parametrize("fill", guard.FILLS, ids=lambda f: f"fill{f:02X}")
@pytest.mark.parametrize("case", grad_cases.CASES, ids=grad_cases.case_id)
def test_case_guarded(case, fill, guarded_alloc):
    _run(case, guarded_alloc, fill)
    assert guarded_alloc.allocs, "nothing went through the guarded proxy"


# ----------------------------------------------------------------------------------------------- autograd and the modules
def _elementwise(xgrad, g, Wd, T, name):
    """x.grad against the float64 product of g.to(T) [rows, N] and Wd [N, K] (the library's dequantise, held against the oracle elsewhere)."""
    gw = g.reshape(-1, g.shape[-1]).to(T)
    Wt = Wd.t().contiguous()
    r, bound = linear_bound(gw, Wt, None, T, xgrad.dtype)
    ratio = assert_bound_elementwise(xgrad.reshape(-1, xgrad.shape[-1]), r, bound, name, "x.grad")
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def _nf4(N, K, T, cs=False):
    W = synthetic.normal_device((N, K), T, seed=61, std=0.05)
    packed, st = F.quantize_4bit(W, blocksize=64, compress_statistics=cs, quant_type="nf4")
    return packed, st, F.dequantize_4bit(packed, st)


def _kernel_of(x):
    seen = []
    x.register_hook(lambda g: seen.append(_native.last_kernel()) and None)
    return seen


@pytest.mark.parametrize("how", ["stride0", "transposed", "3d", "1d"])
def test_grad_out_layouts_and_input_ranks(how):
    T, N, K = torch.bfloat16, 160, 72
    packed, st, Wd = _nf4(N, K, T)
    shape = {"stride0": (5, K), "transposed": (5, K), "3d": (2, 3, K), "1d": (K,)}[how]
    x = synthetic.normal_device(shape, T, seed=62).requires_grad_(True)
    seen = _kernel_of(x)
    y = F.matmul_4bit(x, packed, st)
    if how == "stride0":
        y.sum().backward()                                            # an expanded scalar: every stride 0
        g = torch.ones_like(y)
    else:
        g = synthetic.normal_device(tuple(y.shape), T, seed=63)
        if how == "transposed":
            g = synthetic.normal_device((N, 5), T, seed=63).t()
            assert not g.is_contiguous()
        y.backward(g)
    assert seen == ["grad_generic"] and x.grad.shape == x.shape and x.grad.dtype == T
    _elementwise(x.grad.reshape(-1, K), g, Wd, T, "grad_generic")


@pytest.mark.parametrize("xdt", [torch.float32, torch.float16])
def test_linear4bit_nested_bf16_base_under_another_input_dtype(xdt):
    """The common QLoRA setup: x in f32 (autocast off) or f16 over a bf16 base with compress_statistics."""
    T, M, N, K = torch.bfloat16, 5, 160, 200
    lin = torch.nn.Linear(K, N).to(T).to(DEV)
    m = bnb.Linear4bit.from_linear(lin, compress_statistics=True)
    x = synthetic.normal_device((M, K), xdt, seed=64).requires_grad_(True)
    seen = []
    x.register_hook(lambda g: seen.append(_record()) and None)
    y = m(x)
    g = synthetic.normal_device(tuple(y.shape), y.dtype, seed=65)
    y.backward(g)
    want = f"grad_generic nf4 bf16>{'f32' if xdt == torch.float32 else 'f16'} nested"
    assert seen == [("grad_generic", want)] and x.grad.dtype == xdt
    _elementwise(x.grad, g, m.dequantize(), T, "grad_generic")


@pytest.mark.parametrize("rows", [8, 512])
def test_linear8bit_both_branches(rows):
    """8 rows: linear_int8's backward; 512 rows of 4096 outputs: the cached dequantised weight through linear_dense's (the dense format)."""
    T, N, K = torch.float16, 4096, 128
    lin = torch.nn.Linear(K, N).to(T).to(DEV)
    m = bnb.Linear8bit.from_linear(lin)
    assert F.dense_path_applies(512, N, K) and not F.dense_path_applies(8, N, K)
    x = synthetic.normal_device((rows, K), T, seed=66).requires_grad_(True)
    seen = _kernel_of(x)
    y = m(x)
    g = synthetic.normal_device(tuple(y.shape), T, seed=67)
    y.backward(g)
    assert len(seen) == 1 and seen[0].startswith("grad_t+dense"), seen
    _elementwise(x.grad, g, F.dequantize_rowwise(m.weight_int8, m.weight_scales, T), T, seen[0])


def test_linear_fp8():
    T, M, N, K = torch.bfloat16, 5, 127, 72
    lin = torch.nn.Linear(K, N).to(T).to(DEV)
    m = bnb.LinearFP8.from_linear(lin)
    x = synthetic.normal_device((M, K), T, seed=68).requires_grad_(True)
    seen = _kernel_of(x)
    y = m(x)
    g = synthetic.normal_device(tuple(y.shape), y.dtype, seed=69)
    y.backward(g)
    assert seen == ["grad_generic"]
    _elementwise(x.grad, g, F.dequantize_fp8_e4m3(m.weight_fp8, m.weight_scales, T), T, "grad_generic")


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32])
def test_no_rows_give_a_zero_row_gradient_and_no_launch(xdt):
    T, N, K = torch.bfloat16, 160, 72
    packed, st, _ = _nf4(N, K, T)
    x = torch.empty(0, K, dtype=xdt, device=DEV).requires_grad_(True)
    seen = []
    y = F.matmul_4bit(x, packed, st)
    y.register_hook(lambda g: _sentinel())
    x.register_hook(lambda g: seen.append(_record()) and None)
    y.backward(torch.empty(0, N, dtype=y.dtype, device=DEV))
    assert x.grad.shape == (0, K) and x.grad.dtype == xdt
    assert seen == [("embedding8", "")], f"M = 0 launches nothing and names nothing: {seen}"


def test_zz_report_the_worst_ratio_per_kernel():
    for name, ratio in sorted(WORST.items()):
        print(f"\ngrad forms: {name}: worst err / bound {ratio:.3g}")
    assert all(ratio <= 1.0 for ratio in WORST.values())
