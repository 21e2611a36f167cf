"""The weight-only MXFP4 decode linear (k_mx_decode) through the C ABI on guard-banded buffers under the fills 0xFF
and 0x00, and through the Python surface.  The tables are tests/mx_decode_cases.py (closed on the CPU by
tests/test_mx_decode_host.py); the reference for everything is float64 over tests/mx_emul.py's decode, rounded once.

  A  lossless operands at every M, N and K edge: bit-equal
  B  scale bytes from one end of E8M0 to the other, a result below 2^-126
  C  0xFF scale bytes, and Inf / NaN activations
  D  random data inside the project's elementwise bound      E  the dtype cross
  F  every operand off its boundary                           G  the Python surface, streams, a captured graph, the composed route
  H  the accuracy against the quantising route"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _mx_native as mxn, _native
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import elementwise, guard, mx_cases, mx_decode_cases as cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _mx_bound, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)
NO_OFFSETS = dict(x=0, w_codes=0, w_scales=0, out=0, bias=0)


def _name(v):
    return str(v).replace("torch.", "")


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _placed(name, t, fill, offset_bytes):
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def run_decode(x, w_codes, w_scales, bias, out_dtype, fill, offsets=None):
    """mbnb_mx_linear_weight_only through the C ABI, every operand carved inside guard bands at its offset (x, w_codes and w_scales in
    bytes, out and bias in elements) -> y on the CPU"""
    off = dict(NO_OFFSETS, **(offsets or {}))
    lib = mxn.lib()
    M, K = x.shape
    N = w_codes.shape[0]
    xg = _placed("x", x.contiguous(), fill, off["x"])
    wc = _placed("w_codes", torch.from_numpy(w_codes), fill, off["w_codes"])
    wsc = _placed("w_scales", torch.from_numpy(w_scales), fill, off["w_scales"])
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    out = guard._carve("out", (M, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
    st = lib.mbnb_mx_linear_weight_only(ptr(xg.view), M, K, _native.DTYPE_CODE[x.dtype], ptr(wc.view), ptr(wsc.view), N,
                                        None if b is None else ptr(b.view), 0 if b is None else _native.DTYPE_CODE[bias.dtype],
                                        ptr(out.view), _native.DTYPE_CODE[out_dtype], stream_ptr(DEV))
    mxn.check(st, "linear_weight_only")
    torch.cuda.synchronize()
    for g in (out, xg, wc, wsc) + (() if b is None else (b,)):
        assert g.violation() is None, (g.name, g.violation(), (M, N, K, x.dtype, out_dtype, fill, off))
    assert mxn.last_launch() == cases.launch_text(M, x.dtype), mxn.last_launch()
    return out.view.cpu().clone()


def _exact_run(x64, x_dtype, w_codes, w_scales, bias64, bias_dtype, out_dtype, what, fills=FILLS, offsets=None, want=None):
    if want is None:
        r = x64 @ emul.decode_f64(w_codes, w_scales, "fp4").T + (0 if bias64 is None else bias64[None, :])
        want = _round_once(r, out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, bias_dtype)
    y = None
    for fill in fills:
        y = run_decode(cases.to_dtype(x64, x_dtype), w_codes, w_scales, bias, out_dtype, fill, offsets)
        _assert_bits(y, want, f"{what}, fill {fill:#x}")
    return y


# ----------------------------------------------------------------------------- A. exact
@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.EXACT_CASES[i]))
def test_lossless_operands_bit_for_bit(index):
    case = cases.EXACT_CASES[index]
    _, _, _, x_dtype, out_dtype, _ = case
    x64, w64, bias64 = cases.exact_operands(case, index)
    w_codes, w_scales = emul.quantize(w64, "fp4")
    _exact_run(x64, x_dtype, w_codes, w_scales, bias64, cases.DTYPES[index % 3], out_dtype, f"exact {case}")


# ----------------------------------------------------------------------------- B. scale bytes
@pytest.mark.parametrize("index", range(len(cases.WIDE_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.WIDE_CASES[i]))
def test_scale_bytes_from_end_to_end_bit_for_bit(index):
    case = cases.WIDE_CASES[index]
    _, _, _, x_dtype, out_dtype, _ = case
    x64, w64, w_codes, w_scales, _, _ = cases.wide_operands(case, index)
    y = _exact_run(x64, x_dtype, w_codes, w_scales, None, None, out_dtype, f"wide {case}", want=_round_once(x64 @ w64.T, out_dtype))
    assert bool(torch.isfinite(y).all()) and bool((y != 0).all())


@pytest.mark.parametrize("which", range(len(cases.SUBNORMAL_CASES)))
def test_a_result_below_the_normal_range(which):
    """What the f32 FMA leaves of a sum below 2^-126 is cases.SUBNORMAL_RESULTS_KEPT, a measured fact."""
    index, case = cases.SUBNORMAL_CASES[which]
    x64, w64, w_codes, w_scales = mx_cases.range_operands(case, index)
    r = x64 @ w64.T
    y = run_decode(cases.to_dtype(x64, case[6]), w_codes, w_scales, None, torch.float32, FILLS[0])
    kept = int((y.double().numpy() == r).sum())
    zeros = int(((y == 0) & torch.from_numpy(np.signbit(y.numpy()) == (r < 0))).sum())
    print(f"mx_decode subnormal results, x {case[6]}: {kept} of {r.size} kept exactly, {zeros} zeros of the result's sign")
    _exact_run(x64, case[6], w_codes, w_scales, None, None, torch.float32, f"subnormal {case}", want=cases.expected_subnormal_output(r))


# ----------------------------------------------------------------------------- C. NaN and Inf
@pytest.mark.parametrize("x_dtype", (torch.bfloat16, torch.float32), ids=_name)
def test_a_nan_scale_byte_makes_its_column_nan_in_every_row(x_dtype):
    M, N, K = cases.NAN_SHAPE
    x64, w64 = cases.nan_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    clean = _exact_run(x64, x_dtype, w_codes, w_scales, None, None, torch.float32, "clean")
    keep = torch.ones(N, dtype=torch.bool)
    keep[cases.NAN_COLUMN] = False
    for i, b in enumerate(cases.NAN_BLOCKS):
        planted = w_scales.copy()
        planted[cases.NAN_COLUMN, b] = 255
        for zero_x in (False, True):
            xb = x64.copy()
            if zero_x:
                xb[:, 32 * b:32 * b + 32] = 0.0
            want = _round_once(xb @ w64.T, torch.float32)
            y = run_decode(cases.to_dtype(xb, x_dtype), w_codes, planted, None, torch.float32, FILLS[(i + zero_x) % 2])
            assert bool(torch.isnan(y[:, cases.NAN_COLUMN]).all()), (b, zero_x, y[:, cases.NAN_COLUMN])
            _assert_bits(y[:, keep], want[:, keep], f"0xFF in block {b}, x block zero: {zero_x}: the other columns")
    planted = w_scales.copy()
    planted[cases.NAN_COLUMN, list(cases.NAN_BLOCKS)] = 255
    planted[0, 1] = 255
    y = run_decode(cases.to_dtype(x64, x_dtype), w_codes, planted, cases.to_dtype(np.ones(N), torch.float32), torch.bfloat16, FILLS[0])
    assert bool(torch.isnan(y[:, [0, cases.NAN_COLUMN]]).all())
    keep[0] = False
    _assert_bits(y[:, keep], (clean + 1.0).to(torch.bfloat16)[:, keep], "several 0xFF bytes, a bias: the other columns")


@pytest.mark.parametrize("x_dtype", (torch.bfloat16, torch.float16, torch.float32), ids=_name)
def test_inf_and_nan_activations_propagate_as_ieee_over_the_decoded_weight(x_dtype):
    M, N, K = cases.NAN_SHAPE
    x64, w64 = cases.nan_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    clean = _round_once(x64 @ w64.T, torch.float32)
    other = torch.tensor([m != cases.X_BAD_ROW for m in range(M)])
    n = 0
    for ki, k in enumerate(cases.X_BAD_KS):
        for vi, v in enumerate(cases.X_BAD_VALUES):
            xb = x64.copy()
            xb[cases.X_BAD_ROW, k] = v
            with np.errstate(invalid="ignore"):
                want_row = (xb[cases.X_BAD_ROW][None, :] * w64).sum(axis=1)          # elementwise IEEE: Inf * 0 = NaN, +Inf + -Inf = NaN
            assert not np.isfinite(want_row).any()
            y = run_decode(cases.to_dtype(xb, x_dtype), w_codes, w_scales, None, torch.float32, FILLS[(ki + vi) % 2])
            got = y[cases.X_BAD_ROW].double().numpy()
            assert (np.isnan(got) == np.isnan(want_row)).all() and (got[~np.isnan(want_row)] == want_row[~np.isnan(want_row)]).all(), (k, v, got, want_row)
            _assert_bits(y[other], clean[other], f"{v} at k = {k}: the other rows")
            n += int(np.isinf(want_row).any())
    assert n > 0                                                                      # some weights there are non-zero: +-Inf came through as such


# ----------------------------------------------------------------------------- D. random data
_RANDOM = {}


def _random_reference(shape, x_dtype):
    key = (shape, x_dtype)
    if key not in _RANDOM:
        if shape not in _RANDOM:
            _, w, _ = cases.random_operands(shape, torch.float32)
            codes, scales = bnb.quantize_mxfp4(w.to(DEV))
            codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
            assert all((a == b).all() for a, b in zip((codes, scales), emul.quantize(w.numpy(), "fp4")))
            _RANDOM[shape] = (codes, scales, emul.decode_f64(codes, scales, "fp4"))
        x, _, bias = cases.random_operands(shape, x_dtype)
        _RANDOM[key] = (x, bias) + _RANDOM[shape]
    return _RANDOM[key]


@pytest.mark.parametrize("index", range(len(cases.RANDOM_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.RANDOM_CASES[i]))
def test_random_data_elementwise_against_f64_over_the_decoded_weight(index):
    shape, x_dtype, out_dtype = cases.RANDOM_CASES[index]
    x, bias, w_codes, w_scales, wq = _random_reference(shape, x_dtype)
    r, bound = _mx_bound(x.double().numpy(), wq, bias, out_dtype)
    none = torch.zeros(r.shape, dtype=torch.bool)
    y = run_decode(x, w_codes, w_scales, bias, out_dtype, FILLS[index % 2])
    ratio = elementwise._compare(y, r, bound, none, none, none, mxn.last_launch(), "y = x . W^T + b")
    print(f"mx_decode random {shape}, x {x_dtype} -> {out_dtype}: worst err / bound = {ratio:.4f}")


# ----------------------------------------------------------------------------- E. the dtype cross
def test_every_x_bias_and_output_dtype_together():
    x64, w64, bias64 = cases.cross_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    for i, (xd, bd, od) in enumerate(cases.CROSS_CASES):
        _exact_run(x64, xd, w_codes, w_scales, None if bd is None else bias64, bd, od, f"cross x {xd}, bias {bd}, out {od}", fills=(FILLS[i % 2],))


# ----------------------------------------------------------------------------- F. operand offsets
def test_every_operand_off_its_boundary():
    for si, (M, N, K) in enumerate(cases.OFFSET_SHAPES):
        x64, w64 = emul.lossless(M, K, seed=18001), emul.lossless(N, K, seed=18002)
        bias64 = np.random.default_rng(18003).integers(-8, 9, size=N).astype(np.float64)
        w_codes, w_scales = emul.quantize(w64, "fp4")
        for di, dtype in enumerate(cases.DTYPES):
            xd = cases.DTYPES[(di + 1) % 3]
            base = _exact_run(x64, xd, w_codes, w_scales, bias64, dtype, dtype, "offset 0", fills=FILLS[:1])
            for oi, off in enumerate(cases.OFFSETS):
                y = _exact_run(x64, xd, w_codes, w_scales, bias64, dtype, dtype, f"offsets {off}", fills=(FILLS[(oi + si) % 2],), offsets=off)
                _assert_bits(y, base, f"offsets {off} against offset 0")


# ----------------------------------------------------------------------------- G. the Python surface
def _surface_operands(M=5, N=9, K=cases.CHUNK + 32):
    x64, w64 = emul.lossless(M, K, seed=19001), emul.lossless(N, K, seed=19002)
    bias64 = np.random.default_rng(19003).integers(-8, 9, size=N).astype(np.float64)
    w_codes, w_scales = emul.quantize(w64, "fp4")
    return x64, w64, bias64, torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)


def test_folded_one_dimensional_strided_and_misaligned_inputs():
    M, N, K = 6, 9, cases.CHUNK + 32
    x64, w64, bias64, wc, wsc = _surface_operands(M, N, K)
    x = cases.to_dtype(x64, torch.bfloat16).to(DEV)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    want = _round_once(x64 @ w64.T + bias64, torch.bfloat16)
    plain = bnb.matmul_mxfp4(x, wc, wsc, bias, act_format="none")
    assert mxn.last_launch() == "mx_decode_mfma bf16 MT16"
    _assert_bits(plain.cpu(), want, "the plain call")
    y = bnb.matmul_mxfp4(x.reshape(2, 3, K), wc, wsc, bias, act_format="none")
    assert tuple(y.shape) == (2, 3, N)
    _assert_bits(y.cpu().reshape(M, N), want, "leading dimensions folded")
    y = bnb.matmul_mxfp4(x[2], wc, wsc, act_format="none", dtype=torch.float32)
    assert tuple(y.shape) == (N,) and mxn.last_launch() == "mx_decode bf16 MT1"
    _assert_bits(y.cpu(), _round_once((x64 @ w64.T)[2], torch.float32), "1-D input")
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous()
    _assert_bits(bnb.matmul_mxfp4(xt, wc, wsc, bias, act_format="none").cpu(), want, "transposed view")
    flat = torch.zeros((M + 1) * K + 8, dtype=torch.bfloat16, device=DEV)
    xs = flat[1:1 + (M + 1) * K].view(M + 1, K)[1:]
    xs.copy_(x)
    assert xs.data_ptr() % 16 != 0
    _assert_bits(bnb.matmul_mxfp4(xs, wc, wsc, bias, act_format="none").cpu(), want, "misaligned row slice")
    wflat = torch.zeros(N * K // 2 + 16, dtype=torch.uint8, device=DEV)
    wv = wflat[1:1 + N * K // 2].view(N, K // 2)
    wv.copy_(wc)
    sv = torch.zeros(N, 2 * (K // 32), dtype=torch.uint8, device=DEV)[:, ::2]
    sv.copy_(wsc)
    assert wv.data_ptr() % 16 != 0 and not sv.is_contiguous()
    _assert_bits(bnb.matmul_mxfp4(x, wv, sv, bias, act_format="none").cpu(), want, "misaligned weight view, strided scales")
    y64 = bnb.matmul_mxfp4(x.double(), wc, wsc, bias.double(), act_format="none", dtype=torch.float32)
    _assert_bits(y64.cpu(), _round_once(x64 @ w64.T + bias64, torch.float32), "float64 input and bias read as f32")
    y = bnb.matmul_mxfp4(x[:0], wc, wsc, bias, act_format="none")
    assert tuple(y.shape) == (0, N) and y.dtype == torch.bfloat16


def test_side_stream_captured_graph_and_the_layer():
    M, N, K = 5, 9, cases.CHUNK + 32
    x64, w64, bias64, wc, wsc = _surface_operands(M, N, K)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(cases.to_dtype(w64, torch.bfloat16))
        lin.bias.copy_(bias.cpu())
    layer = bnb.LinearMXFP4.from_linear(lin.to(DEV), act_format="none")
    assert layer.act_format == "none" and torch.equal(layer.weight, wc) and torch.equal(layer.weight_scales, wsc)
    inputs = [cases.to_dtype(emul.lossless(M, K, seed=19101 + i), torch.bfloat16).to(DEV) for i in range(3)]
    with torch.no_grad():
        eager = []
        for xin in inputs:
            a, b = bnb.matmul_mxfp4(xin, wc, wsc, bias, act_format="none").clone(), layer(xin).clone()
            _assert_bits(a.cpu(), _round_once(xin.double().cpu().numpy() @ w64.T + bias64, torch.bfloat16), "eager")
            assert torch.equal(a, b) and mxn.last_launch() == "mx_decode_mfma bf16 MT16"
            eager.append(a)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ys = layer(inputs[1])
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        assert torch.equal(ys, eager[1])
        # one captured graph, a single chain, replayed after x is overwritten in place
        A = inputs[0].clone()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            layer(A)                                                     # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = layer(A)
        for xin, want in zip(inputs[::-1], eager[::-1]):
            A.copy_(xin)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_the_bf16_composed_route_beyond_sixteen_rows():
    M, N, K = cases.COMPOSED_SHAPE
    x64, w64, bias64, wc, wsc = _surface_operands(M, N, K)
    x = cases.to_dtype(x64, torch.bfloat16).to(DEV)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    before = mxn.last_launch()
    y = bnb.matmul_mxfp4(x, wc, wsc, bias, act_format="none")
    assert mxn.last_launch() in (before, "mx_dequant fp4")              # dequantise + the dense GEMM, not k_mx_decode
    _assert_bits(y.cpu(), _round_once(x64 @ w64.T + bias64, torch.bfloat16), "composed route, lossless")
    # the same rows through the launch itself (f32 out keeps it there), and a random case of both routes inside the bound
    y32 = bnb.matmul_mxfp4(x, wc, wsc, bias, act_format="none", dtype=torch.float32)
    assert mxn.last_launch() == "mx_decode_mfma bf16 MT16"
    _assert_bits(y32.cpu(), _round_once(x64 @ w64.T + bias64, torch.float32), "17 rows in one launch")
    g = torch.Generator().manual_seed(19201)
    xr = torch.randn(M, K, generator=g).to(torch.bfloat16)
    codes, scales = emul.quantize((torch.randn(N, K, generator=g) * 0.02).numpy(), "fp4")
    r, bound = _mx_bound(xr.double().numpy(), emul.decode_f64(codes, scales, "fp4"), None, torch.bfloat16)
    none = torch.zeros(r.shape, dtype=torch.bool)
    args = (xr.to(DEV), torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV))
    composed = bnb.matmul_mxfp4(*args, act_format="none")
    assert mxn.last_launch() == "mx_dequant fp4"
    ratio = elementwise._compare(composed.cpu(), r, bound, none, none, none, "dequantise + dense", "composed route")
    r32, bound32 = _mx_bound(xr.double().numpy(), emul.decode_f64(codes, scales, "fp4"), None, torch.float32)
    direct = bnb.matmul_mxfp4(*args, act_format="none", dtype=torch.float32)
    ratio32 = elementwise._compare(direct.cpu(), r32, bound32, none, none, none, mxn.last_launch(), "the launch, f32 out")
    print(f"mx_decode composed route at {cases.COMPOSED_SHAPE}: worst err / bound = {ratio:.4f}; the launch into f32 = {ratio32:.4f}")


# ----------------------------------------------------------------------------- H. accuracy
def test_weight_only_is_closer_to_the_unquantised_linear_than_the_fp8_route():
    M, N, K = 8, 256, 1024
    g = torch.Generator().manual_seed(19301)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    codes, scales = bnb.quantize_mxfp4(w)
    ref = x.double() @ w.double().t()
    rel = lambda y: float((y.double() - ref).norm() / ref.norm())
    e_none = rel(bnb.matmul_mxfp4(x, codes, scales, act_format="none", dtype=torch.float32))
    e_fp8 = rel(bnb.matmul_mxfp4(x, codes, scales, act_format="fp8", dtype=torch.float32))
    e_weight = rel(x.double() @ bnb.dequantize_mxfp4(codes, scales, torch.float32).double().t())
    print(f"relative Frobenius error against the unquantised linear: none {e_none:.4f}, fp8 {e_fp8:.4f}, the weight alone {e_weight:.4f}")
    assert e_none < e_fp8
    assert abs(e_none - e_weight) < 1e-4
