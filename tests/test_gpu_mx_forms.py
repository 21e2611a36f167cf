"""Every form and limit of libmbnb_mx.so on guarded buffers (the tables: tests/mx_cases.py, closed on the CPU by
tests/test_mx_host.py).  The reference for everything is tests/mx_emul.py in float64:

  A  scale bytes from one end of E8M0 to the other on both operands, exact; results that overflow f32 / f16 or fall below 2^-126
  B  every finite E4M3 code at every k of the K-step, bit for bit
  C  NaN / Inf blocks at every fragment place of the row and column masks, in every k block
  D  K % 128 == 64          E  the (x, bias, out, activation) dtype cross
  F  the three entry points through the C ABI on guard-banded operands at the offsets the ABI allows
  G  random data at more shapes, dtypes and a heavy-tailed activation, inside test_gpu_mx.py's bound as it stands
  H  views, misaligned and float64 tensors, M = 0, a side stream, a captured graph
  I  a problem whose activation codes, rows and bytes pass 2^31

Every linear runs inside guard bands under the fills 0xFF and 0x00 with a workspace exactly mbnb_mx_workspace_bytes long."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _mx_native as mxn, _native
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import elementwise, guard, mx_cases as cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _mx_bound, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)
TM, TN, KS = cases.TM, cases.TN, cases.KS
NO_OFFSETS = dict(w_scales=0, out=0, bias=0, workspace=0)


def _name(v):
    return str(v).replace("torch.", "")


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _placed(name, t, fill, offset_bytes):
    """a copy of the CPU tensor `t` on the device inside guard bands, `offset_bytes` off a 16-byte boundary"""
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def run_linear(x, w_codes, w_scales, act, bias, out_dtype, fill, offsets=None):
    """mbnb_mx_linear through the C ABI, every operand the ABI lets move carved at its offset (w_scales in bytes, out and bias in
    elements, the workspace in bytes) -> (y on the CPU, the activation codes and scale bytes the kernel left in the workspace)"""
    off = dict(NO_OFFSETS, **(offsets or {}))
    lib = mxn.lib()
    M, K = x.shape
    N = w_codes.shape[0]
    xd, wc = x.to(DEV).contiguous(), torch.from_numpy(w_codes).to(DEV)
    wsc = _placed("w_scales", torch.from_numpy(w_scales), fill, off["w_scales"])
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    out = guard._carve("out", (M, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
    need = int(lib.mbnb_mx_workspace_bytes(M, K, mxn.ELEM_CODE[act]))
    ws = guard._carve("workspace", (need,), torch.uint8, DEV, fill, off["workspace"])
    st = lib.mbnb_mx_linear(ptr(xd), M, K, _native.DTYPE_CODE[xd.dtype], ptr(wc), ptr(wsc.view), N, mxn.ELEM_CODE[act],
                            None if b is None else ptr(b.view), 0 if b is None else _native.DTYPE_CODE[bias.dtype], ptr(out.view),
                            _native.DTYPE_CODE[out_dtype], ptr(ws.view), need, stream_ptr(DEV))
    mxn.check(st, "linear")
    torch.cuda.synchronize()
    for g in (out, ws, wsc) + (() if b is None else (b,)):
        assert g.violation() is None, (g.name, g.violation(), (M, N, K, act, out_dtype, fill, off))
    assert mxn.last_launch() == f"mx_quant {act} + gemm_mx {act} {TM}x{TN}"
    cbytes = M * K // 2 if act == "fp4" else M * K
    r256 = (cbytes + 255) // 256 * 256
    a_codes = ws.view[:cbytes].cpu().numpy().reshape(M, -1)
    a_scales = ws.view[r256:r256 + M * K // 32].cpu().numpy().reshape(M, K // 32)
    return out.view.cpu().clone(), a_codes, a_scales


def _exact_run(x64, x_dtype, w_codes, w_scales, act, bias64, bias_dtype, out_dtype, what, fills=FILLS, offsets=None, want=None):
    """run the linear under `fills`; the workspace must hold the emulation's codes and bytes and y its float64 result rounded once"""
    xa_codes, xa_scales = emul.quantize(x64, act)
    if want is None:
        want = _round_once(emul.linear_f64(xa_codes, xa_scales, act, w_codes, w_scales, bias64), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, bias_dtype)
    y = None
    for fill in fills:
        y, a_codes, a_scales = run_linear(cases.to_dtype(x64, x_dtype), w_codes, w_scales, act, bias, out_dtype, fill, offsets)
        assert (a_scales == xa_scales).all(), (what, np.argwhere(a_scales != xa_scales)[:4], a_scales[a_scales != xa_scales][:4])
        assert (a_codes == xa_codes).all(), (what, np.argwhere(a_codes != xa_codes)[:4])
        _assert_bits(y, want, f"{what}, fill {fill:#x}")
    return y


# ----------------------------------------------------------------------------- A. wide scales
@pytest.mark.parametrize("index", range(len(cases.WIDE_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.WIDE_CASES[i]))
def test_wide_scale_gemm_bit_for_bit(index):
    case = cases.WIDE_CASES[index]
    _, _, _, act, x_dtype, out_dtype, _ = case
    x64, w64, w_codes, w_scales, _, _ = cases.wide_operands(case, index)
    y = _exact_run(x64, x_dtype, w_codes, w_scales, act, None, None, out_dtype, f"wide {case}")
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("act", ("fp8", "fp4"))
@pytest.mark.parametrize("index", range(len(cases.RANGE_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.RANGE_CASES[i][:1] + cases.RANGE_CASES[i][6:]))
def test_results_outside_the_normal_f32_range(index, act):
    """Sums of 2^128 and more come out as +-Inf and never NaN, an f32 sum beyond f16 as +-Inf by the one rounding, and a sum below
    2^-126 as cases.SUBNORMAL_RESULTS_KEPT states (measured), the same for both activation formats."""
    case = cases.RANGE_CASES[index]
    name, _, _, _, _, _, x_dtype, out_dtype = case
    x64, w64, w_codes, w_scales = cases.range_operands(case, index)
    r = x64 @ w64.T
    want = cases.expected_range_output(r, out_dtype)
    y, _, _ = run_linear(cases.to_dtype(x64, x_dtype), w_codes, w_scales, act, None, out_dtype, FILLS[0])
    if name == "subnormal":
        kept = int((y.double().numpy() == r).sum())
        zeros = int(((y == 0) & (torch.from_numpy(np.signbit(y.numpy()) == (r < 0)))).sum())
        print(f"mx subnormal results, {act}, x {x_dtype}: {kept} of {r.size} kept exactly, {zeros} zeros of the result's sign")
    assert not bool(torch.isnan(y).any()), (name, act, int(torch.isnan(y).sum()))
    _exact_run(x64, x_dtype, w_codes, w_scales, act, None, None, out_dtype, f"{name} {act}", want=want)


# ----------------------------------------------------------------------------- B. every E4M3 code
@pytest.mark.parametrize("index", range(len(cases.FP8_CODE_CASES)), ids=lambda i: "x".join(map(str, cases.FP8_CODE_CASES[i])))
def test_every_e4m3_code_at_every_k_of_the_step(index):
    case = cases.FP8_CODE_CASES[index]
    x, codes, w_codes, w_scales = cases.fp8_code_operands(case)
    want = _round_once(emul.linear_f64(codes, np.full((case[0], case[2] // 32), 127, dtype=np.uint8), "fp8", w_codes, w_scales), torch.float32)
    for fill in FILLS:
        y, a_codes, a_scales = run_linear(torch.from_numpy(x), w_codes, w_scales, "fp8", None, torch.float32, fill)
        assert (a_scales == 127).all() and (a_codes == codes).all()
        _assert_bits(y, want, f"E4M3 codes {case}, fill {fill:#x}")


# ----------------------------------------------------------------------------- C. the NaN masks
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_nan_masks_at_every_fragment_place_and_k_block(act):
    M, N, K = cases.NAN_M, cases.NAN_N, cases.NAN_K
    x64, w64 = cases.nan_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    x = cases.to_dtype(x64, torch.bfloat16)
    places = torch.tensor(cases.NAN_PLACES)
    keep = torch.ones(M, dtype=torch.bool)
    keep[places] = False

    def planted_x(run):
        xb, want_ff = x.clone(), np.zeros((M, K // 32), dtype=bool)
        for p, b, e, v in run:
            xb[p, 32 * b + e] = v
            want_ff[p, b] = True
        return xb, want_ff

    def planted_w(run):
        wsb = w_scales.copy()
        for p, b, _, _ in run:
            wsb[p, b] = 255
        return wsb

    clean, _, _ = run_linear(x, w_codes, w_scales, act, None, torch.float32, FILLS[0])
    _assert_bits(clean, _round_once(x64 @ w64.T, torch.float32), "clean run")
    for r, run in enumerate(cases.NAN_PLAN):
        xb, want_ff = planted_x(run)
        y, _, a_scales = run_linear(xb, w_codes, w_scales, act, None, torch.float32, FILLS[r % 2])
        assert ((a_scales == 255) == want_ff).all(), (r, np.argwhere((a_scales == 255) != want_ff)[:4])
        assert bool(torch.isnan(y[places]).all()), (act, r, "rows", [int(p) for p in places if not bool(torch.isnan(y[p]).all())])
        _assert_bits(y[keep], clean[keep], f"run {r}: rows beside the planted ones")
        y, _, _ = run_linear(x, w_codes, planted_w(run), act, None, torch.float32, FILLS[(r + 1) % 2])
        assert bool(torch.isnan(y[:, places]).all()), (act, r, "columns", [int(p) for p in places if not bool(torch.isnan(y[:, p]).all())])
        _assert_bits(y[:, keep], clean[:, keep], f"run {r}: columns beside the planted ones")
    xb, _ = planted_x(cases.NAN_PLAN[3])
    y, _, _ = run_linear(xb, w_codes, planted_w(cases.NAN_PLAN[8]), act, None, torch.float32, FILLS[0])
    assert bool(torch.isnan(y[places]).all()) and bool(torch.isnan(y[:, places]).all())
    _assert_bits(y[keep][:, keep], clean[keep][:, keep], "rows and columns at once")


# ----------------------------------------------------------------------------- D. K % 128 == 64
@pytest.mark.parametrize("act", ("fp8", "fp4"))
@pytest.mark.parametrize("K", (64, 192))
def test_exact_gemm_where_half_the_last_k_step_stays(K, act):
    for index, case in enumerate(cases.K64_CASES):
        if case[2:] != (K, act):
            continue
        x64, w64 = cases.k64_operands(case, index)
        w_codes, w_scales = emul.quantize(w64, "fp4")
        x_dtype, out_dtype = cases.X_DTYPES[index % 3], cases.OUT_DTYPES[(index // 3) % 3]
        y = _exact_run(x64, x_dtype, w_codes, w_scales, act, None, None, out_dtype, f"K64 {case}")
        assert (y.double().numpy() == x64 @ w64.T).all() or out_dtype != torch.float32


# ----------------------------------------------------------------------------- E. the dtype cross
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_every_x_bias_and_output_dtype_together(act):
    x64, w64, bias64 = cases.cross_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    n = 0
    for i, (xd, bd, od, a) in enumerate(cases.CROSS_CASES):
        if a != act:
            continue
        _exact_run(x64, xd, w_codes, w_scales, act, None if bd is None else bias64, bd, od, f"cross x {xd}, bias {bd}, out {od}, {act}",
                   fills=(FILLS[i % 2],))
        n += 1
    assert n == 36


# ----------------------------------------------------------------------------- F. guarded, offset operands
@pytest.mark.parametrize("elem", ("fp4", "fp8"))
def test_quantize_and_dequantize_abi_on_guarded_offset_buffers(elem):
    lib = mxn.lib()
    for si, (rows, K) in enumerate(cases.ABI_SHAPES):
        for di, dtype in enumerate(cases.X_DTYPES):
            kind = cases.QUANT_KINDS[(si + di) % len(cases.QUANT_KINDS)]
            x = cases.quantiser_input(kind, elem, dtype, rows, K)
            want_codes, want_scales = emul.quantize(cases.as_f32(x), elem)
            want_out = _round_once(emul.decode_f64(want_codes, want_scales, elem), dtype)
            xd = x.to(DEV)
            for fill in FILLS:
                for so in cases.SCALE_OFFSETS:
                    where = (elem, rows, K, dtype, kind, fill, so)
                    codes = guard._carve("codes", want_codes.shape, torch.uint8, DEV, fill, 0)
                    scales = guard._carve("scales", want_scales.shape, torch.uint8, DEV, fill, so)
                    mxn.check(lib.mbnb_mx_quantize(ptr(xd), rows, K, _native.DTYPE_CODE[dtype], mxn.ELEM_CODE[elem], ptr(codes.view),
                                                   ptr(scales.view), stream_ptr(DEV)), "quantize")
                    torch.cuda.synchronize()
                    assert codes.violation() is None and scales.violation() is None, (where, codes.violation(), scales.violation())
                    assert mxn.last_launch() == f"mx_quant {elem}"
                    assert (scales.view.cpu().numpy() == want_scales).all() and (codes.view.cpu().numpy() == want_codes).all(), where
                    out = guard._carve("out", (rows, K), dtype, DEV, fill, 0)
                    mxn.check(lib.mbnb_mx_dequantize(ptr(codes.view), ptr(scales.view), rows, K, mxn.ELEM_CODE[elem], _native.DTYPE_CODE[dtype],
                                                     ptr(out.view), stream_ptr(DEV)), "dequantize")
                    torch.cuda.synchronize()
                    for g in (codes, scales, out):
                        assert g.violation() is None, (where, g.name, g.violation())
                    assert mxn.last_launch() == f"mx_dequant {elem}"
                    _assert_bits(out.view.cpu(), want_out, f"dequantize {where}")


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_linear_with_every_operand_off_its_boundary(act):
    for shape_index, (M, N, K) in enumerate(((17, 19, 160), (TM + 1, TN + 1, 192))):
        x64, w64 = emul.lossless(M, K, seed=7101 + shape_index), emul.lossless(N, K, seed=7111 + shape_index)
        bias64 = np.random.default_rng(7121).integers(-8, 9, size=N).astype(np.float64)
        w_codes, w_scales = emul.quantize(w64, "fp4")
        for di, dtype in enumerate(cases.OUT_DTYPES):
            base = _exact_run(x64, cases.X_DTYPES[(di + 1) % 3], w_codes, w_scales, act, bias64, dtype, dtype, "offset 0", fills=FILLS[:1])
            for oi, off in enumerate(cases.LINEAR_OFFSETS):
                y = _exact_run(x64, cases.X_DTYPES[(di + 1) % 3], w_codes, w_scales, act, bias64, dtype, dtype, f"offsets {off}",
                               fills=(FILLS[oi % 2], FILLS[(oi + 1) % 2]), offsets=off)
                _assert_bits(y, base, f"offsets {off} against offset 0")


# ----------------------------------------------------------------------------- G. random data
_RANDOM = {}


def _random_reference(x_dtype, kind, act):
    """the operands, the emulation's quantised activation and the float64 reference of a random case, computed once"""
    key = (x_dtype, kind, act)
    if key not in _RANDOM:
        x, w, bias = cases.random_operands(x_dtype, kind)
        if "w" not in _RANDOM:
            _RANDOM["w"] = emul.quantize(cases.as_f32(w), "fp4")
        w_codes, w_scales = _RANDOM["w"]
        xa_codes, xa_scales = emul.quantize(cases.as_f32(x), act)
        xq, wq = emul.decode_f64(xa_codes, xa_scales, act), emul.decode_f64(w_codes, w_scales, "fp4")
        _RANDOM[key] = (x, bias, w_codes, w_scales, xa_codes, xa_scales, xq, wq)
    return _RANDOM[key]


@pytest.mark.parametrize("index", range(len(cases.RANDOM_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.RANDOM_CASES[i]))
def test_random_data_at_more_places_inside_the_same_bound(index):
    x_dtype, out_dtype, act, kind = cases.RANDOM_CASES[index]
    x, bias, w_codes, w_scales, xa_codes, xa_scales, xq, wq = _random_reference(x_dtype, kind, act)
    r, bound = _mx_bound(xq, wq, bias, out_dtype)
    none = torch.zeros(r.shape, dtype=torch.bool)
    y, a_codes, a_scales = run_linear(x, w_codes, w_scales, act, bias, out_dtype, FILLS[index % 2])
    assert (a_codes == xa_codes).all() and (a_scales == xa_scales).all()
    if kind == "heavy":
        assert int(np.ptp(xa_scales.astype(np.int64), axis=1).min()) >= 4            # the block bytes spread within every row
    ratio = elementwise._compare(y, r, bound, none, none, none, mxn.last_launch(), "y = Q(x) . W^T + b")
    print(f"mx random {kind} {act}, x {x_dtype} -> {out_dtype}: worst err / bound = {ratio:.4f}")


# ----------------------------------------------------------------------------- H. the Python surface and the execution context
def _surface_operands():
    x64, w64, bias64 = cases.cross_operands()
    w_codes, w_scales = emul.quantize(w64, "fp4")
    return x64, w64, bias64, torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_views_misaligned_and_float64_tensors_equal_the_plain_call(act, monkeypatch):
    M, N, K = cases.CROSS_SHAPE
    x64, w64, bias64, wc, wsc = _surface_operands()
    x = cases.to_dtype(x64, torch.bfloat16).to(DEV)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    plain = bnb.matmul_mxfp4(x, wc, wsc, bias, act_format=act)
    _assert_bits(plain.cpu(), _round_once(x64 @ w64.T + bias64, torch.bfloat16), "the plain call")
    # a transposed view
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(xt, x)
    _assert_bits(bnb.matmul_mxfp4(xt, wc, wsc, bias, act_format=act).cpu(), plain.cpu(), "transposed view")
    # rows sliced out of a tensor that starts one element off a 16-byte boundary
    flat = torch.zeros((M + 1) * K + 8, dtype=torch.bfloat16, device=DEV)
    xs = flat[1:1 + (M + 1) * K].view(M + 1, K)[1:]
    xs.copy_(x)
    assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
    _assert_bits(bnb.matmul_mxfp4(xs, wc, wsc, bias, act_format=act).cpu(), plain.cpu(), "misaligned row slice")
    codes, scales = bnb.quantize_mx(xs, act)
    want_codes, want_scales = emul.quantize(x64, act)
    assert (codes.cpu().numpy() == want_codes).all() and (scales.cpu().numpy() == want_scales).all()
    # a weight view off a 16-byte boundary, and a strided scales view
    wflat = torch.zeros(N * K // 2 + 16, dtype=torch.uint8, device=DEV)
    wv = wflat[1:1 + N * K // 2].view(N, K // 2)
    wv.copy_(wc)
    sv = torch.zeros(N, 2 * (K // 32), dtype=torch.uint8, device=DEV)[:, ::2]
    sv.copy_(wsc)
    assert wv.data_ptr() % 16 != 0 and not sv.is_contiguous()
    _assert_bits(bnb.matmul_mxfp4(x, wv, sv, bias, act_format=act).cpu(), plain.cpu(), "misaligned weight view")
    _assert_bits(bnb.dequantize_mx(wv, sv, "fp4", torch.float32).cpu(), _round_once(w64, torch.float32), "dequantize_mx of the views")
    # float64 input and bias are read as f32
    y32 = bnb.matmul_mxfp4(x.float(), wc, wsc, bias.float(), act_format=act, dtype=torch.float32)
    y64 = bnb.matmul_mxfp4(x.double(), wc, wsc, bias.double(), act_format=act, dtype=torch.float32)
    _assert_bits(y32.cpu(), _round_once(x64 @ w64.T + bias64, torch.float32), "f32 in, f32 out")
    _assert_bits(y64.cpu(), y32.cpu(), "float64 input and bias")
    c64, s64 = bnb.quantize_mx(x.double(), act)
    assert torch.equal(c64, codes) and torch.equal(s64, scales)
    # M = 0: the right empty shape, and the library is not called at all
    def no_library():
        raise AssertionError("the library was called for an empty input")
    monkeypatch.setattr(mxn, "lib", no_library)
    y = bnb.matmul_mxfp4(x[:0], wc, wsc, bias, act_format=act)
    assert tuple(y.shape) == (0, N) and y.dtype == torch.bfloat16 and y.device == x.device
    y = bnb.matmul_mxfp4(x[:0].reshape(2, 0, K), wc, wsc, None, act_format=act, dtype=torch.float16)
    assert tuple(y.shape) == (2, 0, N) and y.dtype == torch.float16


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_side_stream_and_captured_graph_equal_the_eager_call(act):
    M, N, K = cases.CROSS_SHAPE
    x64, w64, bias64, wc, wsc = _surface_operands()
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    layer = bnb.LinearMXFP4(K, N, act_format=act, device=DEV)
    layer.load_state_dict({"weight": wc, "weight_scales": wsc, "bias": bias})
    inputs = [cases.to_dtype(emul.lossless(M, K, seed=7201 + i), torch.bfloat16).to(DEV) for i in range(3)]
    with torch.no_grad():
        eager = [(bnb.matmul_mxfp4(xin, wc, wsc, bias, act_format=act).clone(), layer(xin).clone()) for xin in inputs]
        for xin, (a, b) in zip(inputs, eager):
            _assert_bits(a.cpu(), _round_once(xin.double().cpu().numpy() @ w64.T + bias64, torch.bfloat16), "eager")
            assert torch.equal(a, b)
        torch.cuda.synchronize()
        # a side stream
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ys = (bnb.matmul_mxfp4(inputs[1], wc, wsc, bias, act_format=act), layer(inputs[1]))
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        assert torch.equal(ys[0], eager[1][0]) and torch.equal(ys[1], eager[1][1])
        # a captured graph, replayed after x is overwritten in place
        A = inputs[0].clone()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            bnb.matmul_mxfp4(A, wc, wsc, bias, act_format=act)          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = (bnb.matmul_mxfp4(A, wc, wsc, bias, act_format=act), layer(A))
        for xin, want in zip(inputs[::-1], eager[::-1]):
            A.copy_(xin)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])


# ----------------------------------------------------------------------------- I. past 2^31
def test_rows_and_bytes_past_2_to_the_31():
    """fp8 activations, 65665 x 32768: the quantiser's input index, the activation codes and (m0 + row) * lda all pass 2^31.  Row r of
    x is row r % 251 of a lossless pattern, so a 32-bit wrap of any of them would land on a row with other contents."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs about 7 GiB of device memory; {free / 2 ** 30:.1f} GiB free")
    M, N, K, P = cases.BIG_M, cases.BIG_N, cases.BIG_K, cases.BIG_PATTERN
    assert (M - 129) * K == 2 ** 31 and cases.BIG_ROWS[-140] < 65536 < cases.BIG_ROWS[-1]      # the checked rows straddle 2^31 bytes of codes
    pat64, w64 = emul.lossless(P, K, seed=9001), emul.lossless(N, K, seed=9002)
    assert (np.abs(pat64) @ np.abs(w64).T).max() < 2.0 ** 20                        # multiples of 2^-4 below 2^20: exact in any order
    w_codes, w_scales = emul.quantize(w64, "fp4")
    pat_codes, pat_scales = emul.quantize(pat64, "fp8")
    pat_out = _round_once(emul.linear_f64(pat_codes, pat_scales, "fp8", w_codes, w_scales), torch.float32)
    pat = cases.to_dtype(pat64, torch.bfloat16).to(DEV)
    x = pat[torch.arange(M, device=DEV) % P]
    assert x.is_contiguous() and x.numel() * 2 > 2 ** 32
    lib = mxn.lib()
    need = int(lib.mbnb_mx_workspace_bytes(M, K, mxn.FP8))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    wc, wsc = torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)
    mxn.check(lib.mbnb_mx_linear(ptr(x), M, K, _native.DTYPE_CODE[x.dtype], ptr(wc), ptr(wsc), N, mxn.FP8, None, 0, ptr(out),
                                 _native.DTYPE_CODE[torch.float32], ptr(ws), need, stream_ptr(DEV)), "linear")
    torch.cuda.synchronize()
    del x
    rows = torch.tensor(cases.BIG_ROWS)
    src = (rows % P).numpy()
    codes = ws[:M * K].view(M, K)
    r256 = (M * K + 255) // 256 * 256
    scales = ws[r256:r256 + M * (K // 32)].view(M, K // 32)
    dev_rows = rows.to(DEV)
    assert (scales[dev_rows].cpu().numpy() == pat_scales[src]).all(), "scale bytes of the checked rows"
    assert (codes[dev_rows].cpu().numpy() == pat_codes[src]).all(), "codes of the checked rows"
    _assert_bits(out[dev_rows].cpu(), pat_out[torch.from_numpy(src)], "output rows past 2^31 bytes of codes")
    deq = bnb.dequantize_mx(codes, scales, "fp8", torch.bfloat16)
    _assert_bits(deq[dev_rows].cpu(), cases.to_dtype(pat64[src], torch.bfloat16), "dequantize_mx past 2^31")
