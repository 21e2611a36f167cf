"""GPU checks of libmbnb_mx.so against the numpy emulation of the OCP MX format (tests/mx_emul.py): the quantiser and the decoder bit
for bit, the lane map of the block-scaled MFMA on an identity activation, the GEMM bit for bit on lossless operands (whose f32
accumulation is exact in any order: tests/test_mx_host.py asserts it for every case), random data element by element against
float64 over the emulation's quantised operands, and non-finite blocks.

The linear's output and workspace sit inside larger buffers filled with 0xFF for one run and 0x00 for the other; the bands around
them must come back untouched and the workspace is exactly mbnb_mx_workspace_bytes long."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _mx_native as mxn, _native, synthetic
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import elementwise, guard, mx_cases as cases, mx_emul as emul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TM, TN, KS = cases.TM, cases.TN, cases.KS


def _bits(t):
    """the bits of a float tensor as integers, every NaN as one value"""
    t = t.detach().cpu().contiguous()
    b = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).to(torch.int64)
    return torch.where(torch.isnan(t), torch.full_like(b, -1), b)


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    g, w = _bits(got), _bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {got.cpu()[i].item()!r} "
                             f"(bits {int(g[i]):#x}), want {want.cpu()[i].item()!r} (bits {int(w[i]):#x})")


def _round_once(values_f64, dtype):
    """float64 -> dtype; the values this file passes are exact in f32 (or overflow it), so the rounding to 16 bits is the only one"""
    return torch.from_numpy(np.ascontiguousarray(values_f64)).to(torch.float32).to(dtype)


def run_linear(x, w_codes, w_scales, act, bias, out_dtype, fill):
    """mbnb_mx_linear through the C ABI on guard-banded buffers -> (y on the CPU, activation codes, activation scales as the kernel left
    them in the workspace, the last-launch text)"""
    lib = mxn.lib()
    M, K = x.shape
    N = w_codes.shape[0]
    xd, wc, wsc = x.to(DEV).contiguous(), torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)
    b = None if bias is None else bias.to(DEV)
    out = guard._carve("out", (M, N), out_dtype, DEV, fill, 0)
    need = int(lib.mbnb_mx_workspace_bytes(M, K, mxn.ELEM_CODE[act]))
    ws = guard._carve("workspace", (need,), torch.uint8, DEV, fill, 0)
    st = lib.mbnb_mx_linear(ptr(xd), M, K, _native.DTYPE_CODE[xd.dtype], ptr(wc), ptr(wsc), N, mxn.ELEM_CODE[act], ptr(b),
                            0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out.view), _native.DTYPE_CODE[out_dtype], ptr(ws.view), need,
                            stream_ptr(DEV))
    mxn.check(st, "linear")
    torch.cuda.synchronize()
    for g in (out, ws):
        assert g.violation() is None, (g.name, g.violation(), (M, N, K, act, out_dtype, fill))
    cbytes = M * K // 2 if act == "fp4" else M * K
    r256 = (cbytes + 255) // 256 * 256
    a_codes = ws.view[:cbytes].cpu().numpy().reshape(M, -1)
    a_scales = ws.view[r256:r256 + M * K // 32].cpu().numpy().reshape(M, K // 32)
    return out.view.cpu().clone(), a_codes, a_scales, mxn.last_launch()


# ----------------------------------------------------------------------------- 1. the quantiser
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("elem", ("fp4", "fp8"))
def test_quantiser_is_the_emulation_bit_for_bit(elem, dtype):
    for kind in cases.QUANT_KINDS:
        for rows, K in cases.QUANT_SHAPES:
            x = cases.quantiser_input(kind, elem, dtype, rows, K)
            want_codes, want_scales = emul.quantize(cases.as_f32(x), elem)
            codes, scales = bnb.quantize_mx(x.to(DEV), elem)
            assert codes.dtype == torch.uint8 and tuple(codes.shape) == want_codes.shape and tuple(scales.shape) == want_scales.shape
            got_s, got_c = scales.cpu().numpy(), codes.cpu().numpy()
            where = (kind, elem, dtype, rows, K)
            assert (got_s == want_scales).all(), (where, np.argwhere(got_s != want_scales)[:4], got_s[got_s != want_scales][:4], want_scales[got_s != want_scales][:4])
            if not (got_c == want_codes).all():
                r, c = np.argwhere(got_c != want_codes)[0]
                k = c * 2 if elem == "fp4" else c
                raise AssertionError(f"{where}: codes differ at row {r}, byte {c}: got {got_c[r, c]:#x}, want {want_codes[r, c]:#x}; "
                                     f"inputs {x[r, k:k + 2].tolist()}, scale byte {want_scales[r, k // 32]}")
    if elem == "fp4":
        x = cases.quantiser_input("binades", elem, dtype, 17, 160).to(DEV)
        a, b = bnb.quantize_mxfp4(x), bnb.quantize_mx(x, "fp4")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------- 2. the decoder
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("elem", ("fp4", "fp8"))
def test_decoder_is_the_emulation_bit_for_bit(elem, dtype):
    bytes_ = (0, 1, 126, 127, 128, 254, 255)
    if elem == "fp4":
        row = np.array([c | (c << 4) for c in range(16)], dtype=np.uint8)                     # K = 32: every code twice
        codes = np.tile(row, (len(bytes_), 1))
    else:
        codes = np.tile(np.arange(256, dtype=np.uint8), (len(bytes_), 1))                     # K = 256: every code
    K = codes.shape[1] * (2 if elem == "fp4" else 1)
    scales = np.repeat(np.array(bytes_, dtype=np.uint8)[:, None], K // 32, axis=1)
    rng = np.random.default_rng(77)
    rcodes = rng.integers(0, 256, size=(17, 80 if elem == "fp4" else 160), dtype=np.uint8)
    rscales = rng.integers(100, 150, size=(17, 5), dtype=np.uint8)
    for c, s in ((codes, scales), (rcodes, rscales)):
        want = _round_once(emul.decode_f64(c, s, elem), dtype)
        got = bnb.dequantize_mx(torch.from_numpy(c).to(DEV), torch.from_numpy(s).to(DEV), elem, dtype)
        _assert_bits(got.cpu(), want, f"dequantize_mx {elem} -> {dtype}")
    if elem == "fp4":
        got = bnb.dequantize_mxfp4(torch.from_numpy(rcodes).to(DEV), torch.from_numpy(rscales).to(DEV), dtype)
        _assert_bits(got.cpu(), _round_once(emul.decode_f64(rcodes, rscales, "fp4"), dtype), "dequantize_mxfp4")


# ----------------------------------------------------------------------------- 3. the lane map
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_identity_activation_returns_the_decoded_weight(act):
    """X = I (a lone 1 in a block quantises losslessly), W lossless with asymmetric random codes: y = dequantize_mx(W)^T bit for bit
    (a -0 of W comes out as +0: it is summed with the +0 products of its row).  Any other assignment of k to lanes, registers,
    nibbles or scale bytes moves or rescales an element of W."""
    K, N = 256, 48
    w = emul.lossless(N, K, seed=31)
    w_codes, w_scales = emul.quantize(w, "fp4")
    assert (emul.decode_f64(w_codes, w_scales, "fp4") == w).all()
    x = torch.eye(K, dtype=torch.bfloat16)
    want = _round_once(w.T + 0.0, torch.float32)
    for fill in FILLS:
        y, a_codes, a_scales, text = run_linear(x, w_codes, w_scales, act, None, torch.float32, fill)
        assert (emul.decode_f64(a_codes, a_scales, act) == np.eye(K)).all()
        assert text == f"mx_quant {act} + gemm_mx {act} {TM}x{TN}", text
        _assert_bits(y, want, f"identity, activation {act}, fill {fill:#x}")
    deq = bnb.dequantize_mx(torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV), "fp4", torch.float32)
    _assert_bits(y, deq.cpu().t().contiguous() + 0.0, "identity vs dequantize_mx")


# ----------------------------------------------------------------------------- 4. exact GEMM
@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)), ids=lambda i: "-".join(str(v).replace("torch.", "") for v in cases.EXACT_CASES[i]))
def test_exact_gemm_bit_for_bit(index):
    case = cases.EXACT_CASES[index]
    M, N, K, act, out_dtype, _ = case
    x64, w64, bias64 = cases.exact_operands(case, index)
    x_dtype = (torch.bfloat16, torch.float16, torch.float32)[index % 3]
    x = cases.to_dtype(x64, x_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, (torch.float32, torch.bfloat16, torch.float16)[index % 3])
    w_codes, w_scales = emul.quantize(w64, "fp4")
    xa_codes, xa_scales = emul.quantize(x64, act)
    want = _round_once(emul.linear_f64(xa_codes, xa_scales, act, w_codes, w_scales, bias64), out_dtype)
    assert (emul.linear_f64(xa_codes, xa_scales, act, w_codes, w_scales, bias64) == x64 @ w64.T + (0 if bias64 is None else bias64)).all()
    for fill in FILLS:
        y, a_codes, a_scales, _ = run_linear(x, w_codes, w_scales, act, bias, out_dtype, fill)
        assert (a_codes == xa_codes).all() and (a_scales == xa_scales).all()
        _assert_bits(y, want, f"exact GEMM {case}, fill {fill:#x}")
    # the same through the Python surface
    y = bnb.matmul_mxfp4(x.to(DEV), torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV),
                         None if bias is None else bias.to(DEV), act_format=act, dtype=out_dtype)
    _assert_bits(y.cpu(), want, f"matmul_mxfp4 {case}")


def test_one_and_three_dimensional_inputs_and_the_layer():
    K, N = 160, 17
    w64 = emul.lossless(N, K, seed=41)
    w_codes, w_scales = emul.quantize(w64, "fp4")
    wc, wsc = torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)
    x1 = emul.lossless(1, K, seed=42)
    y = bnb.matmul_mxfp4(cases.to_dtype(x1[0], torch.bfloat16).to(DEV), wc, wsc, act_format="fp4")
    assert tuple(y.shape) == (N,) and y.dtype == torch.bfloat16
    _assert_bits(y.cpu(), _round_once((x1 @ w64.T)[0], torch.bfloat16), "1-D input")
    x3 = emul.lossless(6, K, seed=43)
    bias = np.arange(N, dtype=np.float64) - 8
    y = bnb.matmul_mxfp4(cases.to_dtype(x3, torch.float16).reshape(2, 3, K).to(DEV), wc, wsc, cases.to_dtype(bias, torch.float16).to(DEV))
    assert tuple(y.shape) == (2, 3, N) and y.dtype == torch.float16
    _assert_bits(y.cpu(), _round_once(x3 @ w64.T + bias, torch.float16).reshape(2, 3, N), "3-D input")
    # LinearMXFP4: from_linear quantises the lossless weight to exactly its codes; state-dict round trip; both activation formats
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(cases.to_dtype(w64, torch.bfloat16))
        lin.bias.copy_(cases.to_dtype(bias, torch.bfloat16))
    for act in ("fp8", "fp4"):
        layer = bnb.LinearMXFP4.from_linear(lin.to(DEV), act_format=act)
        assert torch.equal(layer.weight.cpu(), torch.from_numpy(w_codes)) and torch.equal(layer.weight_scales.cpu(), torch.from_numpy(w_scales))
        _assert_bits(layer.dequantize().cpu(), cases.to_dtype(w64, torch.bfloat16), "LinearMXFP4.dequantize")
        twin = bnb.LinearMXFP4(K, N, act_format=act, device=DEV)
        twin.load_state_dict(layer.state_dict())
        with torch.no_grad():
            for m in (layer, twin):
                y = m(cases.to_dtype(x3, torch.bfloat16).reshape(3, 2, K).to(DEV))
                _assert_bits(y.cpu(), _round_once(x3 @ w64.T + bias, torch.bfloat16).reshape(3, 2, N), f"LinearMXFP4 {act}")


# ----------------------------------------------------------------------------- 5. random data
@pytest.fixture(scope="module")
def random_case():
    M, N, K = 33, 2 * TN + 5, 1024
    x = synthetic.normal((M, K), torch.bfloat16, seed=51)
    w = synthetic.normal((N, K), torch.bfloat16, seed=52, std=0.02)
    bias = synthetic.normal((N,), torch.bfloat16, seed=53, std=0.1)
    w_codes, w_scales = emul.quantize(cases.as_f32(w), "fp4")
    return x, w, bias, w_codes, w_scales


def _mx_bound(xq, wq, bias, out_dtype):
    """(r, bound): tests/elementwise.py's g*S + u_out*(|r| + g*S) + a with g = (K + 2) * 2^-23: the products of an fp4 / fp8 element
    and an fp4 element are exact in f32, as those of its 16-bit operands"""
    X, W = torch.from_numpy(xq), torch.from_numpy(wq)
    r, S = X @ W.t(), X.abs() @ W.abs().t()
    if bias is not None:
        r, S = r + bias.double(), S + bias.double().abs()
    g = (X.shape[1] + 2) * 2.0 ** -23
    u_out = 0.0 if out_dtype == torch.float32 else elementwise.UNIT[out_dtype]
    a = 2.0 ** -24 if out_dtype == torch.float16 else 0.0
    return r, g * S + u_out * (r.abs() + g * S) + a


@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float32), ids=str)
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_random_data_elementwise_against_f64_over_the_quantised_operands(random_case, act, out_dtype):
    x, w, bias, w_codes, w_scales = random_case
    xa_codes, xa_scales = emul.quantize(cases.as_f32(x), act)
    xq, wq = emul.decode_f64(xa_codes, xa_scales, act), emul.decode_f64(w_codes, w_scales, "fp4")
    r, bound = _mx_bound(xq, wq, bias, out_dtype)
    none = torch.zeros(r.shape, dtype=torch.bool)
    y, a_codes, a_scales, text = run_linear(x, w_codes, w_scales, act, bias, out_dtype, FILLS[0])
    assert (a_codes == xa_codes).all() and (a_scales == xa_scales).all()
    ratio = elementwise._compare(y, r, bound, none, none, none, text, "y = Q(x) . W^T + b")
    print(f"mx random {act} -> {out_dtype}: worst err / bound = {ratio:.4f}")
    # the layer: the same numbers
    layer = bnb.LinearMXFP4(x.shape[1], w.shape[0], act_format=act, device=DEV)
    layer.load_state_dict({"weight": torch.from_numpy(w_codes), "weight_scales": torch.from_numpy(w_scales), "bias": bias})
    with torch.no_grad():
        y2 = layer(x.to(DEV)) if out_dtype == torch.bfloat16 else layer(x.float().to(DEV))
    assert y2.dtype == out_dtype
    _assert_bits(y2.cpu(), y, "LinearMXFP4 vs the C ABI")


# ----------------------------------------------------------------------------- 6. non-finite
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_non_finite_blocks_poison_exactly_their_row_or_column(act):
    M, N, K = 17, 48, 256
    x64, w64 = emul.lossless(M, K, seed=61), emul.lossless(N, K, seed=62)
    w_codes, w_scales = emul.quantize(w64, "fp4")
    x = cases.to_dtype(x64, torch.bfloat16)
    clean, _, _, _ = run_linear(x, w_codes, w_scales, act, None, torch.bfloat16, FILLS[0])
    _assert_bits(clean, _round_once(x64 @ w64.T, torch.bfloat16), "clean run")
    for bad, k in ((float("nan"), 0), (float("inf"), 77), (float("-inf"), K - 1)):
        xb = x.clone()
        xb[3, k] = bad
        y, _, a_scales, _ = run_linear(xb, w_codes, w_scales, act, None, torch.bfloat16, FILLS[1])
        assert a_scales[3, k // 32] == 255 and (a_scales == 255).sum() == 1
        assert bool(torch.isnan(y[3]).all()), (bad, k)
        keep = torch.arange(M) != 3
        _assert_bits(y[keep], clean[keep], f"rows beside the {bad} row")
    ws_bad = w_scales.copy()
    ws_bad[5, 2] = 255
    y, _, _, _ = run_linear(x, w_codes, ws_bad, act, None, torch.bfloat16, FILLS[1])
    assert bool(torch.isnan(y[:, 5]).all())
    keep = torch.arange(N) != 5
    _assert_bits(y[:, keep], clean[:, keep], "columns beside the NaN column")
