"""GPU checks of k_mx_experts_scaled (libmbnb_moemx.so): exact cases through the C ABI on guard-banded output and plan, the
bit rule against matmul_mxfp4, non-finite scale bytes, the Python keyword.  tests/test_moemx_host.py closes the tables' exactness."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moegemm_native as gn, _moemx_native as xn, _native, functional as F, synthetic
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import guard, moemx_cases as cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _mx_bound, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def run_abi(xc, xs, act, per_slot, wc, ws, ids, bias, out_dtype, fill):
    """mbnb_moegemm_plan + mbnb_moemx_experts through the C ABI, the output and the plan in guard bands -> (out on the CPU, launch text)"""
    (T, A), (E, N), K = ids.shape, wc.shape[:2], ws.shape[2] * 32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xc, xs, wc, ws, idt, b = dev(xc), dev(xs), dev(wc), dev(ws), dev(ids), None if bias is None else bias.to(DEV)
    need = gn.plan_bytes(T * A, E)
    out, plan = guard._carve("out", (T, A, N), out_dtype, DEV, fill, 0), guard._carve("plan", (need,), torch.uint8, DEV, fill, 0)
    gn.check(gn.lib().mbnb_moegemm_plan(ptr(idt), T * A, E, ptr(plan.view), need, stream_ptr(DEV)), "plan")
    xn.check(xn.lib().mbnb_moemx_experts(ptr(xc), ptr(xs), xn.FP8 if act == "fp8" else xn.FP4, T, A, int(per_slot), K, ptr(wc), ptr(ws), E, N,
                                         ptr(idt), ptr(b), 0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out.view), _native.DTYPE_CODE[out_dtype], ptr(plan.view), need,
                                         stream_ptr(DEV)), "experts")
    torch.cuda.synchronize()
    assert out.violation() is None and plan.violation() is None, (out.violation(), plan.violation())
    return out.view.cpu(), xn.last_launch()


def want_f64(xc, xs, act, per_slot, wc, ws, ids, bias):
    """float64 over the decoded operands, pair by pair; a pair outside [0, E) a row of +0.0"""
    (T, A), (E, N) = ids.shape, wc.shape[:2]
    want = np.zeros((T * A, N))
    rows = np.arange(T * A) if per_slot else np.arange(T * A) // A
    for e in range(E):
        at = np.nonzero(ids.reshape(-1) == e)[0]
        want[at] = emul.linear_f64(xc[rows[at]], xs[rows[at]], act, wc[e], ws[e], None if bias is None else bias[e].double().numpy())
    return want.reshape(T, A, N)


def lossless_case(act, per_slot, N, K):
    ids = cases.exact_ids()
    xc, xs = emul.quantize(emul.lossless(70 if per_slot else 35, K, 1), act)
    wc, ws = emul.lossless_codes(emul.lossless(3 * N, K, 2))
    bias = torch.from_numpy(np.random.default_rng(3).integers(-8, 9, size=(3, N))).to(torch.bfloat16)
    return xc, xs, wc.reshape(3, N, -1), ws.reshape(3, N, -1), ids, bias


@pytest.mark.parametrize("K", cases.EXACT_K)
@pytest.mark.parametrize("act,per_slot,out_dtype", cases.FORMS, ids=str)
def test_exact(act, per_slot, out_dtype, K):
    for N in cases.EXACT_N:
        xc, xs, wc, ws, ids, bias = lossless_case(act, per_slot, N, K)
        want = _round_once(want_f64(xc, xs, act, per_slot, wc, ws, ids, bias), out_dtype)
        outside = torch.from_numpy((ids < 0) | (ids >= 3))
        assert outside.sum() == 4 and not want[outside].view(torch.uint8).any()     # rows of +0.0, not -0.0
        for fill in (0xFF, 0x00):
            got, text = run_abi(xc, xs, act, per_slot, wc, ws, ids, bias, out_dtype, fill)
            _assert_bits(got, want, f"{act} N{N} K{K} fill {fill:#x}")
            assert text == f"mx_grouped_scaled {act} {'slot' if per_slot else 'shared'} E3 P70 {cases.R}x{cases.CT}"


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_non_finite_and_extreme_scale_bytes(act):
    """planted on an exact case: a 0xFF activation block, a 0xFF weight block, a weight row under byte 0 (f32 subnormal sums) and byte 254
    over an activation block of zeros (0 x 6 * 2^127 is 0: the product is scaled, not the operand)"""
    N, K = 17, 416
    xc, xs, wc, ws, ids, bias = lossless_case(act, False, N, K)
    ids = np.where((ids < 0) | (ids >= 3), 2, ids).astype(np.int32)          # expert 2 has pairs too: the 0xFF of expert 1 must not reach them
    xs[7, 4] = 0xFF
    ws[1, 5, 12], ws[1, 7, :] = 0xFF, 0
    ws[0, 3, 2], ws[1, 3, 2], ws[2, 3, 2] = 254, 254, 254
    xc[:, (64 if act == "fp8" else 32):(96 if act == "fp8" else 48)], xs[:, 2] = 0, 0
    want = want_f64(xc, xs, act, False, wc, ws, ids, None)
    nan = np.isnan(want)
    expect = (np.arange(35) == 7)[:, None, None] | ((ids == 1)[..., None] & (np.arange(N) == 5))
    tiny = want[~nan & (ids == 1)[..., None] & (np.arange(N) == 7)[None, None]]
    assert np.array_equal(nan, expect) and 0 < np.abs(tiny).max() < 2.0 ** -100
    got, _ = run_abi(xc, xs, act, False, wc, ws, ids, None, torch.float32, 0xFF)
    _assert_bits(got, _round_once(want, torch.float32), act)
    x = torch.ones(2, K, device=DEV, dtype=torch.bfloat16)
    x[1, 40] = float("inf")
    one = 127 - emul.EMAX[act]                                               # an Inf makes its block 0xFF by the format's rule
    assert F.quantize_mx(x, act)[1].cpu().tolist() == [[one] * (K // 32), [one, 255] + [one] * (K // 32 - 2)]


@pytest.mark.parametrize("skewed", (False, True))
@pytest.mark.parametrize("N,K", cases.RANDOM_NK)
@pytest.mark.parametrize("act,per_slot,out_dtype", cases.FORMS[:2] + cases.FORMS[3:], ids=str)
def test_a_pair_has_the_bits_of_matmul_mxfp4_on_its_row(act, per_slot, out_dtype, N, K, skewed):
    T, A, E, ids = 75, 4, 9, cases.random_ids(75, 4, 9, skewed, 11)
    x = synthetic.normal((T, A, K) if per_slot else (T, K), torch.bfloat16, seed=12).to(DEV)
    w, s = F.quantize_mx((synthetic.normal((E * N, K), torch.float32, seed=13) * 0.02).to(DEV), "fp4")
    w, s, bias = w.view(E, N, -1), s.view(E, N, -1), synthetic.normal((E, N), torch.bfloat16, seed=14).to(DEV)
    got = F.matmul_mxfp4_experts_scaled(x, w, s, torch.from_numpy(ids).to(DEV), bias, dtype=out_dtype, act_format=act)
    assert xn.last_launch() == f"mx_grouped_scaled {act} {'slot' if per_slot else 'shared'} E{E} P{T * A} {cases.R}x{cases.CT}"
    rows = x.reshape(-1, K)
    pair_row = torch.arange(T * A) if per_slot else torch.arange(T * A) // A
    xq = emul.decode_f64(*emul.quantize(rows.float().cpu().numpy(), act), act)
    for e in range(E):
        at = torch.from_numpy(np.nonzero(ids.reshape(-1) == e)[0])
        alone = F.matmul_mxfp4(rows, w[e], s[e], bias[e], act_format=act, dtype=out_dtype)[pair_row[at].to(DEV)]
        _assert_bits(got.reshape(T * A, N)[at.to(DEV)], alone, f"expert {e}")
        r, bound = _mx_bound(xq[pair_row[at]], emul.decode_f64(w[e].cpu().numpy(), s[e].cpu().numpy(), "fp4"), bias[e].cpu(), out_dtype)
        err = (alone.double().cpu() - r).abs()
        assert bool((err <= bound).all()), (e, float((err / bound).max()))


def _operands(T, A, E, N, K, seed):
    w, s = F.quantize_mx(synthetic.normal((E * N, K), torch.float32, seed=seed + 1).to(DEV), "fp4")
    return (synthetic.normal((T, K), torch.bfloat16, seed=seed).to(DEV), w.view(E, N, -1), s.view(E, N, -1),
            torch.from_numpy(cases.random_ids(T, A, E, False, seed + 2)).to(DEV))


def test_the_keyword_the_module_a_shared_plan_and_the_cut():
    x, w, s, ids = _operands(19, 4, 5, 40, 160, 21)
    y = F.matmul_mxfp4_experts_scaled(x, w, s, ids, act_format="fp8")
    ids32, plans = F.moe_grouped_plan(ids, 5)
    _assert_bits(F.matmul_mxfp4_experts_scaled(x, w, s, ids32, plan=plans, act_format="fp8"), y, "a shared plan")
    layer = bnb.ExpertsMXFP4(5, 160, 40, bias=False, device=DEV)
    layer.weight.copy_(w), layer.weight_scales.copy_(s)
    layer.act_format = "fp8"
    _assert_bits(layer(x, ids), y, "the module")
    assert xn.last_launch() == "mx_grouped_scaled fp8 shared E5 P76 64x256"
    assert not torch.equal(F.matmul_mxfp4_experts_scaled(x, w, s, ids, act_format="none"), y) and gn.last_launch() == "mx_grouped bf16 shared E5 P76 R64"
    # 2 * MOE_GROUPED_MAX_PAIRS + 8 pairs: three calls over the tokens, bit-equal to the calls on its parts
    A, T = 8, (2 * F.MOE_GROUPED_MAX_PAIRS + 8) // 8
    x, w, s, ids = _operands(T, A, 4, 8, 32, 31)
    whole, step = F.matmul_mxfp4_experts_scaled(x, w, s, ids, act_format="fp4"), F.MOE_GROUPED_MAX_PAIRS // A
    assert xn.last_launch() == "mx_grouped_scaled fp4 shared E4 P8 64x256"
    parts = [F.matmul_mxfp4_experts_scaled(x[t:t + step], w, s, ids[t:t + step], act_format="fp4") for t in range(0, T, step)]
    _assert_bits(whole, torch.cat(parts), "the cut")


def test_a_captured_graph_serves_new_rows_and_a_new_routing():
    x, w, s, ids = _operands(33, 4, 6, 48, 224, 41)
    call = lambda: F.matmul_mxfp4_experts_scaled(x, w, s, ids, act_format="fp8")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # the quantiser, the plan and the launch
        y = call()
    for seed in (51, 61, 71):
        x2, _, _, ids2 = _operands(33, 4, 6, 48, 224, seed)
        x.copy_(x2), ids.copy_(ids2)
        graph.replay()
        _assert_bits(y, call(), f"replay {seed}")
