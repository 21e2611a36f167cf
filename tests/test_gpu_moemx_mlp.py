"""GPU checks of the expert MLP on k_mx_experts_scaled: GluQ bit for bit at alpha = 0 and inside the chain's bound at
1.702, down + sum bit for bit, the whole MLP against its parts, across the cut, in a graph and against float64."""
import numpy as np
import pytest
import torch

from mps_bitsandbytes_amd import _moegemm_native as gn, _moemx_native as xn, _native, functional as F, synthetic
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import guard, moemlp_cases as mlp, mx_emul as emul
from tests.test_gpu_moemx import _operands, lossless_case, want_f64
from tests.test_gpu_mx import _assert_bits, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ACT = {"fp8": xn.FP8, "fp4": xn.FP4}
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def planned(ids, E, fill):   # -> (ids on the device, the guard-banded plan of mbnb_moegemm_plan, its bytes)
    idt, need = dev(ids), gn.plan_bytes(ids.size, E)
    plan = guard._carve("plan", (need,), torch.uint8, DEV, fill, 0)
    gn.check(gn.lib().mbnb_moegemm_plan(ptr(idt), ids.size, E, ptr(plan.view), need, stream_ptr(DEV)), "plan")
    return idt, plan, need


@pytest.mark.parametrize("limit", (mlp.INF, 7.0))
@pytest.mark.parametrize("K", (32, 96, 128, 416))
@pytest.mark.parametrize("I", (32, 160))
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_gluq_is_the_quantiser_over_the_f32_chain_bit_for_bit(act, I, K, limit):
    """alpha = 0: the activation is exact f32 arithmetic, so the bytes are the quantiser's over glu_f32(pre); skipped pairs read 0"""
    xc, xs, wc, ws, ids, bias = lossless_case(act, False, 2 * I, K)
    pre = want_f64(xc, xs, act, False, wc, ws, ids, bias).reshape(70, 2 * I).astype(np.float32)
    h = mlp.glu_f32(*mlp.split(pre), 0.0, limit)
    h[((ids < 0) | (ids >= 3)).reshape(-1)] = 0.0
    want_c, want_s = emul.quantize(h, act)
    for fill in (0xFF, 0x00):
        idt, plan, need = planned(ids, 3, fill)
        hc, hs = (guard._carve(n, (70, w), torch.uint8, DEV, fill, 0) for n, w in (("h_codes", want_c.shape[1]), ("h_scales", I // 32)))
        args = [dev(xc), dev(xs), dev(wc), dev(ws), bias.to(DEV)]
        xn.check(xn.lib().mbnb_moemx_gate_up_glu(ptr(args[0]), ptr(args[1]), ACT[act], 35, 2, K, ptr(args[2]), ptr(args[3]), 3, I, ptr(idt), ptr(args[4]), _native.BF16,
                                                 0.0, limit, ptr(hc.view), ptr(hs.view), ACT[act], ptr(plan.view), need, stream_ptr(DEV)), "glu")
        torch.cuda.synchronize()
        assert [b.violation() for b in (hc, hs, plan)] == [None] * 3
        assert xn.last_launch() == f"mx_grouped_scaled_glu {act}>{act} E3 P70 64x256"
        for name, got, want in (("scales", hs, want_s), ("codes", hc, want_c)):
            diff = np.argwhere(got.view.cpu().numpy() != want)
            assert not len(diff), f"{name}, fill {fill:#x}: {len(diff)} of {want.size} bytes differ, first at {tuple(diff[0])}"


# the quantiser's scale byte for a finite block amax, max(E - emax, 0) with E the f32 exponent field; and the signed grid value nearest
# to v (ties to the even code, saturating), monotone in v
_byte_of = lambda amax, act: np.maximum(np.where(amax >= 2.0 ** -126, np.floor(np.log2(np.maximum(amax, 2.0 ** -126))) + 127, 0) - emul.EMAX[act], 0)
_grid = lambda v, act: np.sign(v) * emul.GRID[act][emul._nearest_even_code(np.abs(v), emul.GRID[act])]


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_gluq_at_the_model_alpha_stays_inside_the_chain_bound_and_marks_non_finite_blocks(act):
    """h = glu_f64(the Plain launch's f32 pre), d = glu_tol |h|: every scale byte is the quantiser's for some amax in [a - d, a + d] and
    under it every element lies between the grid values of h -+ d; exactly the blocks with a non-finite h read byte 0xFF, codes 0"""
    T, A, E, I, K = 24, 4, 5, 160, 224
    x, w, s, ids = _operands(T, A, E, 2 * I, K, 81)
    bias = synthetic.normal((E, 2 * I), torch.bfloat16, seed=85).to(DEV)
    x[7, 40], s[1, 5, 3] = float("inf"), 0xFF
    pre = F.matmul_mxfp4_experts_scaled(x, w, s, ids, bias, dtype=torch.float32, act_format=act).reshape(T * A, 2 * I).cpu().numpy()
    codes, scales = F.matmul_mxfp4_experts_scaled_glu(x, w, s, ids, bias, act_format=act)
    assert xn.last_launch() == f"mx_grouped_scaled_glu {act}>{act} E{E} P{T * A} 64x256"
    with np.errstate(invalid="ignore"):
        h = mlp.glu_f64(*mlp.split(pre), mlp.ALPHA, mlp.LIMIT).reshape(T * A, I // 32, 32)
    bad = ~np.isfinite(h).all(axis=2)
    assert bad[7 * A:8 * A].all() and bad.sum() > A and not bad.all()              # the token's pairs whole, expert 1's pairs at block 0
    got_s = scales.reshape(T * A, I // 32).cpu().numpy().astype(np.int64)
    got = emul.decode_f64(codes.reshape(T * A, -1).cpu().numpy(), np.where(bad, 127, got_s), act).reshape(h.shape)
    assert np.array_equal(got_s == 255, bad) and not emul.unpack(codes.reshape(T * A, -1).cpu().numpy(), act).reshape(h.shape)[bad].any()
    h, got, got_s = h[~bad], got[~bad], got_s[~bad]
    d = mlp.glu_tol(h)
    lo, hi = _byte_of(np.maximum(np.abs(h) - d, 0).max(axis=1), act), _byte_of((np.abs(h) + d).max(axis=1), act)
    assert ((lo <= got_s) & (got_s <= hi)).all(), "a scale byte outside the bytes of [amax - d, amax + d]"
    unit = np.ldexp(1.0, got_s - 127)[:, None]
    ok = (_grid((h - d) / unit, act) <= got / unit) & (got / unit <= _grid((h + d) / unit, act))
    assert ok.all(), f"{(~ok).sum()} of {ok.size} elements outside the grid values of h -+ d"


@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float16, torch.float32), ids=str)
@pytest.mark.parametrize("N,K", ((17, 32), (257, 416), (17, 416), (257, 32)))
@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_down_sum_is_the_float64_chain_rounded_once(act, N, K, out_dtype):
    """lossless codes, power-of-two routing weights: every fmaf is exact; a skipped slot's routing weight is NaN and must not appear"""
    hc, hsc, wc, ws, ids, bias = lossless_case(act, True, N, K)
    live = (ids >= 0) & (ids < 3)
    rw = np.ldexp(1.0, np.random.default_rng(7).integers(-3, 2, size=ids.shape)).astype(np.float32)
    y = want_f64(hc, hsc, act, True, wc, ws, ids, bias)
    total = np.where(live[..., None], rw[..., None] * y, 0.0).sum(axis=1)
    assert np.array_equal(total.astype(np.float32).astype(np.float64), total)      # exact in f32: one rounding, the output's
    want = _round_once(total, out_dtype)
    rw[~live] = np.nan
    for fill in (0xFF, 0x00):
        idt, plan, need = planned(ids, 3, fill)
        wsb = xn.workspace_bytes(70, N)
        out, wsp = guard._carve("out", (35, N), out_dtype, DEV, fill, 0), guard._carve("workspace", (wsb,), torch.uint8, DEV, fill, 0)
        args = [dev(hc), dev(hsc), dev(wc), dev(ws), bias.to(DEV), dev(rw)]
        xn.check(xn.lib().mbnb_moemx_down_sum(ptr(args[0]), ptr(args[1]), ACT[act], 35, 2, K, ptr(args[2]), ptr(args[3]), 3, N, ptr(idt), ptr(args[4]), _native.BF16,
                                              ptr(args[5]), _native.F32, ptr(out.view), _native.DTYPE_CODE[out_dtype], ptr(wsp.view), wsb, ptr(plan.view), need, stream_ptr(DEV)), "down_sum")
        torch.cuda.synchronize()
        assert [b.violation() for b in (out, wsp, plan)] == [None] * 3
        assert xn.last_launch() == f"mx_grouped_scaled_down_sum {act} E3 P70 64x256 A2"
        _assert_bits(out.view.cpu(), want, f"fill {fill:#x}")


def _mlp_operands(T, A, E, H, I, seed):
    x, gw, gs, ids = _operands(T, A, E, 2 * I, H, seed)
    dw, ds = F.quantize_mx((synthetic.normal((E * H, I), torch.float32, seed=seed + 3) * 0.1).to(DEV), "fp4")
    rw = torch.softmax(synthetic.normal((T, A), torch.float32, seed=seed + 4).to(DEV), dim=1)
    gb, db = (synthetic.normal((E, n), torch.bfloat16, seed=seed + 5 + i).to(DEV) for i, n in enumerate((2 * I, H)))
    return x, gw, gs, gb, dw.view(E, H, -1), ds.view(E, H, -1), db, ids, rw


# |dh| of an element under its block's scale <= c1 |h| + c2 amax(block).  fp8 (scale 2^(E(amax) - 8)): half a spacing 2^-4 |h|, 448 for
# up to 512 loses 2^-3 |h|, the subnormal half-spacing 2^-10 of the scale is 2^-18 amax.  fp4 (scale 2^(E(amax) - 2)): half a spacing
# and 6 for up to 8 lose |h| / 4 from 1 up; below 1 a quarter of the scale, amax / 16.
QUANT = {"fp8": (2.0 ** -3, 2.0 ** -18), "fp4": (2.0 ** -2, 2.0 ** -4)}


@pytest.mark.parametrize("act", ("fp8", "fp4"))
def test_the_whole_mlp_is_its_parts_and_stays_inside_the_format_bound(act):
    T, A, E, H, I = 37, 4, 5, 96, 64
    ops = _mlp_operands(T, A, E, H, I, 91)
    x, gw, gs, gb, dw, ds, db, ids, rw = ops
    y = F.moe_mlp_mxfp4_scaled(*ops, act_format=act)
    assert xn.last_launch() == f"mx_grouped_scaled_down_sum {act} E{E} P{T * A} 64x256 A{A}" and y.dtype == x.dtype
    h = F.matmul_mxfp4_experts_scaled_glu(x, gw, gs, ids, gb, act_format=act)
    _assert_bits(y, F.matmul_mxfp4_experts_scaled_sum(h, dw, ds, ids, rw, db, dtype=x.dtype, act_format=act), "the three calls composed")
    # float64 over the same quantised operands.  The bound: both accumulations' f32 roundings ((K + 2) 2^-23 of the sums of magnitudes),
    # the first through the activation (|d/du| <= limit, |d/dg| <= 1.1 (limit + 1)), glu_tol, the quantiser of h, the bf16 rounding
    xq = emul.decode_f64(*(t.cpu().numpy() for t in F.quantize_mx(x, act)), act)
    dec = lambda w, s: emul.decode_f64(w.reshape(-1, w.shape[-1]).cpu().numpy(), s.reshape(-1, s.shape[-1]).cpu().numpy(), "fp4").reshape(E, w.shape[1], -1)
    gwd, dwd, idn, rwn, c1, c2 = dec(gw, gs), dec(dw, ds), ids.cpu().numpy(), rw.double().cpu().numpy(), *QUANT[act]
    want, bound = np.zeros((T, H)), np.zeros((T, H))
    for t in range(T):
        for a in range(A):
            e, r = idn[t, a], rwn[t, a]
            pre, S = xq[t] @ gwd[e].T + gb[e].double().cpu().numpy(), np.abs(xq[t]) @ np.abs(gwd[e]).T + gb[e].double().abs().cpu().numpy()
            h64 = mlp.glu_f64(pre[0::2], pre[1::2], mlp.ALPHA, mlp.LIMIT)
            dh = 1.1 * (mlp.LIMIT + 1) * (H + 2) * 2.0 ** -23 * (S[0::2] + S[1::2]) + mlp.glu_tol(h64)
            amax = np.repeat((np.abs(h64) + dh).reshape(-1, 32).max(axis=1), 32)
            dh = dh + c1 * (np.abs(h64) + dh) + c2 * amax
            S2 = (np.abs(h64) + dh) @ np.abs(dwd[e]).T + db[e].double().abs().cpu().numpy()
            want[t] += r * (h64 @ dwd[e].T + db[e].double().cpu().numpy())
            bound[t] += r * (dh @ np.abs(dwd[e]).T + (I + 2 + A) * 2.0 ** -23 * S2)
    bound += 2.0 ** -8 * (np.abs(want) + bound)
    err = np.abs(y.double().cpu().numpy() - want)
    print(f"{act}: max err / bound {float((err / bound).max()):.3f}, relative Frobenius error {np.linalg.norm(err) / np.linalg.norm(want):.4f}")
    assert (err <= bound).all(), float((err / bound).max())


def test_the_whole_mlp_across_the_cut_and_in_a_captured_graph():
    A, T = 8, (F.MOE_GROUPED_MAX_PAIRS + 8) // 8
    ops = _mlp_operands(T, A, 4, 32, 32, 101)
    whole, step = F.moe_mlp_mxfp4_scaled(*ops, act_format="fp4"), F.MOE_GROUPED_MAX_PAIRS // A
    assert xn.last_launch() == "mx_grouped_scaled_down_sum fp4 E4 P8 64x256 A8"
    part = lambda a, b: F.moe_mlp_mxfp4_scaled(ops[0][a:b], *ops[1:7], ops[7][a:b], ops[8][a:b], act_format="fp4")
    _assert_bits(whole, torch.cat((part(0, step), part(step, T))), "the cut")
    ops = _mlp_operands(33, 4, 6, 224, 96, 111)
    call = lambda: F.moe_mlp_mxfp4_scaled(*ops, act_format="fp8")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # the plan, the quantiser, GluQ, down and the sum
        y = call()
    for seed in (121, 131, 141):
        for mine, new in zip(ops, _mlp_operands(33, 4, 6, 224, 96, seed)):
            mine.copy_(new)                                  # ids, weights, biases, routing weights and input, all in place
        graph.replay()
        _assert_bits(y, call(), f"replay {seed}")
