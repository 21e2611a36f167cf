"""The MXFP4 mixture-of-experts MLP (k_mx_experts_rt, k_routed_sum) through the C ABI on guard-banded, offset operands,
outputs and workspace under the fills 0xFF and 0x00, and through the Python surface.  The tables and the numpy chains are
tests/moemlp_cases.py (closed on the CPU by tests/test_moemlp_host.py).  The yardstick is the f32 output of mbnb_moe_mxfp4_experts,
a kernel older than these, for the same rows, experts and bias: the gated activation and the routed sum are restated over it.

  1  gate / up + GLU, alpha = 0: bit for bit        2  alpha = 1.702 inside the derived bound of the float64 chain
  3  every pair alone and inside another batch      4  ids outside [0, E), 0xFF scale bytes, Inf / NaN rows
  5  down + sum: bit for bit                        6  skipped pairs, 0xFF scale bytes, the workspace
  7  the Python surface: the composition, the whole block against float64, views, streams, cuts, a captured graph, the module"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _moemlp_native as mlpn, _native
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import guard, moe_cases, moemlp_cases as cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)
F32 = np.float32
CODE = _native.DTYPE_CODE


def _name(v):
    return str(v).replace("torch.", "").replace(" ", "")[:40]


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _placed(name, t, fill, offset_bytes):
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def _canon(t):
    """every NaN on one bit pattern: which NaN an Inf * 0 gives is the only thing numpy and the device may differ in"""
    t = t.clone()
    t[torch.isnan(t)] = float("nan")
    return t


def _assert_bits_nan(got, want, what):
    _assert_bits(_canon(got), _canon(want), what)


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16) == 0).all())


def run_parent(x, w_codes, w_scales, ids, bias):
    """The yardstick: mbnb_moe_mxfp4_experts into f32 -> numpy f32 [T * A, N].  x [T, K] (shared) or [T, A, K] (a row per slot)."""
    T, A = ids.shape
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xd, wc, wsc = x.to(DEV).contiguous(), torch.as_tensor(w_codes).to(DEV), torch.as_tensor(w_scales).to(DEV)
    ig = torch.as_tensor(ids).to(DEV)
    b = None if bias is None else bias.to(DEV)
    out = torch.empty(T * A, N, dtype=torch.float32, device=DEV)
    st = moen.lib().mbnb_moe_mxfp4_experts(ptr(xd), T, A, int(x.dim() == 3), K, CODE[x.dtype], ptr(wc), ptr(wsc), E, N, ptr(ig),
                                           None if b is None else ptr(b), 0 if b is None else CODE[b.dtype], ptr(out), CODE[torch.float32],
                                           stream_ptr(DEV))
    moen.check(st, "mxfp4_experts")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_guards(guards, what):
    for g in guards:
        assert g.violation() is None, (g.name, g.violation(), what)


def run_glu(x, w_codes, w_scales, ids, bias, alpha, limit, out_dtype, fill, offsets=None):
    """mbnb_moemlp_gate_up_glu through the C ABI, every operand carved inside guard bands at its offset -> h [T * A, I] on the CPU"""
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    T, A = ids.shape
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xg = _placed("x", x.contiguous(), fill, off["x"])
    wc = _placed("w_codes", torch.as_tensor(w_codes), fill, off["w_codes"])
    wsc = _placed("w_scales", torch.as_tensor(w_scales), fill, off["w_scales"])
    ig = _placed("ids", torch.as_tensor(ids), fill, 4 * off["ids"])
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    out = guard._carve("out", (T * A, N // 2), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
    st = mlpn.lib().mbnb_moemlp_gate_up_glu(ptr(xg.view), T, A, K, CODE[x.dtype], ptr(wc.view), ptr(wsc.view), E, N // 2, ptr(ig.view),
                                            None if b is None else ptr(b.view), 0 if b is None else CODE[bias.dtype], alpha, limit,
                                            ptr(out.view), CODE[out_dtype], stream_ptr(DEV))
    mlpn.check(st, "gate_up_glu")
    torch.cuda.synchronize()
    _check_guards((out, xg, wc, wsc, ig) + (() if b is None else (b,)), (E, N, K, T, A, x.dtype, out_dtype, fill, off))
    assert mlpn.last_launch() == cases.glu_text(x.dtype, E, T * A), mlpn.last_launch()
    return out.view.cpu().clone()


def run_down(h, w_codes, w_scales, ids, bias, rw, out_dtype, fill, offsets=None, ws_fill=None):
    """mbnb_moemlp_down_sum through the C ABI; the workspace is carved too, exactly workspace_bytes long -> out [T, N] on the CPU"""
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    T, A = ids.shape
    K, (E, N) = h.shape[-1], w_codes.shape[:2]
    lib = mlpn.lib()
    hg = _placed("h", h.contiguous(), fill, off["x"])
    wc = _placed("w_codes", torch.as_tensor(w_codes), fill, off["w_codes"])
    wsc = _placed("w_scales", torch.as_tensor(w_scales), fill, off["w_scales"])
    ig = _placed("ids", torch.as_tensor(ids), fill, 4 * off["ids"])
    rg = _placed("rw", rw, fill, off["rw"] * _esize(rw.dtype))
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    need = int(lib.mbnb_moemlp_workspace_bytes(T, A, N))
    assert need == -(-T * A * N * 4 // 256) * 256
    ws = guard._carve("workspace", (need,), torch.uint8, DEV, fill if ws_fill is None else ws_fill, off["ws"])
    out = guard._carve("out", (T, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
    st = lib.mbnb_moemlp_down_sum(ptr(hg.view), T, A, K, CODE[h.dtype], ptr(wc.view), ptr(wsc.view), E, N, ptr(ig.view),
                                  None if b is None else ptr(b.view), 0 if b is None else CODE[bias.dtype], ptr(rg.view), CODE[rw.dtype],
                                  ptr(out.view), CODE[out_dtype], ptr(ws.view), need, stream_ptr(DEV))
    mlpn.check(st, "down_sum")
    torch.cuda.synchronize()
    _check_guards((out, ws, hg, wc, wsc, ig, rg) + (() if b is None else (b,)), (E, N, K, T, A, h.dtype, out_dtype, fill, off))
    assert mlpn.last_launch() == cases.down_text(h.dtype, E, T * A, A), mlpn.last_launch()
    return out.view.cpu().clone()


def _glu_want(pre, alpha, limit, out_dtype):
    g, u = cases.split(pre)
    return _round_once(cases.glu_f32(g, u, alpha, limit).astype(np.float64), out_dtype)


def _sum_want(y, rw, ids, E, out_dtype):
    return _round_once(cases.routed_sum_f32(y, rw.float().numpy(), ids, E).astype(np.float64), out_dtype)


# ----------------------------------------------------------------------------- 1. the exact chain, alpha = 0
@pytest.mark.parametrize("index", range(len(cases.GLU_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.GLU_CASES[i]))
def test_glu_with_alpha_zero_bit_for_bit(index):
    case = cases.GLU_CASES[index]
    E, I, K, T, A, _, x_dtype, out_dtype, _, limit = case
    x64, w64, bias64, ids = cases.glu_operands(case, index)
    w_codes, w_scales = cases.quantize_experts(w64)
    x = cases.to_dtype(x64, x_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[index % 3])
    pre = run_parent(x, w_codes, w_scales, ids, bias)
    assert np.isfinite(pre).all()
    want = _glu_want(pre, 0.0, limit, out_dtype)
    for fill in FILLS:                                       # an element the launch never wrote holds the fill: it cannot match under both
        h = run_glu(x, w_codes, w_scales, ids, bias, 0.0, limit, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits(h, want, f"glu alpha 0 {case[:5]}, fill {fill:#x}")


def _pre_is_float64(pre, x64, w_codes, w_scales, bias64, ids):
    """the yardstick's f32 pre-activations are the float64 result over the decoded weights, rounded once"""
    want = _round_once(moe_cases.reference_f64(x64, moe_cases.decode_experts(w_codes, w_scales), bias64, ids), torch.float32)
    _assert_bits_nan(torch.from_numpy(pre), want, "the f32 pre-activations against float64")


@pytest.mark.parametrize("index", range(len(cases.WALK_GLU_CASES)), ids=lambda i: f"K{cases.WALK_KS[i]}")
def test_glu_with_alpha_zero_at_every_k_of_the_walk_bit_for_bit(index):
    """tests/moe_cases.py WALK_KS through k_mx_experts_rt's GLU epilogue, under the rule of test_glu_with_alpha_zero_bit_for_bit"""
    case = cases.WALK_GLU_CASES[index]
    E, I, K, T, A, _, x_dtype, out_dtype, _, limit = case
    x64, w64, bias64, ids = cases.glu_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    x = cases.to_dtype(x64, x_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[(index + 1) % 3])
    pre = run_parent(x, w_codes, w_scales, ids, bias)
    assert np.isfinite(pre).all()
    _pre_is_float64(pre, x64, w_codes, w_scales, bias64, ids)
    want = _glu_want(pre, 0.0, limit, out_dtype)
    for fill in FILLS:
        h = run_glu(x, w_codes, w_scales, ids, bias, 0.0, limit, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits(h, want, f"glu alpha 0 at K = {K} {case[:5]}, fill {fill:#x}")


# ----------------------------------------------------------------------------- 2. alpha = 1.702 against float64
def _assert_glu_bound(h, pre, out_dtype, what):
    g, u = cases.split(pre)
    r = cases.glu_f64(g, u, cases.ALPHA, cases.LIMIT)
    y = h.double().numpy()
    ok, lo, hi = cases.within_glu_bound(y, r, out_dtype)
    worst = float((np.abs(y - r) / cases.glu_tol(r)).max())
    print(f"{what} -> {_name(out_dtype)}: worst |gpu - f64| / tol = {worst:.4f}" + (" (the output's own rounding included)" if out_dtype != torch.float32 else ""))
    assert np.isfinite(y).all() and ok.all(), (what, out_dtype, int((~ok).sum()), y[~ok][:4], lo[~ok][:4], hi[~ok][:4], g[~ok][:4], u[~ok][:4])
    return worst


@pytest.mark.parametrize("out_dtype", cases.DTYPES, ids=_name)
def test_glu_on_planted_pre_activations_inside_the_bound_of_float64(out_dtype):
    E, I, K, T, A = cases.PLANT_SHAPE
    bias, ids = torch.from_numpy(cases.planted_bias()), cases.planted_ids()
    x = cases.to_dtype(emul.lossless(T, K, seed=39200), torch.bfloat16)
    w_codes, w_scales = np.zeros((E, 2 * I, K // 2), dtype=np.uint8), np.full((E, 2 * I, K // 32), 127, dtype=np.uint8)
    pre = run_parent(x, w_codes, w_scales, ids, bias)
    assert (pre.view(np.uint32) == bias.numpy()[ids.reshape(-1)].view(np.uint32)).all()      # zero codes: pre is the planted bias
    h = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, out_dtype, FILLS[0])
    _assert_glu_bound(h, pre, out_dtype, "planted (g, u)")
    h0 = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, out_dtype, FILLS[1])
    _assert_bits(h0, h, "the same bits under the other fill")


_RANDOM = {}


def _random_glu(shape, x_dtype):
    """(x, codes, scales, bias, ids) of a random gate / up case, the weights quantised once per shape"""
    x, w, bias, ids = cases.random_operands(shape, x_dtype)
    if shape not in _RANDOM:
        T, A, E, N, K = shape
        codes, scales = emul.quantize(w.reshape(E * N, K).numpy(), "fp4")
        _RANDOM[shape] = (codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32))
    return (x,) + _RANDOM[shape] + (bias, ids)


@pytest.mark.parametrize("x_dtype", cases.X16, ids=_name)
@pytest.mark.parametrize("shape", cases.RANDOM_GLU_SHAPES, ids=_name)
def test_glu_on_random_data_inside_the_bound_and_every_pair_alone_and_in_another_batch(shape, x_dtype):
    T, A, E, N, K = shape
    x, w_codes, w_scales, bias, ids = _random_glu(shape, x_dtype)
    bias = bias * 4.0                                        # pre-activations on both sides of the limit
    pre = run_parent(x, w_codes, w_scales, ids, bias)
    assert (np.abs(pre) > cases.LIMIT).any() and (np.abs(pre) < cases.LIMIT).any()
    h32 = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, torch.float32, FILLS[0], cases.OFFSETS[1])
    _assert_glu_bound(h32, pre, torch.float32, f"random {shape} {_name(x_dtype)}")
    h = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, x_dtype, FILLS[1], cases.OFFSETS[2])
    _assert_bits(h, h32.to(x_dtype), "one rounding of the f32 value")
    _assert_glu_bound(h, pre, x_dtype, f"random {shape} {_name(x_dtype)}")
    # 3. every pair alone: T = 1, A = 1
    h = h.reshape(T, A, N // 2)
    for t in range(T):
        for a in range(A):
            one = run_glu(x[t:t + 1], w_codes, w_scales, ids[t:t + 1, a:a + 1], bias, cases.ALPHA, cases.LIMIT, x_dtype, FILLS[(t + a) % 2])
            _assert_bits(one, h[t, a:a + 1], f"pair ({t}, {a}) alone")
    # and inside another batch: the first two tokens kept (moved to the end), every other token and routing redrawn
    g = torch.Generator().manual_seed(39300 + N)
    x2 = torch.randn(x.shape, generator=g).to(x_dtype)
    ids2 = np.random.default_rng(39400 + N).integers(-1, E, size=(T, A)).astype(np.int32)
    x2[T - 2:], ids2[T - 2:] = x[:2], ids[:2]
    h2 = run_glu(x2, w_codes, w_scales, ids2, bias, cases.ALPHA, cases.LIMIT, x_dtype, FILLS[0]).reshape(T, A, N // 2)
    _assert_bits(h2[T - 2:], h[:2], "the kept tokens inside another batch")


# ----------------------------------------------------------------------------- 4. the edges of the semantics
def _edge_glu_operands(K=cases.EDGE_SHAPE[2]):
    E, I, _, T, A = cases.EDGE_SHAPE
    x64 = emul.lossless(T, K, seed=39501) * 0.125
    w64 = emul.lossless(E * 2 * I, K, seed=39502).reshape(E, 2 * I, K)
    bias = torch.from_numpy(np.random.default_rng(39503).integers(1, 9, size=(E, 2 * I)).astype(F32))      # never zero: a bias that leaked shows
    return x64, cases.quantize_experts(w64), bias, cases.EDGE_IDS.copy()


def test_glu_ids_outside_the_experts_give_rows_of_plus_zero_and_leave_every_other_pair_alone():
    E, I, K, T, A = cases.EDGE_SHAPE
    x64, (w_codes, w_scales), bias, ids = _edge_glu_operands()
    x = cases.to_dtype(x64, torch.bfloat16)
    for od in cases.DTYPES:
        base = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, od, FILLS[0])
        assert not _is_plus_zero(base)
        planted = ids.copy()
        for (t, a), v in zip(cases.OUT_OF_RANGE_PLACES, cases.OUT_OF_RANGE):
            planted[t, a] = np.int64(E if v is None else v).astype(np.int32)
        gone = torch.from_numpy(((planted < 0) | (planted >= E)).reshape(-1))
        assert int(gone.sum()) == 4
        for fill in FILLS:
            h = run_glu(x, w_codes, w_scales, planted, bias, cases.ALPHA, cases.LIMIT, od, fill, cases.OFFSETS[3])
            assert _is_plus_zero(h[gone]), (od, fill)
            _assert_bits(h[~gone], base[~gone], "the pairs whose id stayed")
        for v in cases.OUT_OF_RANGE:
            every = np.full((T, A), np.int64(E if v is None else v).astype(np.int32), dtype=np.int32)
            for fill in FILLS:
                assert _is_plus_zero(run_glu(x, w_codes, w_scales, every, bias, cases.ALPHA, cases.LIMIT, od, fill)), (v, od, fill)


def _glu_nan_bytes(row, K, blocks):
    E, I, _, T, A = cases.EDGE_SHAPE
    x64, (w_codes, w_scales), bias, ids = _edge_glu_operands(K)
    clean = None
    hit = torch.zeros(T * A, I, dtype=torch.bool)
    hit[torch.from_numpy(ids.reshape(-1) == cases.NAN_EXPERT), cases.NAN_OUTPUT] = True
    assert 0 < int(hit.sum()) < T * A
    for i, b in enumerate(blocks):
        x = cases.to_dtype(x64, cases.X16[i % 2])
        clean = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, torch.float32, FILLS[0])
        assert bool(torch.isfinite(clean).all())
        planted = w_scales.copy()
        planted[cases.NAN_EXPERT, 2 * cases.NAN_OUTPUT + row, b] = 255
        for fill in FILLS:
            h = run_glu(x, w_codes, planted, ids, bias, cases.ALPHA, cases.LIMIT, torch.float32, fill)
            assert bool(torch.isnan(h[hit]).all()), (row, b, fill)
            _assert_bits(h[~hit], clean[~hit], f"0xFF in block {b} of the {('gate', 'up')[row]} row: every other element")


@pytest.mark.parametrize("row", (0, 1), ids=("gate-row", "up-row"))
def test_glu_a_nan_scale_byte_makes_its_output_nan_for_the_pairs_of_its_expert_only(row):
    _glu_nan_bytes(row, cases.EDGE_SHAPE[2], cases.NAN_BLOCKS)


def _glu_bad_activations(x_dtype, K, ks):
    E, I, _, T, A = cases.EDGE_SHAPE
    x64, (w_codes, w_scales), bias, ids = _edge_glu_operands(K)
    clean = run_glu(cases.to_dtype(x64, x_dtype), w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, torch.float32, FILLS[0]).reshape(T, A, I)
    other = torch.tensor([t != cases.X_BAD_TOKEN for t in range(T)])
    seen_nan = 0
    for ki, k in enumerate(ks):
        for vi, v in enumerate(cases.X_BAD_VALUES):
            xb = x64.copy()
            xb[cases.X_BAD_TOKEN, k] = v
            x = cases.to_dtype(xb, x_dtype)
            pre = run_parent(x, w_codes, w_scales, ids, bias)
            want = torch.from_numpy(cases.glu_f32(*cases.split(pre), 0.0, cases.LIMIT)).reshape(T, A, I)       # IEEE propagation, exactly
            h = run_glu(x, w_codes, w_scales, ids, bias, 0.0, cases.LIMIT, torch.float32, FILLS[(ki + vi) % 2]).reshape(T, A, I)
            _assert_bits_nan(h, want, f"{v} at k = {k}, alpha 0")
            h = run_glu(x, w_codes, w_scales, ids, bias, cases.ALPHA, cases.LIMIT, torch.float32, FILLS[(ki + vi + 1) % 2]).reshape(T, A, I)
            _assert_bits(h[other], clean[other], f"{v} at k = {k}: the other tokens")
            seen_nan += int(torch.isnan(h[cases.X_BAD_TOKEN]).sum())
    assert seen_nan > 0


@pytest.mark.parametrize("x_dtype", cases.X16, ids=_name)
def test_glu_inf_and_nan_in_a_token_row_touch_that_tokens_pairs_only(x_dtype):
    K = cases.EDGE_SHAPE[2]
    _glu_bad_activations(x_dtype, K, (0, 31, 32, K - 1))


@pytest.mark.parametrize("K", cases.WALK_NONFINITE_KS)
def test_glu_nan_bytes_inf_and_nan_on_a_ragged_last_step_off_wave_0(K):
    """The 0xFF byte on the first block of the last step and on block KB - 1 (of a gate row at one K, of an up row at the other), the
    Inf and the NaN at the first k of that step and at k = K - 1: the step runs on wave 7 (K = 992), on wave 6 in its third pass (2880)"""
    i = cases.WALK_NONFINITE_KS.index(K)
    _glu_nan_bytes(i % 2, K, moe_cases.walk_nan_blocks(K))
    _glu_bad_activations(cases.X16[i % 2], K, moe_cases.walk_bad_ks(K))


# ----------------------------------------------------------------------------- 5. down + sum, bit for bit
@pytest.mark.parametrize("index", range(len(cases.SUM_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.SUM_CASES[i]))
def test_down_and_routed_sum_bit_for_bit(index):
    case = cases.SUM_CASES[index]
    E, N, K, T, A, _, h_dtype, out_dtype, _, rw_dtype = case
    h64, w64, bias64, ids, rw64 = cases.sum_operands(case, index)
    w_codes, w_scales = cases.quantize_experts(w64)
    h = cases.to_dtype(h64, h_dtype)
    rw = cases.to_dtype(rw64, rw_dtype)
    assert (rw.double().numpy() == rw64).all()
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[index % 3])
    y = run_parent(h, w_codes, w_scales, ids, bias)
    want = _sum_want(y, rw, ids, E, out_dtype)
    for fill in FILLS:
        out = run_down(h, w_codes, w_scales, ids, bias, rw, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits_nan(out, want, f"down + sum {case[:5]}, fill {fill:#x}")


@pytest.mark.parametrize("index", range(len(cases.WALK_SUM_CASES)), ids=lambda i: f"K{cases.WALK_KS[i]}")
def test_down_and_routed_sum_at_every_k_of_the_walk_bit_for_bit(index):
    """tests/moe_cases.py WALK_KS through k_mx_experts_rt's f32 epilogue and k_routed_sum, under the rule of the test above"""
    case = cases.WALK_SUM_CASES[index]
    E, N, K, T, A, _, h_dtype, out_dtype, _, rw_dtype = case
    h64, w64, bias64, ids, rw64 = cases.sum_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    h = cases.to_dtype(h64, h_dtype)
    rw = cases.to_dtype(rw64, rw_dtype)
    assert (rw.double().numpy() == rw64).all()
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[(index + 1) % 3])
    y = run_parent(h, w_codes, w_scales, ids, bias)
    _pre_is_float64(y, h64, w_codes, w_scales, bias64, ids)
    want = _sum_want(y, rw, ids, E, out_dtype)
    for fill in FILLS:
        out = run_down(h, w_codes, w_scales, ids, bias, rw, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits_nan(out, want, f"down + sum at K = {K} {case[:5]}, fill {fill:#x}")


@pytest.mark.parametrize("h_dtype", cases.X16, ids=_name)
def test_down_and_routed_sum_on_random_data_bit_for_bit(h_dtype):
    T, A, E, N, K = cases.RANDOM_SUM_SHAPE
    h, w, bias, ids = cases.random_operands(cases.RANDOM_SUM_SHAPE, h_dtype, per_slot=True)
    codes, scales = emul.quantize(w.reshape(E * N, K).numpy(), "fp4")
    w_codes, w_scales = codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32)
    rw = torch.softmax(torch.randn(T, A, generator=torch.Generator().manual_seed(39600)), dim=1)
    y = run_parent(h, w_codes, w_scales, ids, bias)
    for i, rw_dtype in enumerate(cases.DTYPES):
        r = rw.to(rw_dtype)
        for od in (torch.float32, h_dtype):
            out = run_down(h, w_codes, w_scales, ids, bias, r, od, FILLS[i % 2], cases.OFFSETS[(i + 1) % len(cases.OFFSETS)])
            _assert_bits(out, _sum_want(y, r, ids, E, od), f"random, rw {rw_dtype} -> {od}")
    # a token's bits do not depend on the rest of the call: the first token alone
    one = run_down(h[:1], w_codes, w_scales, ids[:1], bias, rw[:1], torch.float32, FILLS[0])
    _assert_bits(one, _sum_want(y[:A], rw[:1], ids[:1], E, torch.float32), "the first token alone")


# ----------------------------------------------------------------------------- 6. skipping, NaN bytes, the workspace
def _edge_sum_operands(K=cases.EDGE_SHAPE[2]):
    E, N, _, T, A = cases.EDGE_SHAPE
    h64 = (emul.lossless(T * A, K, seed=39701) * 0.125).reshape(T, A, K)
    w64 = emul.lossless(E * N, K, seed=39702).reshape(E, N, K)
    bias = torch.from_numpy(np.random.default_rng(39703).integers(1, 9, size=(E, N)).astype(F32))
    rw = torch.from_numpy((np.random.default_rng(39704).integers(1, 33, size=(T, A)) / 64.0).astype(F32))
    return cases.to_dtype(h64, torch.bfloat16), cases.quantize_experts(w64), bias, cases.EDGE_IDS.copy(), rw


def test_sum_skips_ids_outside_the_experts_without_reading_their_routing_weight_or_workspace_row():
    E, N, K, T, A = cases.EDGE_SHAPE
    h, (w_codes, w_scales), bias, ids, rw = _edge_sum_operands()
    planted, rwp = ids.copy(), rw.clone()
    for (t, a), v in zip(cases.OUT_OF_RANGE_PLACES, cases.OUT_OF_RANGE):
        planted[t, a] = np.int64(E if v is None else v).astype(np.int32)
        rwp[t, a] = float("nan")
    planted[1, :] = (-1, E)                                  # a token whose slots are all outside
    rwp[1, :] = float("nan")
    y = run_parent(h, w_codes, w_scales, ids, bias)          # the rows of the pairs that stay are those of the in-range call
    for od in cases.DTYPES:
        want = _sum_want(y, torch.nan_to_num(rwp, nan=1.0), planted, E, od)
        assert bool(torch.isfinite(want).all()) and _is_plus_zero(want[1])
        outs = []
        for fill in FILLS:                                   # the never-written workspace rows of the skipped pairs hold 0xFF.. (NaN) or 0
            for ws_fill in FILLS:
                out = run_down(h, w_codes, w_scales, planted, bias, rwp, od, fill, cases.OFFSETS[2], ws_fill=ws_fill)
                _assert_bits(out, want, f"skipped pairs, {od}, fill {fill:#x}, workspace {ws_fill:#x}")
                outs.append(out)
        assert _is_plus_zero(outs[0][1])
    for v in cases.OUT_OF_RANGE:
        every = np.full((T, A), np.int64(E if v is None else v).astype(np.int32), dtype=np.int32)
        for fill in FILLS:
            assert _is_plus_zero(run_down(h, w_codes, w_scales, every, bias, rwp, torch.bfloat16, fill)), (v, fill)


def _sum_nan_bytes(K, blocks):
    E, N, _, T, A = cases.EDGE_SHAPE
    h, (w_codes, w_scales), bias, ids, rw = _edge_sum_operands(K)
    hit = torch.zeros(T, N, dtype=torch.bool)
    hit[torch.from_numpy((ids == cases.NAN_EXPERT).any(axis=1)), cases.NAN_OUTPUT] = True
    assert 0 < int(hit[:, cases.NAN_OUTPUT].sum()) < T
    clean = run_down(h, w_codes, w_scales, ids, bias, rw, torch.float32, FILLS[0])
    assert bool(torch.isfinite(clean).all())
    for i, b in enumerate(blocks):
        planted = w_scales.copy()
        planted[cases.NAN_EXPERT, cases.NAN_OUTPUT, b] = 255
        out = run_down(h, w_codes, planted, ids, bias, rw, torch.float32, FILLS[i % 2], cases.OFFSETS[1 + i])
        assert bool(torch.isnan(out[hit]).all()), b
        _assert_bits(out[~hit], clean[~hit], f"0xFF in block {b}: every other element")


def test_sum_a_nan_scale_byte_makes_its_column_nan_for_the_tokens_routed_to_its_expert_only():
    _sum_nan_bytes(cases.EDGE_SHAPE[2], cases.NAN_BLOCKS)


@pytest.mark.parametrize("K", cases.WALK_NONFINITE_KS)
def test_sum_a_nan_scale_byte_on_a_ragged_last_step_off_wave_0(K):
    _sum_nan_bytes(K, moe_cases.walk_nan_blocks(K))


# ----------------------------------------------------------------------------- 7. the Python surface
def _block(T=6, A=4, E=5, H=160, I=96, dtype=torch.bfloat16, seed=39800):
    g = torch.Generator().manual_seed(seed)
    gate, up = torch.randn(E, I, H, generator=g) * 0.1, torch.randn(E, I, H, generator=g) * 0.1
    down = torch.randn(E, H, I, generator=g) * 0.1
    gb, ub, db = torch.randn(E, I, generator=g), torch.randn(E, I, generator=g), torch.randn(E, H, generator=g)
    x = torch.randn(T, H, generator=g).to(dtype)
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(E)[:A] for _ in range(T)]).astype(np.int32)
    rw = torch.softmax(torch.randn(T, A, generator=g), dim=1)
    layer = bnb.MoEMLPMXFP4.from_weights(gate.to(DEV), up.to(DEV), down.to(DEV), gb, ub, db, compute_dtype=dtype)
    return layer, x, ids, rw, (gate, up, down, gb, ub, db)


def _block_f64_and_bound(layer, x, ids, rw, out_dtype):
    """(r, bound): the whole block in float64 over the decoded weights and the stored biases, and an elementwise bound of the
    device's distance from it.  Gate / up: the §25 bound b1 = (H + 2) 2^-23 (|x| . |W| + |b|) on g and u; through the activation
    with |d/dg g sigma(alpha g)| <= 1.1 and |g sigma| <= |g| (the clamps are 1-Lipschitz): 1.1 (|u + 1| + b1_u) b1_g + |g| b1_u; the
    chain's own 2^-16 |h| + 2^-118 (item 2) and the rounding of h to 16 bits.  Down: dh . |Wd| plus the §25 bound over the rounded
    h; the sum: |rw| times that, plus A + 1 roundings of 2^-24 over sum |rw y|, plus the output's rounding."""
    E, H, I = layer.num_experts, layer.hidden_size, layer.intermediate_size
    u16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
    wgu = emul.decode_f64(layer.gate_up_proj_blocks.cpu().numpy().reshape(E * 2 * I, -1), layer.gate_up_proj_scales.cpu().numpy().reshape(E * 2 * I, -1)).reshape(E, 2 * I, H)
    wd = emul.decode_f64(layer.down_proj_blocks.cpu().numpy().reshape(E * H, -1), layer.down_proj_scales.cpu().numpy().reshape(E * H, -1)).reshape(E, H, I)
    bgu, bd = layer.gate_up_proj_bias.double().cpu().numpy(), layer.down_proj_bias.double().cpu().numpy()
    X, RW = x.double().numpy(), rw.double().numpy()
    T, A = ids.shape
    r, bound = np.zeros((T, H)), np.zeros((T, H))
    mag = np.zeros((T, H))
    for t in range(T):
        for a in range(A):
            e = int(ids[t, a])
            pre = wgu[e] @ X[t] + bgu[e]
            b1 = (H + 2) * 2.0 ** -23 * (np.abs(wgu[e]) @ np.abs(X[t]) + np.abs(bgu[e]))
            g, u, bg, bu = pre[0::2], pre[1::2], b1[0::2], b1[1::2]
            h = cases.glu_f64(g, u, layer.alpha, layer.limit)
            gc = np.minimum(g, layer.limit)
            uc = np.clip(u, -layer.limit, layer.limit)
            dh = 1.1 * (np.abs(uc + 1.0) + bu) * bg + (np.abs(gc) + bg) * bu
            dh = dh + cases.glu_tol(np.abs(h) + dh)
            dh = dh + u16[x.dtype] * (np.abs(h) + dh) + 2.0 ** -24
            y = wd[e] @ h + bd[e]
            s = np.abs(wd[e]) @ (np.abs(h) + dh) + np.abs(bd[e])
            dy = np.abs(wd[e]) @ dh + (I + 2) * 2.0 ** -23 * s
            r[t] += RW[t, a] * y
            bound[t] += np.abs(RW[t, a]) * dy
            mag[t] += np.abs(RW[t, a]) * (np.abs(y) + dy)
    bound += (A + 1) * 2.0 ** -24 * mag
    bound += u16[out_dtype] * (np.abs(r) + bound) + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
    return r, bound


@pytest.mark.parametrize("dtype", cases.X16, ids=_name)
def test_the_block_is_the_composition_and_stays_inside_the_bound_of_float64(dtype):
    layer, x, ids, rw, _ = _block(dtype=dtype)
    xd, idt, rwd = x.to(DEV), torch.from_numpy(ids).to(DEV), rw.to(DEV)
    args = (layer.gate_up_proj_blocks, layer.gate_up_proj_scales, layer.gate_up_proj_bias, layer.down_proj_blocks, layer.down_proj_scales,
            layer.down_proj_bias)
    with torch.no_grad():
        out = bnb.moe_mlp_mxfp4(xd, *args, idt, rwd)
        assert mlpn.last_launch() == cases.down_text(dtype, 5, 24, 4)
        h = bnb.matmul_mxfp4_experts_glu(xd, args[0], args[1], idt, args[2])
        assert mlpn.last_launch() == cases.glu_text(dtype, 5, 24) and h.dtype == dtype and tuple(h.shape) == (6, 4, 96)
        two = bnb.matmul_mxfp4_experts_sum(h, args[3], args[4], idt, rwd, args[5])
        _assert_bits(out.cpu(), two.cpu(), "moe_mlp_mxfp4 against its two halves")
        _assert_bits(layer(xd, idt, rwd).cpu(), out.cpu(), "the module's forward")
        # each half against the expert linears of §28 and the chains
        pre = bnb.matmul_mxfp4_experts(xd, args[0].reshape(5, 192, -1), args[1], idt, args[2], dtype=torch.float32).cpu().numpy().reshape(24, 192)
        ok, _, _ = cases.within_glu_bound(h.double().cpu().numpy().reshape(24, 96), cases.glu_f64(*cases.split(pre), cases.ALPHA, cases.LIMIT), dtype)
        assert ok.all()
        y = bnb.matmul_mxfp4_experts(h, args[3].reshape(5, 160, -1), args[4], idt, args[5], dtype=torch.float32).cpu().numpy().reshape(24, 160)
        _assert_bits(out.cpu(), _sum_want(y, rw, ids, 5, dtype), "the sum over §28's f32 rows")
        for od in (dtype, torch.float32):
            o = bnb.moe_mlp_mxfp4(xd, *args, idt, rwd, dtype=od)
            r, bound = _block_f64_and_bound(layer, x, ids, rw, od)
            err = np.abs(o.double().cpu().numpy() - r)
            print(f"moe_mlp_mxfp4 {_name(dtype)} -> {_name(od)}: worst err / bound = {(err / bound).max():.4f}")
            assert (err <= bound).all(), (od, float((err / bound).max()))


def test_id_and_weight_dtypes_views_a_side_stream_and_more_pairs_than_one_call():
    layer, x, ids, rw, _ = _block()
    xd, idt, rwd = x.to(DEV), torch.from_numpy(ids).to(DEV), rw.to(DEV)
    args = (layer.gate_up_proj_blocks, layer.gate_up_proj_scales, layer.gate_up_proj_bias, layer.down_proj_blocks, layer.down_proj_scales,
            layer.down_proj_bias)
    with torch.no_grad():
        want = bnb.moe_mlp_mxfp4(xd, *args, idt, rwd).cpu()
        _assert_bits(bnb.moe_mlp_mxfp4(xd, *args, idt.long(), rwd).cpu(), want, "int64 ids")
        _assert_bits(bnb.moe_mlp_mxfp4(xd, *args, idt, rwd.double()).cpu(), want, "f64 routing weights are read as f32")
        rb = rwd.to(torch.bfloat16)
        _assert_bits(bnb.moe_mlp_mxfp4(xd, *args, idt, rb).cpu(), bnb.moe_mlp_mxfp4(xd, *args, idt, rb.float()).cpu(), "bf16 routing weights")
        wide_x = torch.zeros(6, 320, dtype=x.dtype, device=DEV)[:, ::2]
        wide_x.copy_(xd)
        wide_rw = torch.zeros(4, 6, device=DEV).t()
        wide_rw.copy_(rwd)
        wide_ids = torch.zeros(4, 6, dtype=torch.int32, device=DEV).t()
        wide_ids.copy_(idt)
        assert not wide_x.is_contiguous() and not wide_rw.is_contiguous() and not wide_ids.is_contiguous()
        flat = tuple(a.reshape(a.shape[0], a.shape[1], -1) if a.dim() == 4 else a for a in args)
        _assert_bits(bnb.moe_mlp_mxfp4(wide_x, *flat, wide_ids, wide_rw).cpu(), want, "strided views, the [E, N, K / 2] layout")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ys = bnb.moe_mlp_mxfp4(xd, *args, idt, rwd)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        _assert_bits(ys.cpu(), want, "a side stream")
        empty = bnb.moe_mlp_mxfp4(xd[:0], *args, idt[:0], rwd[:0])
        assert tuple(empty.shape) == (0, 160) and empty.dtype == x.dtype
    # more pairs than one call: cut over the tokens, every piece with the bits of the same tokens in a call of their own
    T, A, E, I, K = cases.CUT_SHAPE
    big = bnb.MoEMLPMXFP4(E, K, K, compute_dtype=torch.float16, device=DEV)
    g = torch.Generator().manual_seed(39900)
    big.gate_up_proj_blocks.copy_(torch.randint(0, 256, tuple(big.gate_up_proj_blocks.shape), generator=g, dtype=torch.uint8))
    big.down_proj_blocks.copy_(torch.randint(0, 256, tuple(big.down_proj_blocks.shape), generator=g, dtype=torch.uint8))
    big.gate_up_proj_bias.copy_(torch.randn(E, 2 * K, generator=g))
    xb = (torch.randn(T, K, generator=g) * 0.25).to(torch.float16).to(DEV)
    idb = torch.from_numpy(np.random.default_rng(39901).integers(-1, E, size=(T, A)).astype(np.int32)).to(DEV)
    rwb = torch.rand(T, A, generator=g).to(DEV)
    with torch.no_grad():
        out = big(xb, idb, rwb)
        assert mlpn.last_launch() == cases.down_text(torch.float16, E, (T - cases.MAX_PAIRS // A) * A, A)
        step = cases.MAX_PAIRS // A
        _assert_bits(out[:step].cpu(), big(xb[:step], idb[:step], rwb[:step]).cpu(), "the first 256 tokens")
        _assert_bits(out[step:].cpu(), big(xb[step:], idb[step:], rwb[step:]).cpu(), "the rest")
        _assert_bits(out[7:8].cpu(), big(xb[7:8], idb[7:8], rwb[7:8]).cpu(), "one token alone")


def test_a_captured_graph_replayed_after_ids_and_routing_weights_change_in_place():
    layer, x, ids, rw, _ = _block(T=4)
    xd = x.to(DEV)
    rounds = []
    for i in range(3):
        rng = np.random.default_rng(39950 + i)
        ii = np.stack([rng.permutation(5)[:4] for _ in range(4)]).astype(np.int32)
        if i == 1:
            ii[2, 1] = -1
        rounds.append((torch.from_numpy(ii).to(DEV), torch.softmax(torch.randn(4, 4, generator=torch.Generator().manual_seed(39960 + i)), dim=1).to(DEV)))
    with torch.no_grad():
        wants = [layer(xd, ii, rr).cpu() for ii, rr in rounds]
        assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[1], wants[2])
        torch.cuda.synchronize()
        I, R = rounds[0][0].clone(), rounds[0][1].clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            layer(xd, I, R)                                  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):        # a single chain of three kernels
            out = layer(xd, I, R)
        for (ii, rr), want in list(zip(rounds, wants))[::-1]:
            I.copy_(ii)
            R.copy_(rr)
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu(), want, "a replay after ids and routing weights changed in place")


def test_the_module_loads_a_checkpoint_state_dict_and_interleaves_from_weights():
    layer, x, ids, rw, (gate, up, down, gb, ub, db) = _block()
    E, H, I = 5, 160, 96
    codes, scales = emul.quantize(torch.stack((gate, up), dim=2).reshape(E * 2 * I, H).numpy(), "fp4")
    assert np.array_equal(layer.gate_up_proj_blocks.cpu().numpy().reshape(E * 2 * I, -1), codes)
    assert np.array_equal(layer.gate_up_proj_scales.cpu().numpy().reshape(E * 2 * I, -1), scales)
    g_only, _ = emul.quantize(gate.reshape(E * I, H).numpy(), "fp4")
    assert np.array_equal(layer.gate_up_proj_blocks.cpu().numpy().reshape(E, I, 2, -1)[:, :, 0].reshape(E * I, -1), g_only)   # row 2j is gate j
    assert torch.equal(layer.gate_up_proj_bias.cpu()[:, 0::2], gb.to(torch.bfloat16)) and torch.equal(layer.gate_up_proj_bias.cpu()[:, 1::2], ub.to(torch.bfloat16))
    dg, du, dd = layer.dequantize()
    wq = emul.decode_f64(codes, scales).reshape(E, I, 2, H)
    _assert_bits(dg.cpu().contiguous(), _round_once(wq[:, :, 0], torch.bfloat16), "dequantize(): gate")
    _assert_bits(du.cpu().contiguous(), _round_once(wq[:, :, 1], torch.bfloat16), "dequantize(): up")
    assert tuple(dd.shape) == (E, H, I)
    sd = {"mlp.experts." + k: v.cpu() for k, v in layer.state_dict().items()}
    assert set(sd) == {"mlp.experts." + n for n in ("gate_up_proj_blocks", "gate_up_proj_scales", "gate_up_proj_bias", "down_proj_blocks",
                                                    "down_proj_scales", "down_proj_bias")}
    other = bnb.MoEMLPMXFP4(E, H, I, device=DEV)
    other.load_state_dict({k[len("mlp.experts."):]: v for k, v in sd.items()})
    xd, idt, rwd = x.to(DEV), torch.from_numpy(ids).to(DEV), rw.to(DEV)
    with torch.no_grad():
        _assert_bits(other(xd, idt, rwd).cpu(), layer(xd, idt, rwd).cpu(), "the module loaded from the checkpoint's keys")
