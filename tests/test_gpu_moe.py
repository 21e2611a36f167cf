"""The MXFP4 expert linears (k_mx_experts) through the C ABI on guard-banded, offset operands and outputs under the
fills 0xFF and 0x00, and through the Python surface.  The tables are tests/moe_cases.py (closed on the CPU by
tests/test_moe_host.py); the reference of the exact cases is float64 over tests/mx_emul.py's decode per expert, rounded once; the
reference of the bit rule is mbnb_mx_linear_weight_only, a kernel older than this one.

  A  lossless operands at every E, N, K, pair-count and routing edge: bit-equal
  B  ids outside [0, E)                                       C  the bit rule on random data, and the bound against float64
  D  0xFF scale bytes, and Inf / NaN activations              E  scale bytes from one end of E8M0 to the other
  F  the Python surface: both input forms, views, a side stream, more pairs than a launch, a captured graph, the module"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _mx_native as mxn, _native
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import elementwise, guard, moe_cases as cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _mx_bound, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)


def _name(v):
    return str(v).replace("torch.", "").replace(" ", "")


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _placed(name, t, fill, offset_bytes):
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def run_experts(x, w_codes, w_scales, ids, bias, out_dtype, fill, offsets=None):
    """mbnb_moe_mxfp4_experts through the C ABI, every operand carved inside guard bands at its offset (x, w_codes and w_scales in
    bytes; ids, out and bias in elements) -> y [T * A, N] on the CPU.  x [T, K] or [T, A, K]; ids int32 [T, A]."""
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    lib = moen.lib()
    T, A = ids.shape
    per_slot = x.dim() == 3
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xg = _placed("x", x.contiguous(), fill, off["x"])
    wc = _placed("w_codes", torch.as_tensor(w_codes), fill, off["w_codes"])
    wsc = _placed("w_scales", torch.as_tensor(w_scales), fill, off["w_scales"])
    ig = _placed("ids", torch.as_tensor(ids), fill, 4 * off["ids"])
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    out = guard._carve("out", (T * A, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
    st = lib.mbnb_moe_mxfp4_experts(ptr(xg.view), T, A, int(per_slot), K, _native.DTYPE_CODE[x.dtype], ptr(wc.view), ptr(wsc.view), E, N,
                                    ptr(ig.view), None if b is None else ptr(b.view), 0 if b is None else _native.DTYPE_CODE[bias.dtype],
                                    ptr(out.view), _native.DTYPE_CODE[out_dtype], stream_ptr(DEV))
    moen.check(st, "mxfp4_experts")
    torch.cuda.synchronize()
    for g in (out, xg, wc, wsc, ig) + (() if b is None else (b,)):
        assert g.violation() is None, (g.name, g.violation(), (E, N, K, T, A, x.dtype, out_dtype, fill, off))
    assert moen.last_launch() == cases.launch_text(x.dtype, per_slot, E, T * A), moen.last_launch()
    return out.view.cpu().clone()


def _exact_run(x64, x_dtype, w_codes, w_scales, ids, bias64, bias_dtype, out_dtype, what, fills=FILLS, offsets=None, want=None):
    if want is None:
        want = _round_once(cases.reference_f64(x64, cases.decode_experts(w_codes, w_scales), bias64, ids), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, bias_dtype)
    y = None
    for fill in fills:                                       # an element the launch never wrote holds the fill: it cannot match under both
        y = run_experts(cases.to_dtype(x64, x_dtype), w_codes, w_scales, ids, bias, out_dtype, fill, offsets)
        _assert_bits(y, want, f"{what}, fill {fill:#x}")
    return y


# ----------------------------------------------------------------------------- A. exact
@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.EXACT_CASES[i]))
def test_lossless_operands_bit_for_bit(index):
    case = cases.EXACT_CASES[index]
    x_dtype, out_dtype = case[6], case[7]
    x64, w64, bias64, ids = cases.exact_operands(case, index)
    w_codes, w_scales = cases.quantize_experts(w64)
    _exact_run(x64, x_dtype, w_codes, w_scales, ids, bias64, cases.DTYPES[index % 3], out_dtype, f"exact {case}",
               offsets=cases.OFFSETS[index % len(cases.OFFSETS)])


@pytest.mark.parametrize("index", range(len(cases.WALK_CASES)), ids=lambda i: f"K{cases.WALK_KS[i]}")
def test_lossless_operands_at_every_k_of_the_walk_bit_for_bit(index):
    """tests/moe_cases.py WALK_KS: ragged last steps of 1, 2 and 3 blocks and whole ones, on wave 0, a middle wave and wave 7, in a
    wave's first to fourth pass"""
    case = cases.WALK_CASES[index]
    x_dtype, out_dtype = case[6], case[7]
    x64, w64, bias64, ids = cases.exact_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    _exact_run(x64, x_dtype, w_codes, w_scales, ids, bias64, cases.DTYPES[(index + 1) % 3], out_dtype, f"walk {case}",
               offsets=cases.OFFSETS[index % len(cases.OFFSETS)])


# ----------------------------------------------------------------------------- B. ids outside [0, E)
def test_ids_outside_the_experts_give_rows_of_plus_zero_and_leave_every_other_pair_alone():
    E, N, K, T, A = cases.IDS_SHAPE
    x64, w64, bias64, ids = cases.ids_operands()
    w_codes, w_scales = cases.quantize_experts(w64)
    for od in (torch.float32, torch.bfloat16, torch.float16):
        base = _exact_run(x64, torch.bfloat16, w_codes, w_scales, ids, bias64, od, od, f"in-range ids, {od}")
        planted = ids.copy()
        for (t, a), v in zip(cases.OUT_OF_RANGE_PLACES, cases.OUT_OF_RANGE):
            planted[t, a] = np.int64(v).astype(np.int32)
        gone = torch.from_numpy(((planted < 0) | (planted >= E)).reshape(-1))
        assert int(gone.sum()) == 4
        y = _exact_run(x64, torch.bfloat16, w_codes, w_scales, planted, bias64, od, od, f"ids {cases.OUT_OF_RANGE}, {od}")
        assert bool((y[gone].view(torch.int32 if od == torch.float32 else torch.int16) == 0).all())      # +0.0: the sign bit clear, no bias
        _assert_bits(y[~gone], base[~gone], "the pairs whose id stayed")
        for v in cases.OUT_OF_RANGE:
            every = np.full((T, A), np.int64(v).astype(np.int32), dtype=np.int32)
            y = _exact_run(x64, torch.float16, w_codes, w_scales, every, bias64, od, od, f"every id {v}, {od}", fills=FILLS[:1])
            assert bool((y.view(torch.int32 if od == torch.float32 else torch.int16) == 0).all())


# ----------------------------------------------------------------------------- C. the bit rule
_RANDOM = {}


def _random_weights(shape):
    if shape not in _RANDOM:
        T, A, E, N, K = shape
        _, w, _, _ = cases.random_operands(shape, torch.bfloat16)
        codes, scales = bnb.quantize_mxfp4(w.reshape(E * N, K).to(DEV))
        codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
        assert all((a == b).all() for a, b in zip((codes, scales), emul.quantize(w.reshape(E * N, K).numpy(), "fp4")))
        _RANDOM[shape] = (codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32), emul.decode_f64(codes, scales, "fp4").reshape(E, N, K))
    return _RANDOM[shape]


def _parent_rows(rows, flat_ids, w_codes, w_scales, bias, out_dtype):
    """Every pair through mbnb_mx_linear_weight_only: its row duplicated to 2 rows (the MFMA form) against W[id], bias[id] -> [P, N]"""
    lib = mxn.lib()
    E, N = w_codes.shape[:2]
    K = rows.shape[1]
    wc, wsc = torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)
    b = None if bias is None else bias.to(DEV)
    two = rows.to(DEV).repeat_interleave(2, dim=0).contiguous()
    out = torch.empty(rows.shape[0], 2, N, dtype=out_dtype, device=DEV)
    for p, e in enumerate(flat_ids.tolist()):
        st = lib.mbnb_mx_linear_weight_only(ptr(two[2 * p:]), 2, K, _native.DTYPE_CODE[rows.dtype], ptr(wc[e]), ptr(wsc[e]), N,
                                            None if b is None else ptr(b[e]), 0 if b is None else _native.DTYPE_CODE[b.dtype], ptr(out[p]),
                                            _native.DTYPE_CODE[out_dtype], stream_ptr(DEV))
        mxn.check(st, "linear_weight_only")
        assert mxn.last_launch() == f"mx_decode_mfma {'bf16' if rows.dtype == torch.bfloat16 else 'f16'} MT16"
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0].view(torch.uint8), out[:, 1].view(torch.uint8))
    return out[:, 0].cpu().clone()


@pytest.mark.parametrize("per_slot", (False, True), ids=("shared", "slot"))
@pytest.mark.parametrize("index", range(len(cases.RANDOM_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.RANDOM_CASES[i]))
def test_every_pair_has_the_bits_of_the_weight_only_linear_whatever_else_is_in_the_call(index, per_slot):
    shape, x_dtype, out_dtype = cases.RANDOM_CASES[index]
    T, A, E, N, K = shape
    x, _, bias, ids = cases.random_operands(shape, x_dtype, per_slot)
    w_codes, w_scales, wq = _random_weights(shape)
    rows = x.reshape(T * A, K) if per_slot else x.repeat_interleave(A, dim=0)
    want = _parent_rows(rows, ids.reshape(-1), w_codes, w_scales, bias, out_dtype)
    y = run_experts(x, w_codes, w_scales, ids, bias, out_dtype, FILLS[index % 2], cases.OFFSETS[(index + 1) % len(cases.OFFSETS)])
    _assert_bits(y, want, f"{shape}, {x_dtype} -> {out_dtype}: every pair against mbnb_mx_linear_weight_only")
    # the same outputs inside the project's elementwise bound against float64 over the decoded weight
    r = torch.empty(T * A, N, dtype=torch.float64)
    bound = torch.empty_like(r)
    flat = ids.reshape(-1)
    for e in np.unique(flat):
        sel = torch.from_numpy(flat == e)
        r[sel], bound[sel] = _mx_bound(rows[sel].double().numpy(), wq[e], bias[e], out_dtype)
    none = torch.zeros(r.shape, dtype=torch.bool)
    ratio = elementwise._compare(y, r, bound, none, none, none, moen.last_launch(), "y = x . W[e]^T + b[e]")
    print(f"mx_experts random {shape}, {'slot' if per_slot else 'shared'}, x {x_dtype} -> {out_dtype}: worst err / bound = {ratio:.4f}")
    # another batch: the first two tokens kept (moved to the end), every other token replaced, the routing of the others redrawn
    keep = [0, 1]
    g = torch.Generator().manual_seed(26500 + index)
    x2 = torch.randn(x.shape, generator=g).to(x_dtype)
    ids2 = np.random.default_rng(26600 + index).integers(0, E, size=(T, A)).astype(np.int32)
    x2[T - 2:], ids2[T - 2:] = x[keep], ids[keep]
    y2 = run_experts(x2, w_codes, w_scales, ids2, bias, out_dtype, FILLS[(index + 1) % 2]).reshape(T, A, N)
    _assert_bits(y2[T - 2:], y.reshape(T, A, N)[keep], "the kept tokens inside another batch")
    # and alone
    y3 = run_experts(x[:1], w_codes, w_scales, ids[:1], bias, out_dtype, FILLS[0]).reshape(1, A, N)
    _assert_bits(y3, y.reshape(T, A, N)[:1], "the first token alone")


# ----------------------------------------------------------------------------- D. NaN and Inf
def _nan_bytes(shape, x64, w64, ids, blocks):
    """a 0xFF byte in each of `blocks` in turn, with the activations of that block as they are and zeroed -> (codes, scales, clean, hit)"""
    E, N, K, T, A = shape
    w_codes, w_scales = cases.quantize_experts(w64)
    clean = _exact_run(x64, torch.bfloat16, w_codes, w_scales, ids, None, None, torch.float32, "clean")
    hit = torch.zeros(T * A, N, dtype=torch.bool)
    hit[torch.from_numpy(ids.reshape(-1) == cases.NAN_EXPERT), cases.NAN_COLUMN] = True
    assert 0 < int(hit.sum()) < T * A
    for i, b in enumerate(blocks):
        planted = w_scales.copy()
        planted[cases.NAN_EXPERT, cases.NAN_COLUMN, b] = 255
        for zero_x in (False, True):
            xb = x64.copy()
            if zero_x:
                xb[:, 32 * b:32 * b + 32] = 0.0
            want = _round_once(cases.reference_f64(xb, w64, None, ids), torch.float32)
            y = run_experts(cases.to_dtype(xb, (torch.bfloat16, torch.float16)[i % 2]), w_codes, planted, ids, None, torch.float32, FILLS[(i + zero_x) % 2])
            assert bool(torch.isnan(y[hit]).all()), (b, zero_x)
            _assert_bits(y[~hit], want[~hit], f"0xFF in block {b}, x block zero: {zero_x}: every other element")
    return w_codes, w_scales, clean, hit


def test_a_nan_scale_byte_makes_its_column_nan_for_the_pairs_of_its_expert_only():
    E, N, K, T, A = cases.NAN_SHAPE
    x64, w64, ids = cases.nan_operands()
    w_codes, w_scales, clean, hit = _nan_bytes(cases.NAN_SHAPE, x64, w64, ids, cases.NAN_BLOCKS)
    planted = w_scales.copy()
    planted[cases.NAN_EXPERT, cases.NAN_COLUMN, list(cases.NAN_BLOCKS)] = 255
    bias = torch.ones(E, N)
    y = run_experts(cases.to_dtype(x64, torch.bfloat16), w_codes, planted, ids, bias, torch.bfloat16, FILLS[0])
    assert bool(torch.isnan(y[hit]).all())
    _assert_bits(y[~hit], (clean + 1.0).to(torch.bfloat16)[~hit], "several 0xFF bytes, a bias: every other element")


def _bad_activations(shape, x64, w64, ids, ks, x_dtype):
    """an Inf, a -Inf and a NaN at each k of `ks` of one token's row in turn"""
    E, N, K, T, A = shape
    w_codes, w_scales = cases.quantize_experts(w64)
    clean = _round_once(cases.reference_f64(x64, w64, None, ids), torch.float32).reshape(T, A, N)
    other = torch.tensor([t != cases.X_BAD_TOKEN for t in range(T)])
    n = 0
    for ki, k in enumerate(ks):
        for vi, v in enumerate(cases.X_BAD_VALUES):
            xb = x64.copy()
            xb[cases.X_BAD_TOKEN, k] = v
            want = cases.reference_f64(xb, w64, None, ids).reshape(T, A, N)[cases.X_BAD_TOKEN]   # elementwise IEEE: Inf * 0 = NaN
            assert not np.isfinite(want).any()
            y = run_experts(cases.to_dtype(xb, x_dtype), w_codes, w_scales, ids, None, torch.float32, FILLS[(ki + vi) % 2]).reshape(T, A, N)
            got = y[cases.X_BAD_TOKEN].double().numpy()
            assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (k, v, got, want)
            _assert_bits(y[other], clean[other], f"{v} at k = {k}: the other tokens")
            n += int(np.isinf(want).any())
    assert n > 0


@pytest.mark.parametrize("x_dtype", cases.X16, ids=_name)
def test_inf_and_nan_in_a_token_row_touch_that_tokens_pairs_only(x_dtype):
    x64, w64, ids = cases.nan_operands()
    _bad_activations(cases.NAN_SHAPE, x64, w64, ids, cases.X_BAD_KS, x_dtype)


@pytest.mark.parametrize("K", cases.WALK_NONFINITE_KS)
def test_nan_bytes_inf_and_nan_on_a_ragged_last_step_off_wave_0(K):
    """The 0xFF byte on the first block of the last step and on block KB - 1, the Inf and the NaN at the first k of the last step and
    at k = K - 1, where that step runs on wave 7 (K = 992) and on wave 6 in its third pass (K = 2880, the model's size)"""
    E, N, _, T, A = cases.NAN_SHAPE
    x64, w64, ids = cases.walk_nan_operands(K)
    _nan_bytes((E, N, K, T, A), x64, w64, ids, cases.walk_nan_blocks(K))
    _bad_activations((E, N, K, T, A), x64, w64, ids, cases.walk_bad_ks(K), cases.X16[cases.WALK_NONFINITE_KS.index(K) % 2])


# ----------------------------------------------------------------------------- E. scale bytes
@pytest.mark.parametrize("index", range(len(cases.WIDE_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.WIDE_CASES[i]))
def test_scale_bytes_from_end_to_end_bit_for_bit(index):
    which, out_dtype = cases.WIDE_CASES[index]
    x64, w64, w_codes, w_scales, ids, _, _ = cases.wide_operands(which)
    y = _exact_run(x64, torch.bfloat16, w_codes, w_scales, ids, None, None, out_dtype, f"wide {which}",
                   want=_round_once(cases.reference_f64(x64, w64, None, ids), out_dtype))
    assert bool(torch.isfinite(y).all()) and bool((y != 0).all())


# ----------------------------------------------------------------------------- F. the Python surface
def _surface_operands(T=5, A=3, E=4, N=9, K=160, seed=29000):
    x64 = emul.lossless(T * A, K, seed=seed).reshape(T, A, K)
    w64 = emul.lossless(E * N, K, seed=seed + 1).reshape(E, N, K)
    bias64 = np.random.default_rng(seed + 2).integers(-8, 9, size=(E, N)).astype(np.float64)
    ids = np.random.default_rng(seed + 3).integers(0, E, size=(T, A)).astype(np.int32)
    w_codes, w_scales = cases.quantize_experts(w64)
    return x64, w64, bias64, ids, torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV)


def test_both_input_forms_id_dtypes_views_and_the_blocks_layout():
    T, A, E, N, K = 5, 3, 4, 9, 160
    x64, w64, bias64, ids, wc, wsc = _surface_operands(T, A, E, N, K)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    idt = torch.from_numpy(ids).to(DEV)
    slot = cases.to_dtype(x64, torch.bfloat16).to(DEV)
    want_slot = _round_once(cases.reference_f64(x64, w64, bias64, ids), torch.bfloat16).reshape(T, A, N)
    want_shared = _round_once(cases.reference_f64(x64[:, 0], w64, bias64, ids), torch.bfloat16).reshape(T, A, N)
    y = bnb.matmul_mxfp4_experts(slot, wc, wsc, idt, bias)
    assert tuple(y.shape) == (T, A, N) and y.dtype == torch.bfloat16 and moen.last_launch() == f"mx_experts bf16 slot E{E} P{T * A}"
    _assert_bits(y.cpu(), want_slot, "a row per slot")
    shared = slot[:, 0]
    assert not shared.is_contiguous()
    y = bnb.matmul_mxfp4_experts(shared, wc, wsc, idt, bias)
    assert moen.last_launch() == f"mx_experts bf16 shared E{E} P{T * A}"
    _assert_bits(y.cpu(), want_shared, "a shared row, a strided view")
    _assert_bits(bnb.matmul_mxfp4_experts(shared, wc, wsc, idt.long(), bias).cpu(), want_shared, "int64 ids")
    _assert_bits(bnb.matmul_mxfp4_experts(shared, wc, wsc, idt.to(torch.int16).t().contiguous().t(), bias).cpu(), want_shared, "int16 ids, a transposed view")
    _assert_bits(bnb.matmul_mxfp4_experts(shared, wc.reshape(E, N, K // 32, 16), wsc, idt, bias).cpu(), want_shared, "the blocks layout")
    wide = torch.zeros(E, N, K, dtype=torch.uint8, device=DEV)[:, :, ::2]
    wide.copy_(wc)
    sv = torch.zeros(E, 2 * N, K // 32, dtype=torch.uint8, device=DEV)[:, ::2]
    sv.copy_(wsc)
    assert not wide.is_contiguous() and not sv.is_contiguous()
    _assert_bits(bnb.matmul_mxfp4_experts(shared, wide, sv, idt, bias.float()).cpu(), want_shared, "strided weight and scale views, an f32 bias")
    y = bnb.matmul_mxfp4_experts(slot.to(torch.float16), wc, wsc, idt, dtype=torch.float32)
    assert y.dtype == torch.float32 and moen.last_launch() == f"mx_experts f16 slot E{E} P{T * A}"
    _assert_bits(y.cpu().reshape(T * A, N), _round_once(cases.reference_f64(x64, w64, None, ids), torch.float32), "f16 rows into f32, no bias")
    y = bnb.matmul_mxfp4_experts(shared[:0], wc, wsc, idt[:0], bias)
    assert tuple(y.shape) == (0, A, N) and y.dtype == torch.bfloat16


def test_more_pairs_than_one_launch_are_cut_over_the_tokens():
    T, A, E, N, K = cases.CUT_SHAPE
    x64 = emul.lossless(T, K, seed=29101)
    w64 = emul.lossless(E * N, K, seed=29102).reshape(E, N, K)
    bias64 = np.random.default_rng(29103).integers(-8, 9, size=(E, N)).astype(np.float64)
    ids = np.random.default_rng(29104).integers(-1, E, size=(T, A)).astype(np.int32)          # the padding id among them
    w_codes, w_scales = cases.quantize_experts(w64)
    y = bnb.matmul_mxfp4_experts(cases.to_dtype(x64, torch.float16).to(DEV), torch.from_numpy(w_codes).to(DEV), torch.from_numpy(w_scales).to(DEV),
                                 torch.from_numpy(ids).to(DEV), cases.to_dtype(bias64, torch.float16).to(DEV), dtype=torch.float32)
    assert moen.last_launch() == f"mx_experts f16 shared E{E} P{(T - cases.MAX_PAIRS // A) * A}"
    _assert_bits(y.cpu().reshape(T * A, N), _round_once(cases.reference_f64(x64, w64, bias64, ids), torch.float32), "300 tokens x 4 slots")


def test_a_side_stream_and_a_captured_graph_replayed_after_ids_and_input_change_in_place():
    T, A, E, N, K = 5, 3, 4, 9, 160
    x64, w64, bias64, ids, wc, wsc = _surface_operands(T, A, E, N, K)
    bias = cases.to_dtype(bias64, torch.bfloat16).to(DEV)
    rounds = []
    for i in range(3):
        xi = emul.lossless(T, K, seed=29201 + i)
        ii = np.random.default_rng(29301 + i).integers(-1 if i == 1 else 0, E, size=(T, A)).astype(np.int32)
        rounds.append((cases.to_dtype(xi, torch.bfloat16).to(DEV), torch.from_numpy(ii).to(DEV),
                       _round_once(cases.reference_f64(xi, w64, bias64, ii), torch.bfloat16).reshape(T, A, N)))
    with torch.no_grad():
        for xi, ii, want in rounds:
            _assert_bits(bnb.matmul_mxfp4_experts(xi, wc, wsc, ii, bias).cpu(), want, "eager")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ys = bnb.matmul_mxfp4_experts(rounds[1][0], wc, wsc, rounds[1][1], bias)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        _assert_bits(ys.cpu(), rounds[1][2], "a side stream")
        # one captured graph, a single chain, replayed after the ids and the input are overwritten in place
        X, I = rounds[0][0].clone(), rounds[0][1].clone()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            bnb.matmul_mxfp4_experts(X, wc, wsc, I, bias)                 # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = bnb.matmul_mxfp4_experts(X, wc, wsc, I, bias)
        for xi, ii, want in rounds[::-1]:
            X.copy_(xi)
            I.copy_(ii)
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu(), want, "a replay after ids and input changed in place")


def test_the_module_against_its_dequantised_weights():
    T, A, E, N, K = 6, 2, 5, 33, 1056
    g = torch.Generator().manual_seed(29401)
    w = (torch.randn(E, N, K, generator=g) * 0.02).to(torch.bfloat16)
    bias = torch.randn(E, N, generator=g).to(torch.bfloat16)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    ids = np.stack([np.random.default_rng(29402 + t).permutation(E)[:A] for t in range(T)]).astype(np.int32)
    layer = bnb.ExpertsMXFP4.from_weights(w.to(DEV), bias.to(DEV))
    assert layer.num_experts == E and layer.compute_dtype == torch.bfloat16 and layer.device.type == "cuda"
    codes, scales = emul.quantize(w.reshape(E * N, K).float().numpy(), "fp4")
    assert np.array_equal(layer.weight.cpu().numpy().reshape(E * N, -1), codes) and np.array_equal(layer.weight_scales.cpu().numpy().reshape(E * N, -1), scales)
    wq = emul.decode_f64(codes, scales, "fp4").reshape(E, N, K)
    deq = layer.dequantize()
    assert tuple(deq.shape) == (E, N, K) and deq.dtype == torch.bfloat16
    _assert_bits(deq.cpu(), _round_once(wq, torch.bfloat16), "dequantize()")                # E2M1 x 2^e is exact in bf16
    with torch.no_grad():
        y = layer(x.to(DEV), torch.from_numpy(ids).to(DEV))
    assert tuple(y.shape) == (T, A, N) and y.dtype == torch.bfloat16
    # a torch gather-matmul over dequantize(), and float64 with the bound
    idl = torch.from_numpy(ids).long()
    gathered = torch.einsum("tk,tank->tan", x.double(), deq.cpu().double()[idl]) + bias.double()[idl]
    r = torch.empty(T * A, N, dtype=torch.float64)
    bound = torch.empty_like(r)
    rows = x.repeat_interleave(A, dim=0)
    for p, e in enumerate(ids.reshape(-1).tolist()):
        r[p:p + 1], bound[p:p + 1] = _mx_bound(rows[p:p + 1].double().numpy(), wq[e], bias[e], torch.bfloat16)
    assert torch.allclose(r, gathered.reshape(T * A, N), rtol=1e-12, atol=1e-12)
    none = torch.zeros(r.shape, dtype=torch.bool)
    ratio = elementwise._compare(y.cpu().reshape(T * A, N), r, bound, none, none, none, moen.last_launch(), "ExpertsMXFP4")
    print(f"ExpertsMXFP4 {(T, A, E, N, K)}: worst err / bound = {ratio:.4f}")
