"""The grouped GEMM over MXFP4 experts (k_plan_count, k_plan_fill, k_mx_experts_grouped, k_routed_sum) through the C ABI
on guard-banded, offset operands, outputs, plan and workspace under the fills 0xFF and 0x00, and through the Python surface.  The
tables and the numpy plan are tests/moegemm_cases.py (closed on the CPU by tests/test_moegemm_host.py).  The yardsticks are kernels
older than these: mbnb_moe_mxfp4_experts, mbnb_moemlp_gate_up_glu and mbnb_moemlp_down_sum, cut into calls of at most 1024 pairs.

  1  the plan, integer for integer                  2  lossless operands against float64 rounded once
  3  the bit rule: every pair, the GLU form and the down + sum form against the decode launches; the elementwise bound
  4  0xFF scale bytes, Inf / NaN rows, scale bytes from end to end, ids outside [0, E)
  4b the GLU and down + sum forms past one column tile, every id outside across every column tile, 128 and 1024 experts
     (2 to 4 also at every K of moe_cases.WALK_KS: the ragged last step on every kind of wave and pass, the model's K = 2880)
  5  the Python surface: the three functions, the cut, the automatic route, a captured graph"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _moegemm_native as gn, _moemlp_native as mlpn, _native
from mps_bitsandbytes_amd import functional as F
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import elementwise, guard, moe_cases, moegemm_cases as cases, moemlp_cases, mx_emul as emul
from tests.test_gpu_mx import _assert_bits, _mx_bound, _round_once

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)
CODE = _native.DTYPE_CODE
ALPHA, LIMIT = moemlp_cases.ALPHA, moemlp_cases.LIMIT


def _name(v):
    return str(v).replace("torch.", "").replace(" ", "")[:40]


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _placed(name, t, fill, offset_bytes):
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16) == 0).all())


def _assert_bits_nan(got, want, what):
    """every NaN on one bit pattern: which NaN an Inf * 0 gives is the only thing numpy and the device may differ in"""
    got, want = got.clone(), want.clone()
    got[torch.isnan(got)] = float("nan")
    want[torch.isnan(want)] = float("nan")
    _assert_bits(got, want, what)


def _check_guards(guards, what):
    for g in guards:
        assert g.violation() is None, (g.name, g.violation(), what)


def _plan_into(ig, P, E, fill, offset):
    """mbnb_moegemm_plan into a carved buffer of exactly plan_bytes -> (the guard, the plan as the dict of cases.plan_reference)"""
    lib = gn.lib()
    need = int(lib.mbnb_moegemm_plan_bytes(P, E))
    assert need == cases.plan_bytes(P, E)
    pg = guard._carve("plan", (need // 4,), torch.int32, DEV, fill, offset)
    gn.check(lib.mbnb_moegemm_plan(ptr(ig.view), P, E, ptr(pg.view), need, stream_ptr(DEV)), "plan")
    assert gn.last_launch() == cases.plan_text(E, P), gn.last_launch()
    return pg, need


def run_plan(ids, E, fill, offsets=None):
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    flat = torch.as_tensor(np.asarray(ids).reshape(-1))
    ig = _placed("ids", flat, fill, 4 * off["ids"])
    pg, _ = _plan_into(ig, flat.numel(), E, fill, off["plan"])
    torch.cuda.synchronize()
    _check_guards((pg, ig), (E, flat.numel(), fill, off))
    return cases.plan_from_words(pg.view.cpu().numpy(), flat.numel(), E)


def run_grouped(form, x, w_codes, w_scales, ids, bias, out_dtype, fill, offsets=None, alpha=ALPHA, limit=LIMIT, rw=None, ws_fill=None):
    """One projection of libmbnb_moegemm.so through the C ABI, every operand, the plan and the workspace carved inside guard bands at
    its offset -> the output on the CPU: `plain` [T * A, N], `glu` [T * A, N / 2], `down` [T, N].  The plan the launch read is
    checked against the numpy plan."""
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    lib = gn.lib()
    T, A = ids.shape
    P = T * A
    per_slot = x.dim() == 3
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xg = _placed("x", x.contiguous(), fill, off["x"])
    wc = _placed("w_codes", torch.as_tensor(w_codes), fill, off["w_codes"])
    wsc = _placed("w_scales", torch.as_tensor(w_scales), fill, off["w_scales"])
    ig = _placed("ids", torch.as_tensor(ids), fill, 4 * off["ids"])
    b = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    pg, plan_bytes = _plan_into(ig, P, E, fill, off["plan"])
    head = (ptr(wc.view), ptr(wsc.view), E)
    btail = (None if b is None else ptr(b.view), 0 if b is None else CODE[bias.dtype])
    guards = [xg, wc, wsc, ig, pg] + ([] if b is None else [b])
    if form == "plain":
        out = guard._carve("out", (P, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
        st = lib.mbnb_moegemm_experts(ptr(xg.view), T, A, int(per_slot), K, CODE[x.dtype], *head, N, ptr(ig.view), *btail, ptr(out.view),
                                      CODE[out_dtype], ptr(pg.view), plan_bytes, stream_ptr(DEV))
        text = cases.experts_text(x.dtype, per_slot, E, P)
    elif form == "glu":
        out = guard._carve("out", (P, N // 2), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
        st = lib.mbnb_moegemm_gate_up_glu(ptr(xg.view), T, A, K, CODE[x.dtype], *head, N // 2, ptr(ig.view), *btail, alpha, limit, ptr(out.view),
                                          CODE[out_dtype], ptr(pg.view), plan_bytes, stream_ptr(DEV))
        text = cases.glu_text(x.dtype, E, P)
    else:
        rg = _placed("rw", rw, fill, off["rw"] * _esize(rw.dtype))
        need = int(lib.mbnb_moegemm_workspace_bytes(P, N))
        assert need == -(-P * N * 4 // 256) * 256
        ws = guard._carve("workspace", (need,), torch.uint8, DEV, fill if ws_fill is None else ws_fill, off["ws"])
        out = guard._carve("out", (T, N), out_dtype, DEV, fill, off["out"] * _esize(out_dtype))
        st = lib.mbnb_moegemm_down_sum(ptr(xg.view), T, A, K, CODE[x.dtype], *head, N, ptr(ig.view), *btail, ptr(rg.view), CODE[rw.dtype],
                                       ptr(out.view), CODE[out_dtype], ptr(ws.view), need, ptr(pg.view), plan_bytes, stream_ptr(DEV))
        text = cases.down_text(x.dtype, E, P, A)
        guards += [rg, ws]
    gn.check(st, form)
    torch.cuda.synchronize()
    _check_guards([out] + guards, (form, E, N, K, T, A, x.dtype, out_dtype, fill, off))
    assert gn.last_launch() == text, gn.last_launch()
    assert cases.same_plan(cases.plan_from_words(pg.view.cpu().numpy(), P, E), cases.plan_reference(ids, E))
    return out.view.cpu().clone()


# ----------------------------------------------------------------------------- the yardsticks, cut into calls of <= 1024 pairs
def _cuts(T, A):
    step = max(1, cases.YARDSTICK_MAX_PAIRS // A)
    return [(t0, min(T, t0 + step)) for t0 in range(0, T, step)]


def yard_experts(x, w_codes, w_scales, ids, bias, out_dtype):
    T, A = ids.shape
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xd, wc, wsc, ig = x.to(DEV).contiguous(), torch.as_tensor(w_codes).to(DEV).contiguous(), torch.as_tensor(w_scales).to(DEV).contiguous(), torch.as_tensor(ids).to(DEV)
    b = None if bias is None else bias.to(DEV)
    out = torch.empty(T, A, N, dtype=out_dtype, device=DEV)
    for t0, t1 in _cuts(T, A):
        st = moen.lib().mbnb_moe_mxfp4_experts(ptr(xd[t0:t1]), t1 - t0, A, int(x.dim() == 3), K, CODE[x.dtype], ptr(wc), ptr(wsc), E, N, ptr(ig[t0:t1]),
                                               None if b is None else ptr(b), 0 if b is None else CODE[b.dtype], ptr(out[t0:t1]), CODE[out_dtype],
                                               stream_ptr(DEV))
        moen.check(st, "mxfp4_experts")
        assert moen.last_launch() == moe_cases.launch_text(x.dtype, x.dim() == 3, E, (t1 - t0) * A)
    torch.cuda.synchronize()
    return out.reshape(T * A, N).cpu()


def yard_glu(x, w_codes, w_scales, ids, bias, out_dtype, alpha=ALPHA, limit=LIMIT):
    T, A = ids.shape
    K, (E, N) = x.shape[-1], w_codes.shape[:2]
    xd, wc, wsc, ig = x.to(DEV).contiguous(), torch.as_tensor(w_codes).to(DEV).contiguous(), torch.as_tensor(w_scales).to(DEV).contiguous(), torch.as_tensor(ids).to(DEV)
    b = None if bias is None else bias.to(DEV)
    out = torch.empty(T, A, N // 2, dtype=out_dtype, device=DEV)
    for t0, t1 in _cuts(T, A):
        st = mlpn.lib().mbnb_moemlp_gate_up_glu(ptr(xd[t0:t1]), t1 - t0, A, K, CODE[x.dtype], ptr(wc), ptr(wsc), E, N // 2, ptr(ig[t0:t1]),
                                                None if b is None else ptr(b), 0 if b is None else CODE[b.dtype], alpha, limit, ptr(out[t0:t1]),
                                                CODE[out_dtype], stream_ptr(DEV))
        mlpn.check(st, "gate_up_glu")
    torch.cuda.synchronize()
    return out.reshape(T * A, N // 2).cpu()


def yard_down(h, w_codes, w_scales, ids, bias, rw, out_dtype):
    T, A = ids.shape
    K, (E, N) = h.shape[-1], w_codes.shape[:2]
    hd, wc, wsc, ig = h.to(DEV).contiguous(), torch.as_tensor(w_codes).to(DEV).contiguous(), torch.as_tensor(w_scales).to(DEV).contiguous(), torch.as_tensor(ids).to(DEV)
    b, rd = None if bias is None else bias.to(DEV), rw.to(DEV)
    out = torch.empty(T, N, dtype=out_dtype, device=DEV)
    need = mlpn.workspace_bytes(min(T, _cuts(T, A)[0][1]), A, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for t0, t1 in _cuts(T, A):
        st = mlpn.lib().mbnb_moemlp_down_sum(ptr(hd[t0:t1]), t1 - t0, A, K, CODE[h.dtype], ptr(wc), ptr(wsc), E, N, ptr(ig[t0:t1]),
                                             None if b is None else ptr(b), 0 if b is None else CODE[b.dtype], ptr(rd[t0:t1]), CODE[rw.dtype],
                                             ptr(out[t0:t1]), CODE[out_dtype], ptr(ws), need, stream_ptr(DEV))
        mlpn.check(st, "down_sum")
    torch.cuda.synchronize()
    return out.cpu()


# ----------------------------------------------------------------------------- 1. the plan
_PLAN_CASES = cases.plan_cases()


@pytest.mark.parametrize("index", range(len(_PLAN_CASES)), ids=lambda i: f"E{_PLAN_CASES[i][0]}-P{_PLAN_CASES[i][1].size}-{i}")
def test_the_plan_integer_for_integer(index):
    E, ids = _PLAN_CASES[index]
    want = cases.plan_reference(ids, E)
    for fill in FILLS:                                       # a word the launches never wrote holds the fill: it cannot match under both
        got = run_plan(ids, E, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        for key in ("counts", "tiles", "sorted"):
            assert np.array_equal(np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1)), (key, E, ids.size, fill)
        assert (got["n_tiles"], got["n_listed"]) == (want["n_tiles"], want["n_listed"])


# ----------------------------------------------------------------------------- 2. exact
@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.EXACT_CASES[i]))
def test_lossless_operands_bit_for_bit(index):
    case = cases.EXACT_CASES[index]
    x_dtype, out_dtype = case[6], case[7]
    x64, w64, bias64, ids = cases.exact_operands(case, index)
    w_codes, w_scales = cases.quantize_experts(w64)
    want = _round_once(moe_cases.reference_f64(x64, moe_cases.decode_experts(w_codes, w_scales), bias64, ids), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[index % 3])
    for fill in FILLS:
        y = run_grouped("plain", cases.to_dtype(x64, x_dtype), w_codes, w_scales, ids, bias, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits(y, want, f"exact {case}, fill {fill:#x}")


def _walk_id(i):
    return f"K{cases.WALK_KS[i]}"


@pytest.mark.parametrize("index", range(len(cases.WALK_CASES)), ids=_walk_id)
def test_lossless_operands_at_every_k_of_the_walk_bit_for_bit(index):
    """tests/moe_cases.py WALK_KS through the kernel's own K walk: a full row tile and a one-row tile, a second column tile of one
    live column; ragged last steps of 1 to 3 blocks and whole ones on wave 0, middle waves and wave 7, in a wave's first to fourth pass"""
    case = cases.WALK_CASES[index]
    x_dtype, out_dtype = case[6], case[7]
    x64, w64, bias64, ids = cases.exact_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    want = _round_once(cases.reference("plain", x64, w_codes, w_scales, ids, bias64), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[(index + 1) % 3])
    for fill in FILLS:
        y = run_grouped("plain", cases.to_dtype(x64, x_dtype), w_codes, w_scales, ids, bias, out_dtype, fill, cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits(y, want, f"walk {case}, fill {fill:#x}")


@pytest.mark.parametrize("index", range(len(cases.WALK_GLU_CASES)), ids=_walk_id)
def test_glu_with_alpha_zero_at_every_k_of_the_walk_bit_for_bit(index):
    """With alpha = 0 every step of the chain is a correctly rounded IEEE operation (tests/moemlp_cases.py glu_f32), so the yardstick
    is float64 over the decoded weights, rounded once to the f32 pre-activation, through that chain.  N = C + 2: the second column
    tile holds one (gate, up) pair"""
    case = cases.WALK_GLU_CASES[index]
    E, I, K, T, A, _, x_dtype, out_dtype, _, limit = case
    x64, w64, bias64, ids = cases.glu_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    want = _round_once(cases.reference("glu", x64, w_codes, w_scales, ids, bias64, 0.0, limit).astype(np.float64), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[(index + 2) % 3])
    for fill in FILLS:
        h = run_grouped("glu", cases.to_dtype(x64, x_dtype), w_codes, w_scales, ids, bias, out_dtype, fill, cases.OFFSETS[(index + 1) % len(cases.OFFSETS)],
                        alpha=0.0, limit=limit)
        _assert_bits(h, want, f"walk glu {case[:5]}, fill {fill:#x}")


@pytest.mark.parametrize("index", range(len(cases.WALK_SUM_CASES)), ids=_walk_id)
def test_down_and_routed_sum_at_every_k_of_the_walk_bit_for_bit(index):
    """float64 over the decoded weights, rounded once to the f32 workspace, through tests/moemlp_cases.py routed_sum_f32 (one fmaf per
    slot, in slot order): exact.  N = C + 1: the second column tile's rows of the workspace hold one column"""
    case = cases.WALK_SUM_CASES[index]
    E, N, K, T, A, _, h_dtype, out_dtype, _, rw_dtype = case
    h64, w64, bias64, ids, rw64 = cases.sum_operands(case, cases.WALK_SEED + index)
    w_codes, w_scales = cases.quantize_experts(w64)
    rw = cases.to_dtype(rw64, rw_dtype)
    assert (rw.double().numpy() == rw64).all()
    want = _round_once(cases.reference("down", h64, w_codes, w_scales, ids, bias64, rw=rw64).astype(np.float64), out_dtype)
    bias = None if bias64 is None else cases.to_dtype(bias64, cases.DTYPES[index % 3])
    for i, fill in enumerate(FILLS):
        out = run_grouped("down", cases.to_dtype(h64, h_dtype), w_codes, w_scales, ids, bias, out_dtype, fill, cases.OFFSETS[(index + 2) % len(cases.OFFSETS)],
                          rw=rw, ws_fill=FILLS[(index + i) % 2])
        _assert_bits_nan(out, want, f"walk down + sum {case[:5]}, fill {fill:#x}")


# ----------------------------------------------------------------------------- 3. the bit rule
_WEIGHTS = {}


def _weights(nk):
    if nk not in _WEIGHTS:
        N, K = nk
        w, bias = cases.random_weights(nk)
        codes, scales = emul.quantize(w.reshape(cases.RANDOM_E * N, K).numpy(), "fp4")
        _WEIGHTS[nk] = (codes.reshape(cases.RANDOM_E, N, K // 2), scales.reshape(cases.RANDOM_E, N, K // 32),
                        emul.decode_f64(codes, scales, "fp4").reshape(cases.RANDOM_E, N, K), bias)
    return _WEIGHTS[nk]


@pytest.mark.parametrize("index", range(len(cases.RANDOM_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.RANDOM_CASES[i]))
def test_every_pair_has_the_bits_of_the_decode_launches(index):
    _bit_rule(*cases.RANDOM_CASES[index], index)


@pytest.mark.parametrize("index", range(len(cases.WALK_RANDOM_WEIGHTS)), ids=lambda i: _name(cases.WALK_RANDOM_WEIGHTS[i]))
def test_every_pair_has_the_bits_of_the_decode_launches_at_the_models_k_and_on_a_wave_7_tail(index):
    """(17, 2880) and (C + 1, 992): the three forms against the decode launches bit for bit, and both inside the elementwise bounds
    against float64 without a factor (the GLU form: tests/moemlp_cases.py within_glu_bound over the f32 pre-activations)"""
    _bit_rule(cases.WALK_RANDOM_WEIGHTS[index], cases.WALK_RANDOM_PAIRS, "uniform", index, glu_bound=True)


def _bit_rule(nk, ta, routing, index, glu_bound=False):
    (N, K), (T, A), E = nk, ta, cases.RANDOM_E
    x_dtype = cases.X16[index % 2]
    w_codes, w_scales, wq, bias = _weights(nk)
    ids = cases.random_routing(ta, routing)
    flat = ids.reshape(-1)
    listed = torch.from_numpy((flat >= 0) & (flat < E))
    off = cases.OFFSETS[(index + 1) % len(cases.OFFSETS)]
    # the plain form, shared and per-slot rows, into f32 and into the row dtype
    for per_slot, out_dtype in ((False, torch.float32), (True, x_dtype)):
        x = cases.random_rows(nk, ta, x_dtype, per_slot)
        want = yard_experts(x, w_codes, w_scales, ids, bias, out_dtype)
        y = run_grouped("plain", x, w_codes, w_scales, ids, bias, out_dtype, FILLS[(index + per_slot) % 2], off)
        _assert_bits(y, want, f"{nk} {ta} {routing}, {'slot' if per_slot else 'shared'} -> {out_dtype}: every pair against mbnb_moe_mxfp4_experts")
        assert _is_plus_zero(y[~listed]) and int((~listed).sum()) >= 1
        if not per_slot:                                     # inside §25's elementwise bound against float64, without a factor
            rows = x.repeat_interleave(A, dim=0).double().numpy()
            r, bound = torch.zeros(T * A, N, dtype=torch.float64), torch.zeros(T * A, N, dtype=torch.float64)
            for e in range(E):
                sel = torch.from_numpy(flat == e)
                if bool(sel.any()):
                    r[sel], bound[sel] = _mx_bound(rows[sel.numpy()], wq[e], bias[e], out_dtype)
            none = torch.zeros(r.shape, dtype=torch.bool)
            ratio = elementwise._compare(y, r, bound, none, none, none, gn.last_launch(), "y = x . W[e]^T + b[e]")
            print(f"mx_grouped random {nk} {ta} {routing}, x {x_dtype}: worst err / bound = {ratio:.4f}")
    # the GLU form over the even rows below N
    n2 = N - N % 2
    x = cases.random_rows(nk, ta, x_dtype, False)
    gb = (bias * 4.0)[:, :n2].contiguous()                   # pre-activations on both sides of the limit
    for out_dtype in (torch.float32, x_dtype):
        want = yard_glu(x, w_codes[:, :n2], w_scales[:, :n2], ids, gb, out_dtype)
        h = run_grouped("glu", x, w_codes[:, :n2], w_scales[:, :n2], ids, gb, out_dtype, FILLS[index % 2], off)
        _assert_bits(h, want, f"{nk} {ta} {routing} -> {out_dtype}: the GLU form against mbnb_moemlp_gate_up_glu")
        assert _is_plus_zero(h[~listed])
        if glu_bound:
            pre = yard_experts(x, w_codes[:, :n2], w_scales[:, :n2], ids, gb, torch.float32).numpy()[listed.numpy()]
            assert (np.abs(pre) > LIMIT).any() and (np.abs(pre) < LIMIT).any()
            r = moemlp_cases.glu_f64(*moemlp_cases.split(pre), ALPHA, LIMIT)
            got = h[listed].double().numpy()
            ok, lo, hi = moemlp_cases.within_glu_bound(got, r, out_dtype)
            worst = float((np.abs(got - r) / moemlp_cases.glu_tol(r)).max())
            print(f"mx_grouped_glu random {nk} {ta} {routing}, x {x_dtype} -> {_name(out_dtype)}: worst |gpu - f64| / tol = {worst:.4f}"
                  + (" (the output's own rounding included)" if out_dtype != torch.float32 else ""))
            assert np.isfinite(got).all() and ok.all(), (nk, out_dtype, int((~ok).sum()), got[~ok][:4], lo[~ok][:4], hi[~ok][:4])
    # the down + sum form
    hrows = cases.random_rows(nk, ta, x_dtype, True)
    rw = torch.softmax(torch.randn(T, A, generator=torch.Generator().manual_seed(41300 + index)), dim=1).to(cases.DTYPES[index % 3])
    for out_dtype in (torch.float32, x_dtype):
        want = yard_down(hrows, w_codes, w_scales, ids, bias, rw, out_dtype)
        out = run_grouped("down", hrows, w_codes, w_scales, ids, bias, out_dtype, FILLS[(index + 1) % 2], off, rw=rw, ws_fill=FILLS[index % 2])
        _assert_bits(out, want, f"{nk} {ta} {routing} -> {out_dtype}: down + sum against mbnb_moemlp_down_sum")


# ----------------------------------------------------------------------------- 4. the edges of the semantics
def test_a_nan_scale_byte_makes_its_column_nan_for_the_pairs_of_its_expert_only():
    _nan_bytes(moe_cases.NAN_SHAPE, *moe_cases.nan_operands(), moe_cases.NAN_BLOCKS, moe_cases.NAN_BLOCKS[1])


def _nan_bytes(shape, x64, w64, ids, blocks, forms_block):
    """a 0xFF byte in each of `blocks` in turn (the plain form), and in `forms_block` for the GLU and the down + sum forms"""
    E, N, K, T, A = shape
    w_codes, w_scales = cases.quantize_experts(w64)
    clean = _round_once(moe_cases.reference_f64(x64, w64, None, ids), torch.float32)
    hit = torch.zeros(T * A, N, dtype=torch.bool)
    hit[torch.from_numpy(ids.reshape(-1) == moe_cases.NAN_EXPERT), moe_cases.NAN_COLUMN] = True
    assert 0 < int(hit.sum()) < T * A
    for i, b in enumerate(blocks):
        planted = w_scales.copy()
        planted[moe_cases.NAN_EXPERT, moe_cases.NAN_COLUMN, b] = 255
        for zero_x in (False, True):
            xb = x64.copy()
            if zero_x:
                xb[:, 32 * b:32 * b + 32] = 0.0
            want = _round_once(moe_cases.reference_f64(xb, w64, None, ids), torch.float32)
            y = run_grouped("plain", cases.to_dtype(xb, cases.X16[i % 2]), w_codes, planted, ids, None, torch.float32, FILLS[(i + zero_x) % 2])
            assert bool(torch.isnan(y[hit]).all()), (b, zero_x)
            _assert_bits(y[~hit], want[~hit], f"0xFF in block {b}, x block zero: {zero_x}: every other element")
    # the GLU and the down + sum forms: the output of that row, the tokens routed to that expert
    planted = w_scales.copy()
    planted[moe_cases.NAN_EXPERT, moe_cases.NAN_COLUMN, forms_block] = 255
    x = cases.to_dtype(x64, torch.bfloat16)
    h = run_grouped("glu", x, w_codes[:, :8], planted[:, :8], ids, None, torch.float32, FILLS[0])
    assert torch.equal(torch.isnan(h), hit[:, :8].reshape(T * A, 4, 2).any(dim=2))     # NaN exactly where a row of the output met the byte
    hrows = cases.to_dtype(np.repeat(x64[:, None, :], A, axis=1), torch.bfloat16)
    out = run_grouped("down", hrows, w_codes, planted, ids, None, torch.float32, FILLS[1], rw=torch.ones(T, A))
    want = torch.zeros(T, N, dtype=torch.bool)
    want[torch.from_numpy((ids == moe_cases.NAN_EXPERT).any(axis=1)), moe_cases.NAN_COLUMN] = True
    assert torch.equal(torch.isnan(out), want)              # NaN for exactly the tokens that route a slot to the expert
    _assert_bits(out[~want], clean.reshape(T, A, N).sum(dim=1)[~want], "and every other element (exact sums of two)")


@pytest.mark.parametrize("x_dtype", cases.X16, ids=_name)
def test_inf_and_nan_in_a_token_row_touch_that_tokens_pairs_only(x_dtype):
    _bad_activations(moe_cases.NAN_SHAPE, *moe_cases.nan_operands(), moe_cases.X_BAD_KS, x_dtype)


@pytest.mark.parametrize("K", cases.WALK_NONFINITE_KS)
def test_nan_bytes_inf_and_nan_on_a_ragged_last_step_off_wave_0(K):
    """The 0xFF byte on the first block of the last step and on block KB - 1 (all three forms see one of the two), the Inf and the NaN
    at the first k of that step and at k = K - 1: the step runs on wave 7 (K = 992), on wave 6 in its third pass (K = 2880)"""
    E, N, _, T, A = moe_cases.NAN_SHAPE
    i = cases.WALK_NONFINITE_KS.index(K)
    x64, w64, ids = moe_cases.walk_nan_operands(K)
    _nan_bytes((E, N, K, T, A), x64, w64, ids, moe_cases.walk_nan_blocks(K), moe_cases.walk_nan_blocks(K)[i % 2])
    _bad_activations((E, N, K, T, A), x64, w64, ids, moe_cases.walk_bad_ks(K), cases.X16[i % 2])


def _bad_activations(shape, x64, w64, ids, ks, x_dtype):
    E, N, K, T, A = shape
    w_codes, w_scales = cases.quantize_experts(w64)
    clean = _round_once(moe_cases.reference_f64(x64, w64, None, ids), torch.float32).reshape(T, A, N)
    other = torch.tensor([t != moe_cases.X_BAD_TOKEN for t in range(T)])
    n = 0
    for ki, k in enumerate(ks):
        for vi, v in enumerate(moe_cases.X_BAD_VALUES):
            xb = x64.copy()
            xb[moe_cases.X_BAD_TOKEN, k] = v
            want = moe_cases.reference_f64(xb, w64, None, ids).reshape(T, A, N)[moe_cases.X_BAD_TOKEN]   # elementwise IEEE: Inf * 0 = NaN
            y = run_grouped("plain", cases.to_dtype(xb, x_dtype), w_codes, w_scales, ids, None, torch.float32, FILLS[(ki + vi) % 2]).reshape(T, A, N)
            got = y[moe_cases.X_BAD_TOKEN].double().numpy()
            assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (k, v, got, want)
            _assert_bits(y[other], clean[other], f"{v} at k = {k}: the other tokens")
            n += int(np.isinf(want).any())
    assert n > 0


@pytest.mark.parametrize("index", range(len(moe_cases.WIDE_CASES)), ids=lambda i: "-".join(_name(v) for v in moe_cases.WIDE_CASES[i]))
def test_scale_bytes_from_end_to_end_bit_for_bit(index):
    which, out_dtype = moe_cases.WIDE_CASES[index]
    x64, w64, w_codes, w_scales, ids, _, _ = moe_cases.wide_operands(which)
    assert set(np.unique(w_scales[1]).tolist()) >= (set(range(0, 5)) if which == "low" else set(range(250, 255)))
    want = _round_once(moe_cases.reference_f64(x64, w64, None, ids), out_dtype)
    for fill in FILLS:
        y = run_grouped("plain", cases.to_dtype(x64, torch.bfloat16), w_codes, w_scales, ids, None, out_dtype, fill, cases.OFFSETS[1 + index % 3])
        _assert_bits(y, want, f"wide {which}, fill {fill:#x}")
    assert bool(torch.isfinite(y).all()) and bool((y != 0).all())


def test_ids_outside_the_experts_give_rows_of_plus_zero_and_leave_every_other_pair_alone():
    E, N, K, T, A = moe_cases.IDS_SHAPE
    x64, w64, bias64, ids = moe_cases.ids_operands()
    w_codes, w_scales = cases.quantize_experts(w64)
    x = cases.to_dtype(x64, torch.bfloat16)
    planted = ids.copy()
    for (t, a), v in zip(moe_cases.OUT_OF_RANGE_PLACES, moe_cases.OUT_OF_RANGE):
        planted[t, a] = np.int64(v).astype(np.int32)
    gone = torch.from_numpy(((planted < 0) | (planted >= E)).reshape(-1))
    for od in cases.DTYPES:
        bias = cases.to_dtype(bias64, od)
        base = run_grouped("plain", x, w_codes, w_scales, ids, bias, od, FILLS[0])
        _assert_bits(base, _round_once(moe_cases.reference_f64(x64, w64, bias64, ids), od), "in-range ids")
        for fill in FILLS:
            y = run_grouped("plain", x, w_codes, w_scales, planted, bias, od, fill, cases.OFFSETS[2])
            assert _is_plus_zero(y[gone]) and int(gone.sum()) == 4
            _assert_bits(y[~gone], base[~gone], "the pairs whose id stayed")
            h = run_grouped("glu", x, w_codes[:, :16], w_scales[:, :16], planted, bias[:, :16].contiguous(), od, fill, cases.OFFSETS[3])
            assert _is_plus_zero(h[gone]) and not _is_plus_zero(h[~gone])
        for v in moe_cases.OUT_OF_RANGE:                     # every id outside: no tile, rows of +0.0 from the workgroups that leave
            every = np.full((T, A), np.int64(v).astype(np.int32), dtype=np.int32)
            for form, cols in (("plain", N), ("glu", 16)):
                y = run_grouped(form, x, w_codes[:, :cols], w_scales[:, :cols], every, None, od, FILLS[0])
                assert _is_plus_zero(y), (v, od, form)
            hrows = cases.to_dtype(np.repeat(x64[:, None, :], A, axis=1), torch.bfloat16)
            nan_rw = torch.full((T, A), float("nan"))
            for ws_fill in FILLS:                            # neither the routing weight nor the workspace row of a skipped pair is read
                assert _is_plus_zero(run_grouped("down", hrows, w_codes, w_scales, every, None, od, FILLS[1], rw=nan_rw, ws_fill=ws_fill)), (v, od)


# ----------------------------------------------------------------------------- 4b. past one column tile; many experts
@pytest.mark.parametrize("index", range(len(cases.TILE_CASES)), ids=lambda i: "{}-N{}".format(*cases.TILE_CASES[i]))
def test_glu_and_down_past_one_column_tile_against_float64_and_the_decode_launches(index):
    """N on either side of the column tile and past two of them, counts on the row-tile edges, the four ids outside [0, E) among
    them; the real alpha and limit.  GLU: the bits of mbnb_moemlp_gate_up_glu, inside within_glu_bound of the float64 chain over the
    exact pre-activations, and rows of +0.0 across every column tile for the pairs outside.  Down + sum: the bits of float64 through
    routed_sum_f32 (exact) and of mbnb_moemlp_down_sum, under both fills of the output and of the workspace"""
    form, N = cases.TILE_CASES[index]
    E, x_dtype = cases.TILE_E, cases.X16[index % 2]
    rows64, w64, bias64, ids, rw64 = cases.tile_operands(form, N)
    w_codes, w_scales = cases.quantize_experts(w64)
    rows, bias, rw = cases.to_dtype(rows64, x_dtype), cases.to_dtype(bias64, cases.DTYPES[index % 3]), cases.to_dtype(rw64, cases.DTYPES[(index + 1) % 3])
    assert (bias.double().numpy() == bias64).all() and (rw.double().numpy() == rw64).all()
    flat = ids.reshape(-1)
    gone = torch.from_numpy((flat < 0) | (flat >= E))
    assert int(gone.sum()) == 4
    off = cases.OFFSETS[index % len(cases.OFFSETS)]
    for out_dtype in (torch.float32, x_dtype):
        if form == "glu":
            pre = cases.reference("plain", rows64, w_codes, w_scales, ids, bias64).astype(np.float32)[~gone.numpy()]       # exact in f32
            r = moemlp_cases.glu_f64(*moemlp_cases.split(pre), ALPHA, LIMIT)
            want = yard_glu(rows, w_codes, w_scales, ids, bias, out_dtype)
            for fill in FILLS:
                h = run_grouped("glu", rows, w_codes, w_scales, ids, bias, out_dtype, fill, off)
                _assert_bits(h, want, f"glu N = {N} -> {out_dtype}, fill {fill:#x}: against mbnb_moemlp_gate_up_glu")
                assert _is_plus_zero(h[gone]) and h.shape[1] == N // 2
                got = h[~gone].double().numpy()
                ok, lo, hi = moemlp_cases.within_glu_bound(got, r, out_dtype)
                assert np.isfinite(got).all() and ok.all(), (N, out_dtype, int((~ok).sum()), got[~ok][:4], lo[~ok][:4], hi[~ok][:4])
        else:
            want = _round_once(cases.reference("down", rows64, w_codes, w_scales, ids, bias64, rw=rw64).astype(np.float64), out_dtype)
            _assert_bits(yard_down(rows, w_codes, w_scales, ids, bias, rw, out_dtype), want, f"down N = {N}: mbnb_moemlp_down_sum against float64")
            for fill in FILLS:
                for ws_fill in FILLS:
                    out = run_grouped("down", rows, w_codes, w_scales, ids, bias, out_dtype, fill, off, rw=rw, ws_fill=ws_fill)
                    _assert_bits(out, want, f"down N = {N} -> {out_dtype}, fill {fill:#x}, workspace {ws_fill:#x}")


@pytest.mark.parametrize("form,N", cases.TILE_ALL_OUTSIDE, ids=lambda v: str(v))
def test_every_id_outside_gives_plus_zero_across_every_column_tile_under_both_fills(form, N):
    """No tile: every output element is written by the workgroups that leave, a column tile each; one that nobody wrote would keep
    the fill under one of the two.  Down + sum: neither the routing weight nor the workspace row of a skipped pair is read"""
    rows64, w64, bias64, ids, _ = cases.tile_operands("glu" if form == "glu" else "down", N)
    w_codes, w_scales = cases.quantize_experts(w64)
    rows, bias = cases.to_dtype(rows64, torch.bfloat16), cases.to_dtype(bias64, torch.float32)
    nan_rw = torch.full(ids.shape, float("nan"))
    for i, v in enumerate(moe_cases.OUT_OF_RANGE):
        every = np.full(ids.shape, np.int64(cases.TILE_E if v == moe_cases.IDS_SHAPE[0] else v).astype(np.int32), dtype=np.int32)
        od = cases.DTYPES[i % 3]
        for fill in FILLS:
            for ws_fill in (FILLS if form == "down" else (None,)):
                y = run_grouped(form, rows, w_codes, w_scales, every, bias, od, fill, cases.OFFSETS[i], rw=nan_rw, ws_fill=ws_fill)
                assert _is_plus_zero(y) and y.shape[1] == (N // 2 if form == "glu" else N), (form, N, v, od, fill, ws_fill)


@pytest.mark.parametrize("form", ("plain", "glu", "down"))
@pytest.mark.parametrize("index", range(len(cases.MANY_CASES)), ids=lambda i: f"E{cases.MANY_CASES[i][0]}")
def test_many_experts_bit_for_bit(index, form):
    """E = 128 past one column tile and E = MAX_EXPERTS, sparse counts that include the lowest and the highest expert: float64
    rounded once (the GLU form at alpha = 0, where its chain is exact)"""
    case = cases.MANY_CASES[index]
    rows64, w64, bias64, ids, rw64 = cases.many_operands(case, index, form)
    w_codes, w_scales = cases.quantize_experts(w64)
    x_dtype, out_dtype = cases.X16[index % 2], cases.DTYPES[(index + len(form)) % 3]
    rw = cases.to_dtype(rw64, torch.float32)
    want = _round_once(np.asarray(cases.reference(form, rows64, w_codes, w_scales, ids, bias64, 0.0, LIMIT, rw64), dtype=np.float64), out_dtype)
    for fill in FILLS:
        y = run_grouped(form, cases.to_dtype(rows64, x_dtype), w_codes, w_scales, ids, cases.to_dtype(bias64, torch.float32), out_dtype, fill,
                        cases.OFFSETS[(index + 1) % len(cases.OFFSETS)], alpha=0.0, limit=LIMIT, rw=rw)
        _assert_bits(y, want, f"{form} {case[:5]}, fill {fill:#x}")


# ----------------------------------------------------------------------------- 5. the Python surface
def _surface(T=37, A=3, E=5, N=18, K=160, dtype=torch.bfloat16, seed=43000):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(dtype)
    h = torch.randn(T, A, K, generator=g).to(dtype)
    w = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8)
    s = torch.randint(120, 131, (E, N, K // 32), generator=g, dtype=torch.uint8)
    bias = torch.randn(E, N, generator=g)
    ids = torch.from_numpy(np.random.default_rng(seed).integers(-1, E, size=(T, A)).astype(np.int32))
    rw = torch.softmax(torch.randn(T, A, generator=g), dim=1)
    return tuple(t.to(DEV) for t in (x, h, w, s, bias, ids, rw))


def test_the_three_functions_id_dtypes_views_the_blocks_layout_a_side_stream_and_a_shared_plan():
    x, h, w, s, bias, ids, rw = _surface()
    T, A = ids.shape
    with torch.no_grad():
        want = (bnb.matmul_mxfp4_experts(x, w, s, ids, bias), bnb.matmul_mxfp4_experts(h, w, s, ids, bias, dtype=torch.float32),
                bnb.matmul_mxfp4_experts_glu(x, w, s, ids, bias), bnb.matmul_mxfp4_experts_sum(h, w, s, ids, rw, bias))
        assert moen.last_launch() == moe_cases.launch_text(x.dtype, True, 5, T * A) and mlpn.last_launch() == moemlp_cases.down_text(x.dtype, 5, T * A, A)

        def all_four(xx, hh, ww, ii, rr, plan=None):
            return (bnb.matmul_mxfp4_experts_grouped(xx, ww, s, ii, bias, plan=plan), bnb.matmul_mxfp4_experts_grouped(hh, ww, s, ii, bias, torch.float32, plan=plan),
                    bnb.matmul_mxfp4_experts_grouped_glu(xx, ww, s, ii, bias, plan=plan), bnb.matmul_mxfp4_experts_grouped_sum(hh, ww, s, ii, rr, bias, plan=plan))

        def same(got, what):
            for g_, w_, form in zip(got, want, ("shared", "slot", "glu", "sum")):
                _assert_bits(g_.cpu(), w_.cpu(), f"{what}: {form}")

        same(all_four(x, h, w, ids, rw), "the grouped functions against the decode functions")
        assert gn.last_launch() == cases.down_text(x.dtype, 5, T * A, A)
        same(all_four(x, h, w, ids.long(), rw.double()), "int64 ids, f64 routing weights")
        same(all_four(x, h, w.reshape(5, 18, 5, 16), ids, rw), "the blocks layout")
        wide_x = torch.zeros(T, 320, dtype=x.dtype, device=DEV)[:, ::2]
        wide_x.copy_(x)
        wide_h = torch.zeros(T, A, 320, dtype=x.dtype, device=DEV)[:, :, ::2]
        wide_h.copy_(h)
        wide_ids = torch.zeros(A, T, dtype=torch.int32, device=DEV).t()
        wide_ids.copy_(ids)
        wide_rw = torch.zeros(A, T, device=DEV).t()
        wide_rw.copy_(rw)
        assert not wide_x.is_contiguous() and not wide_h.is_contiguous() and not wide_ids.is_contiguous() and not wide_rw.is_contiguous()
        same(all_four(wide_x, wide_h, w, wide_ids, wide_rw), "strided views")
        i32, plan = bnb.moe_grouped_plan(ids.long(), 5)
        assert i32.dtype == torch.int32 and len(plan) == 1 and plan[0].numel() == gn.plan_bytes(T * A, 5)
        assert bnb.moe_grouped_plan(ids, 5)[0] is ids
        same(all_four(x, h, w, i32, rw, plan), "one plan shared by the four calls")
        for bad in ([], plan + plan, [plan[0][:-256]], [plan[0].cpu()], plan[0]):
            with pytest.raises(ValueError, match="moe_grouped_plan"):
                bnb.matmul_mxfp4_experts_grouped(x, w, s, ids, bias, plan=bad)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            side = all_four(x, h, w, ids, rw)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        same(side, "a side stream")
        assert tuple(bnb.matmul_mxfp4_experts_grouped(x[:0], w, s, ids[:0]).shape) == (0, A, 18)
        assert tuple(bnb.matmul_mxfp4_experts_grouped_glu(x[:0], w, s, ids[:0]).shape) == (0, A, 9)
        empty = bnb.matmul_mxfp4_experts_grouped_sum(h[:0], w, s, ids[:0], rw[:0])
        assert tuple(empty.shape) == (0, 18) and empty.dtype == x.dtype


def test_more_pairs_than_one_call_are_cut_over_the_tokens(monkeypatch):
    A = cases.CUT_A
    E, N, K = cases.CUT_SHAPE_TAIL
    T = F.MOE_GROUPED_MAX_PAIRS // A + 1                     # MOE_GROUPED_MAX_PAIRS + A pairs
    g = torch.Generator().manual_seed(43100)
    x = (torch.randn(T, K, generator=g) * 0.25).to(torch.float16).to(DEV)
    h = (torch.randn(T, A, K, generator=g) * 0.25).to(torch.float16).to(DEV)
    w = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8).to(DEV)
    s = torch.full((E, N, K // 32), 126, dtype=torch.uint8, device=DEV)
    bias = torch.randn(E, N, generator=g).to(DEV)
    ids = torch.from_numpy(np.random.default_rng(43101).integers(-1, E, size=(T, A)).astype(np.int32)).to(DEV)
    rw = torch.rand(T, A, generator=g).to(DEV)
    step = T - 1
    with torch.no_grad():
        i32, plan = bnb.moe_grouped_plan(ids, E)
        assert len(plan) == 2 and plan[1].numel() == gn.plan_bytes(A, E)
        for f, inp, tail in ((bnb.matmul_mxfp4_experts_grouped, x, ()), (bnb.matmul_mxfp4_experts_grouped_glu, x, ()),
                             (bnb.matmul_mxfp4_experts_grouped_sum, h, (rw,))):
            cut = lambda t, lo, hi: tuple(v[lo:hi] for v in t)
            out = f(inp, w, s, ids, *tail, bias)
            assert f" P{A} " in gn.last_launch() + " "        # the last call served the one token left over
            _assert_bits(out[:step].cpu(), f(inp[:step], w, s, ids[:step], *cut(tail, 0, step), bias).cpu(), f"{f.__name__}: the first call's tokens")
            _assert_bits(out[step:].cpu(), f(inp[step:], w, s, ids[step:], *cut(tail, step, T), bias).cpu(), f"{f.__name__}: the rest")
            _assert_bits(out.cpu(), f(inp, w, s, i32, *tail, bias, plan=plan).cpu(), f"{f.__name__}: the shared plans of both cuts")
        # against the decode route, which cuts the same call into 17 launches
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
        _assert_bits(bnb.matmul_mxfp4_experts_grouped_glu(x, w, s, ids, bias).cpu(), bnb.matmul_mxfp4_experts_glu(x, w, s, ids, bias).cpu(), "glu")
        assert gn.last_launch() == cases.glu_text(x.dtype, E, A) and mlpn.last_launch() == moemlp_cases.glu_text(x.dtype, E, A)


def _route_block(dtype=torch.bfloat16):
    T, A, E, H, I = cases.ROUTE_SHAPE
    g = torch.Generator().manual_seed(43200)
    block = bnb.MoEBlockMXFP4(E, H, I, top_k=A, compute_dtype=dtype, device=DEV)
    ex = block.experts
    ex.gate_up_proj_blocks.copy_(torch.randint(0, 256, tuple(ex.gate_up_proj_blocks.shape), generator=g, dtype=torch.uint8))
    ex.down_proj_blocks.copy_(torch.randint(0, 256, tuple(ex.down_proj_blocks.shape), generator=g, dtype=torch.uint8))
    ex.gate_up_proj_bias.copy_(torch.randn(E, 2 * I, generator=g))
    ex.down_proj_bias.copy_(torch.randn(E, H, generator=g))
    block.router.weight.copy_(torch.randn(E, H, generator=g))
    return block, [(torch.randn(T, H, generator=g) * 0.25).to(dtype).to(DEV) for _ in range(3)], [torch.randn(E, H, generator=g).to(dtype).to(DEV) for _ in range(3)]


def test_the_automatic_route_at_the_threshold_has_the_bits_of_the_decode_route(monkeypatch):
    T, A, E, H, I = cases.ROUTE_SHAPE
    block, xs, _ = _route_block()
    x = xs[0]
    ex = block.experts
    args = (ex.gate_up_proj_blocks, ex.gate_up_proj_scales, ex.gate_up_proj_bias, ex.down_proj_blocks, ex.down_proj_scales, ex.down_proj_bias)
    with torch.no_grad():
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
        ids, rw = block.router(x)
        want_mlp, want_block = bnb.moe_mlp_mxfp4(x, *args, ids, rw).cpu(), block(x).cpu()
        want_plain = bnb.matmul_mxfp4_experts(x, args[0], args[1], ids, args[2], dtype=torch.float32).cpu()
        assert mlpn.last_launch() == moemlp_cases.down_text(x.dtype, E, (T % (mlpn.MAX_PAIRS // A)) * A, A)
        # one pair below the threshold the old libraries still serve the call, with their launch texts
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", T * A + 1)
        before = gn.last_launch()
        _assert_bits(bnb.moe_mlp_mxfp4(x, *args, ids, rw).cpu(), want_mlp, "below the threshold")
        assert gn.last_launch() == before and mlpn.last_launch() == moemlp_cases.down_text(x.dtype, E, (T % (mlpn.MAX_PAIRS // A)) * A, A)
        bnb.matmul_mxfp4_experts(x[:300], args[0], args[1], ids[:300], args[2])
        assert moen.last_launch() == moe_cases.launch_text(x.dtype, False, E, (300 - 256) * A) and gn.last_launch() == before
        # at the threshold the grouped library serves it, with the same bits
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", T * A)
        _assert_bits(bnb.moe_mlp_mxfp4(x, *args, ids, rw).cpu(), want_mlp, "moe_mlp_mxfp4 at the threshold")
        assert gn.last_launch() == cases.down_text(x.dtype, E, T * A, A)
        _assert_bits(block(x).cpu(), want_block, "MoEBlockMXFP4 at the threshold")
        _assert_bits(bnb.moe_mlp_mxfp4(x, *args, ids.long(), rw).cpu(), want_mlp, "int64 ids")
        _assert_bits(bnb.matmul_mxfp4_experts(x, args[0], args[1], ids, args[2], dtype=torch.float32).cpu(), want_plain, "matmul_mxfp4_experts")
        assert gn.last_launch() == cases.experts_text(x.dtype, False, E, T * A)
        h = bnb.matmul_mxfp4_experts_glu(x, args[0], args[1], ids, args[2])
        assert gn.last_launch() == cases.glu_text(x.dtype, E, T * A)
        _assert_bits(bnb.matmul_mxfp4_experts_sum(h, args[3], args[4], ids, rw, args[5]).cpu(), want_mlp, "the two halves")


def test_a_captured_graph_of_the_block_on_the_grouped_route(monkeypatch):
    T, A, E, H, I = cases.ROUTE_SHAPE
    block, xs, rws = _route_block()
    with torch.no_grad():
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
        wants = []
        for xv, rv in zip(xs, rws):
            block.router.weight.copy_(rv)
            out, (ids, _) = block(xv, return_routing=True)
            wants.append((out.cpu(), ids.cpu()))
        assert not torch.equal(wants[0][1], wants[1][1]) and not torch.equal(wants[0][0], wants[2][0])
        monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", T * A)
        X = xs[0].clone()
        block.router.weight.copy_(rws[0])
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            block(X)                                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):        # a single chain: the router, the plan, the two projections, the sum
            out, (ids, _) = block(X, return_routing=True)
        assert gn.last_launch() == cases.down_text(X.dtype, E, T * A, A)
        for (want, want_ids), xv, rv in list(zip(wants, xs, rws))[::-1]:
            X.copy_(xv)
            block.router.weight.copy_(rv)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(ids.cpu(), want_ids)
            _assert_bits(out.cpu(), want, "a replay after the input and the router weight, and so the ids, changed in place")
