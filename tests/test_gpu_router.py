"""The mixture-of-experts router (k_router) through the C ABI with every output on a guard-banded, offset buffer under
two fills, and through the Python surface with the block it completes.  The tables and the numpy restatement are
tests/router_cases.py (closed on the CPU by tests/test_router_host.py).

  1  exact logits at every edge: bit-equal to float64 rounded once; ids bit-equal to the restatement
  2  ties: the lower index wins, at every token position                3  random data at the user's shape, the gap fixture
  4  every token alone, in another batch, with and without logits_out   5  non-finite rows, weights and biases
  6  rw_dtype, views, a side stream                                      7  the block and a captured graph"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, _router_native as rn
from mps_bitsandbytes_amd._native import ptr, stream_ptr
from tests import guard, router_cases as cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILLS = guard.FILLS
F32 = np.float32
CODE = _native.DTYPE_CODE


def _name(v):
    return str(v).replace("torch.", "").replace(" ", "")[:40]


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    g, w = _bits(got), _bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {got[i].item()!r} (bits {int(g[i]):#x}), "
                             f"want {want[i].item()!r} (bits {int(w[i]):#x})")


def _canon(t):
    """every NaN on one bit pattern: which NaN an operation gives is the only thing numpy and the device may differ in"""
    t = t.clone()
    t[torch.isnan(t)] = float("nan")
    return t


def _placed(name, t, fill, offset_bytes):
    g = guard._carve(name, tuple(t.shape), t.dtype, DEV, fill, offset_bytes)
    g.view.copy_(t)
    return g


def run_router(x, W, bias, A, fill=FILLS[0], rw_dtype=torch.float32, logits=True, offsets=None):
    """mbnb_router_topk_softmax through the C ABI, every operand carved inside guard bands at its offset
    -> (ids int32 [T, A], rw [T, A], logits f32 [T, E] or None) on the CPU"""
    off = dict(cases.OFFSETS[0], **(offsets or {}))
    T, K = x.shape
    E = W.shape[0]
    xg = _placed("x", x.contiguous(), fill, off["x"])
    wg = _placed("w", W.contiguous(), fill, off["w"])
    bg = None if bias is None else _placed("bias", bias, fill, off["bias"] * _esize(bias.dtype))
    ids = guard._carve("ids", (T, A), torch.int32, DEV, fill, 4 * off["ids"])
    rw = guard._carve("rw", (T, A), rw_dtype, DEV, fill, off["rw"] * _esize(rw_dtype))
    lg = guard._carve("logits_out", (T, E), torch.float32, DEV, fill, 4 * off["logits"]) if logits else None
    st = rn.lib().mbnb_router_topk_softmax(ptr(xg.view), T, K, CODE[x.dtype], ptr(wg.view), E, None if bg is None else ptr(bg.view),
                                           0 if bg is None else CODE[bias.dtype], A, ptr(ids.view), ptr(rw.view), CODE[rw_dtype],
                                           None if lg is None else ptr(lg.view), stream_ptr(DEV))
    rn.check(st, "topk_softmax")
    torch.cuda.synchronize()
    for g in (ids, rw, xg, wg) + (() if bg is None else (bg,)) + (() if lg is None else (lg,)):
        assert g.violation() is None, (g.name, g.violation(), (E, K, T, A, x.dtype, rw_dtype, fill, off))
    assert rn.last_launch() == cases.launch_text(x.dtype, E, K, A, T), rn.last_launch()
    return ids.view.cpu().clone(), rw.view.cpu().clone(), None if lg is None else lg.view.cpu().clone()


def _check_against_stored_logits(ids, rw, logits, A, what, exact=False):
    """the selection and the weights are functions of the stored logits: ids bit-equal to the restatement over them, rw bit-equal
    where the chain is exact, else inside the weight bound of the float64 chain (NaN exactly where that is NaN)"""
    l = logits.numpy()
    want_ids, want_rw = cases.emulate(l, A)
    assert np.array_equal(ids.numpy(), want_ids), (what, np.argwhere(ids.numpy() != want_ids)[:4])
    if exact:
        _assert_bits(_canon(rw), _canon(torch.from_numpy(want_rw)), what + ": weights")
        return 0.0
    _, r = cases.emulate64(l, A)
    got = rw.double().numpy()
    ok = cases.within_weight_bound(got, r, A)
    with np.errstate(all="ignore"):
        ratio = np.abs(got - r) / cases.weight_tol(r, A)
    worst = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else 0.0
    print(f"{what}: worst |w - f64| / bound = {worst:.4f}")
    assert ok.all(), (what, int((~ok).sum()), got[~ok][:4], r[~ok][:4])
    return worst


# ----------------------------------------------------------------------------- 1. exact logits at every edge
@pytest.mark.parametrize("index", range(len(cases.LOGIT_CASES)), ids=lambda i: "-".join(_name(v) for v in cases.LOGIT_CASES[i]))
def test_logits_on_lossless_operands_bit_for_bit(index):
    case = cases.LOGIT_CASES[index]
    E, K, T, A, dtype, bias_dtype = case
    x64, W64, b64 = cases.logit_operands(case, index)
    x, W = cases.to_dtype(x64, dtype), cases.to_dtype(W64, dtype)
    bias = None if b64 is None else cases.to_dtype(b64, bias_dtype)
    want = torch.from_numpy(cases.logits_f64(x64, W64, b64)).to(torch.float32)               # exact in f32: one rounding, of nothing
    want_ids, _ = cases.emulate(want.numpy(), A)
    outs = []
    for fill in FILLS:                                       # an element the launch never wrote holds the fill: it cannot match under both
        ids, rw, logits = run_router(x, W, bias, A, fill, offsets=cases.OFFSETS[index % len(cases.OFFSETS)])
        _assert_bits(logits, want, f"logits {case[:4]}, fill {fill:#x}")
        assert np.array_equal(ids.numpy(), want_ids), (case[:4], fill)
        _check_against_stored_logits(ids, rw, logits, A, f"{case[:4]} fill {fill:#x}")
        outs.append((ids, rw))
    assert torch.equal(outs[0][0], outs[1][0])
    _assert_bits(outs[0][1], outs[1][1], "the same weights under the other fill")


# ----------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("name", cases.PLANTED)
def test_ties_go_to_the_lower_index_at_every_token_position(name):
    b, A, exact = cases.planted(name)
    E, T, K = b.size, 3, 16
    x = cases.to_dtype(cases.lossless(T, K, 46000), torch.bfloat16)
    W = torch.zeros(E, K, dtype=torch.bfloat16)              # the logit is the f32 bias, bit for bit (a -0 bias gives +0)
    want_l = torch.from_numpy(np.repeat((F32(0) + b)[None, :], T, axis=0))
    for fill in FILLS:
        ids, rw, logits = run_router(x, W, torch.from_numpy(b), A, fill, offsets=cases.OFFSETS[1])
        _assert_bits(logits, want_l, name)
        _check_against_stored_logits(ids, rw, logits, A, name, exact=exact)
        v = b[ids.numpy().astype(np.int64)]
        for t in range(T):
            assert (np.diff(v[t]) <= 0).all()
            assert all(ids[t, i] < ids[t, i + 1] for i in range(A - 1) if v[t, i] == v[t, i + 1]), (name, t, ids[t])


def test_ties_between_equal_weight_rows():
    """equal rows of W give equal logits, whichever wave and pass sums them: the order of a sum is fixed by K alone"""
    T, K, E, A = 5, 520, 200, 8
    g = torch.Generator().manual_seed(46100)
    x = torch.randn(T, K, generator=g).to(torch.float16)
    W = (torch.randn(E, K, generator=g) * 0.01).to(torch.float16)
    W[:] = W[:10].repeat(20, 1)                              # expert e equals e % 10: twenty-fold ties, 4, 16 and 64 apart among them
    ids, rw, logits = run_router(x, W, None, A, FILLS[0])
    _assert_bits(logits, logits[:, :10].repeat(1, 20), "equal rows, equal logits")
    _check_against_stored_logits(ids, rw, logits, A, "equal rows")
    best = logits[:, :10].argmax(dim=1)
    assert torch.equal(ids, (best[:, None] + 10 * torch.arange(A)[None, :]).to(torch.int32))      # the best row's copies, ascending


# ----------------------------------------------------------------------------- 3. random data, the gap fixture
@pytest.mark.parametrize("dtype", cases.X16, ids=_name)
@pytest.mark.parametrize("shape", cases.RANDOM_SHAPES, ids=_name)
def test_random_data_at_the_users_shape(shape, dtype):
    T, K, E, A = shape
    x, W, bias = cases.random_operands(shape, dtype)
    ids, rw, logits = run_router(x, W, bias, A, FILLS[0], offsets=cases.OFFSETS[2])
    xd, Wd, bd = x.double().numpy(), W.double().numpy(), bias.double().numpy()
    err = np.abs(logits.double().numpy() - cases.logits_f64(xd, Wd, bd))
    tol = cases.logit_tol(xd, Wd, bd)
    print(f"random {shape} {_name(dtype)}: worst |logit - f64| / bound = {(err / tol).max():.4f}")
    assert (err <= tol).all()
    _check_against_stored_logits(ids, rw, logits, A, f"random {shape} {_name(dtype)}")
    assert abs(rw.double().sum(dim=1) - 1).max() < 1e-5
    ids2, rw2, logits2 = run_router(x, W, bias, A, FILLS[1], offsets=cases.OFFSETS[3])
    assert torch.equal(ids, ids2)
    _assert_bits(rw2, rw, "the other fill")
    _assert_bits(logits2, logits, "the other fill")


@pytest.mark.parametrize("seed", cases.GAP_SEEDS)
def test_the_gap_fixture_routes_as_float64_does(seed):
    T, K, E, A = cases.GAP_SHAPE
    x, W, bias = cases.gap_operands(seed)
    want, ok = cases.gap_margins(x, W, bias, A)
    assert ok.all()
    ids, rw, logits = run_router(x, W, bias, A, FILLS[seed % 2])
    assert np.array_equal(ids.numpy(), want), np.argwhere(ids.numpy() != want)[:4]
    _check_against_stored_logits(ids, rw, logits, A, f"gap fixture {seed}")


# ----------------------------------------------------------------------------- 4. independence
def test_every_token_alone_in_another_batch_and_without_logits_out():
    T, K, E, A = cases.RANDOM_SHAPES[0]
    x, W, bias = cases.random_operands(cases.RANDOM_SHAPES[0], torch.bfloat16)
    ids, rw, logits = run_router(x, W, bias, A, FILLS[0])
    ids_n, rw_n, none = run_router(x, W, bias, A, FILLS[1], logits=False)
    assert none is None and torch.equal(ids_n, ids)
    _assert_bits(rw_n, rw, "without logits_out")
    for t in range(T):
        i1, r1, l1 = run_router(x[t:t + 1], W, bias, A, FILLS[t % 2], logits=bool(t % 3))
        assert torch.equal(i1, ids[t:t + 1]), t
        _assert_bits(r1, rw[t:t + 1], f"token {t} alone")
        if l1 is not None:
            _assert_bits(l1, logits[t:t + 1], f"token {t} alone")
    # another size and order: five of the tokens, reversed, among rows of another draw
    pick = [16, 11, 7, 3, 0]
    other = torch.randn(9, K, generator=torch.Generator().manual_seed(46200)).to(torch.bfloat16)
    place = [8, 1, 4, 6, 2]
    other[place] = x[pick]
    i2, r2, l2 = run_router(other, W, bias, A, FILLS[0], offsets=cases.OFFSETS[1])
    assert torch.equal(i2[place], ids[pick])
    _assert_bits(r2[place], rw[pick], "inside another batch")
    _assert_bits(l2[place], logits[pick], "inside another batch")


# ----------------------------------------------------------------------------- 5. non-finite values
def _bad_operands():
    T, K, E, A = cases.BAD_SHAPE
    g = torch.Generator().manual_seed(46300)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(E, K, generator=g) * 0.1).to(torch.bfloat16)
    W[W == 0] = 0.125                                        # no zero weight: an Inf in x never meets one (that is a NaN, not an Inf)
    bias = torch.randn(E, generator=g).float()
    return x, W, bias


def test_a_nan_or_inf_in_a_tokens_row_stays_within_that_token():
    T, K, E, A = cases.BAD_SHAPE
    x, W, bias = _bad_operands()
    ids, rw, logits = run_router(x, W, bias, A, FILLS[0])
    assert bool(torch.isfinite(logits).all())
    others = torch.tensor([t != cases.BAD_TOKEN for t in range(T)])
    for ki, k in enumerate(cases.BAD_K):
        for vi, v in enumerate(cases.BAD_VALUES):
            xb = x.clone()
            xb[cases.BAD_TOKEN, k] = v
            i2, r2, l2 = run_router(xb, W, bias, A, FILLS[(ki + vi) % 2])
            assert torch.equal(i2[others], ids[others]), (k, v)
            _assert_bits(r2[others], rw[others], f"{v} at k = {k}: the other tokens' weights")
            _assert_bits(l2[others], logits[others], f"{v} at k = {k}: the other tokens' logits")
            row = l2[cases.BAD_TOKEN]
            if v != v:
                assert bool(torch.isnan(row).all())
            else:                                            # +-Inf times a nonzero weight: an Inf of the product's sign
                sign = torch.sign(W[:, k].float()) * (1.0 if v > 0 else -1.0)
                assert torch.equal(row, sign * float("inf")), (k, v)
            _check_against_stored_logits(i2, r2, l2, A, f"{v} at k = {k}")                   # NaN exactly where the float64 chain is NaN
            assert bool(torch.isnan(r2[cases.BAD_TOKEN]).all())                               # a NaN logit, or two +Inf among the selected


def test_a_nan_in_a_weight_row_ranks_its_expert_first_for_every_token():
    T, K, E, A = cases.BAD_SHAPE
    x, W, bias = _bad_operands()
    for k in cases.BAD_K:
        Wb = W.clone()
        Wb[cases.BAD_EXPERT, k] = float("nan")
        ids, rw, logits = run_router(x, Wb, bias, A, FILLS[k % 2])
        assert bool((ids[:, 0] == cases.BAD_EXPERT).all()) and bool(torch.isnan(rw).all())
        assert bool(torch.isnan(logits[:, cases.BAD_EXPERT]).all()) and int(torch.isnan(logits).sum()) == T
        clean = cases.select(np.delete(logits.numpy(), cases.BAD_EXPERT, axis=1), A - 1)
        clean = clean + (clean >= cases.BAD_EXPERT)
        assert np.array_equal(ids[:, 1:].numpy(), clean)     # the others follow in their order


def test_infinite_biases():
    T, K, E, A = cases.BAD_SHAPE
    x, W, bias = _bad_operands()
    up = bias.clone()
    up[cases.BAD_EXPERT] = float("inf")
    ids, rw, logits = run_router(x, W, up, A, FILLS[0])
    assert bool((ids[:, 0] == cases.BAD_EXPERT).all()) and bool(torch.isnan(rw).all())       # Inf - Inf in slot 0
    _check_against_stored_logits(ids, rw, logits, A, "+Inf bias")
    down = bias.clone()
    down[cases.BAD_EXPERT] = -float("inf")
    ids, rw, logits = run_router(x, W, down, A, FILLS[1])
    assert not bool((ids == cases.BAD_EXPERT).any())
    _check_against_stored_logits(ids, rw, logits, A, "-Inf bias, not selected")
    ids, rw, logits = run_router(x, W, down, E, FILLS[0])    # A = E: it is selected last, with weight +0
    assert bool((ids[:, E - 1] == cases.BAD_EXPERT).all()) and bool((_bits(rw[:, E - 1]) == 0).all())
    _check_against_stored_logits(ids, rw, logits, E, "-Inf bias, selected last")


# ----------------------------------------------------------------------------- 6. rw_dtype, views, streams
def test_sixteen_bit_weights_are_one_rounding_of_the_f32_weights():
    for shape in cases.RANDOM_SHAPES:
        T, K, E, A = shape
        x, W, bias = cases.random_operands(shape, torch.float16)
        ids, rw, _ = run_router(x, W, bias, A, FILLS[0])
        for i, dtype in enumerate(cases.X16):
            ids16, rw16, _ = run_router(x, W, bias, A, FILLS[i], rw_dtype=dtype, offsets=cases.OFFSETS[1 + i])
            assert torch.equal(ids16, ids)
            _assert_bits(rw16, rw.to(dtype), f"rw as {dtype}")
    b, A, _ = cases.planted("boundary")
    x, W = torch.zeros(2, 8, dtype=torch.float16), torch.zeros(b.size, 8, dtype=torch.float16)
    _, rw, _ = run_router(x, W, torch.from_numpy(b), A, FILLS[1])
    for dtype in cases.X16:
        _, rw16, _ = run_router(x, W, torch.from_numpy(b), A, FILLS[0], rw_dtype=dtype)
        _assert_bits(rw16, rw.to(dtype), f"rw as {dtype}, planted")


def test_the_function_views_a_side_stream_and_the_device_context():
    shape = cases.RANDOM_SHAPES[1]
    T, K, E, A = shape
    x, W, bias = cases.random_operands(shape, torch.bfloat16)
    ids, rw, logits = run_router(x, W, bias, A, FILLS[0])
    xd, Wd, bd = x.to(DEV), W.to(DEV), bias.to(DEV)
    with torch.no_grad():
        got = bnb.moe_router_topk(xd, Wd, bd)
        assert len(got) == 2 and got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and tuple(got[0].shape) == (T, A)
        assert rn.last_launch() == cases.launch_text(torch.bfloat16, E, K, A, T)
        assert torch.equal(got[0].cpu(), ids)
        _assert_bits(got[1].cpu(), rw, "the function")
        i3, r3, l3 = bnb.moe_router_topk(xd.reshape(1, T, K), Wd, bd.double(), top_k=A, return_logits=True)
        assert torch.equal(i3.cpu(), ids) and tuple(l3.shape) == (T, E)
        _assert_bits(r3.cpu(), rw, "a 3-D input, a float64 bias read as f32")
        _assert_bits(l3.cpu(), logits, "return_logits")
        for dtype in cases.X16:
            _assert_bits(bnb.moe_router_topk(xd, Wd, bd, weights_dtype=dtype)[1].cpu(), rw.to(dtype), f"weights_dtype {dtype}")
        wide_x = torch.zeros(T, 2 * K, dtype=x.dtype, device=DEV)[:, ::2]
        wide_x.copy_(xd)
        wide_w = torch.zeros(K, E, dtype=x.dtype, device=DEV).t()
        wide_w.copy_(Wd)
        off_b = torch.zeros(E + 1, dtype=bias.dtype, device=DEV)[1:]
        off_b.copy_(bd)
        assert not wide_x.is_contiguous() and not wide_w.is_contiguous() and off_b.data_ptr() % 4 == 2
        iv, rv = bnb.moe_router_topk(wide_x, wide_w, off_b)
        assert torch.equal(iv.cpu(), ids)
        _assert_bits(rv.cpu(), rw, "strided views and an offset bias")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            i_s, r_s = bnb.moe_router_topk(xd, Wd, bd)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        assert torch.equal(i_s.cpu(), ids)
        _assert_bits(r_s.cpu(), rw, "a side stream")
        if torch.cuda.device_count() > 1:                    # operands on a device that is not the current one
            far = torch.device("cuda:1")
            i_f, r_f = bnb.moe_router_topk(xd.to(far), Wd.to(far), bd.to(far))
            assert i_f.device == far and torch.equal(i_f.cpu(), ids)
            _assert_bits(r_f.cpu(), rw, "another device")
        empty = bnb.moe_router_topk(xd[:0], Wd, bd, return_logits=True)
        assert [tuple(t.shape) for t in empty] == [(0, A), (0, A), (0, E)]
        layer = bnb.MoERouterTopK(K, E, top_k=A, device=DEV)
        layer.load_state_dict({"weight": W, "bias": bias})
        i_m, r_m = layer(xd)
        assert torch.equal(i_m.cpu(), ids)
        _assert_bits(r_m.cpu(), rw, "the module")


# ----------------------------------------------------------------------------- 7. the block
def _block(E, H, I, A, T, dtype=torch.bfloat16, seed=47000):
    g = torch.Generator().manual_seed(seed + 10 * A + T)
    gate, up = torch.randn(E, I, H, generator=g) * 0.1, torch.randn(E, I, H, generator=g) * 0.1
    down = torch.randn(E, H, I, generator=g) * 0.1
    gb, ub, db = torch.randn(E, I, generator=g), torch.randn(E, I, generator=g), torch.randn(E, H, generator=g)
    linear = torch.nn.Linear(H, E)
    with torch.no_grad():
        linear.weight.copy_(torch.randn(E, H, generator=g) * 0.3)
        linear.bias.copy_(torch.randn(E, generator=g))
    experts = bnb.MoEMLPMXFP4.from_weights(gate.to(DEV), up.to(DEV), down.to(DEV), gb, ub, db, compute_dtype=dtype)
    router = bnb.MoERouterTopK.from_linear(linear, A, device=DEV, dtype=dtype)
    sd = {"mlp.router." + k: v for k, v in router.state_dict().items()}
    sd.update({"mlp.experts." + k: v for k, v in experts.state_dict().items()})
    block = bnb.MoEBlockMXFP4(E, H, I, top_k=A, device=DEV, compute_dtype=dtype)
    block.load_state_dict({k[len("mlp."):]: v for k, v in sd.items()}, strict=True)
    x = torch.randn(T, H, generator=g).to(dtype).to(DEV)
    return block, router, experts, x


@pytest.mark.parametrize("shape", cases.BLOCK_SHAPES, ids=_name)
def test_the_block_is_the_expert_mlp_on_the_routers_ids_and_weights(shape):
    E, H, I, A, T = shape
    block, router, experts, x = _block(*shape)
    with torch.no_grad():
        ids, rw = bnb.moe_router_topk(x, router.weight, router.bias, top_k=A)
        want = experts(x, ids, rw)
        out, (ids_b, rw_b) = block(x, return_routing=True)
        assert out.dtype == x.dtype and tuple(out.shape) == (T, H) and torch.equal(ids_b, ids)
        _assert_bits(rw_b.cpu(), rw.cpu(), "the block's routing weights")
        _assert_bits(out.cpu(), want.cpu(), "the block against the expert MLP on the router's outputs")
        _assert_bits(block(x).cpu(), want.cpu(), "without return_routing")
        e = block.experts
        fn = bnb.moe_block_mxfp4(x, block.router.weight, block.router.bias, e.gate_up_proj_blocks, e.gate_up_proj_scales, e.gate_up_proj_bias,
                                 e.down_proj_blocks, e.down_proj_scales, e.down_proj_bias, top_k=A)
        _assert_bits(fn.cpu(), want.cpu(), "the function")
        _assert_bits(block(x.reshape(1, T, H)).cpu(), want.cpu().reshape(1, T, H), "leading dimensions")


def test_a_captured_graph_replayed_after_the_input_and_the_router_weight_change_in_place():
    E, H, I, A, T = 8, 64, 64, 2, 5
    block, router, experts, x = _block(E, H, I, A, T)
    g = torch.Generator().manual_seed(47100)
    x2 = torch.randn(T, H, generator=g).to(x.dtype).to(DEV)
    w2 = (torch.randn(E, H, generator=g) * 0.3).to(x.dtype).to(DEV)
    with torch.no_grad():
        want1 = block(x).cpu()
        want2, (ids2, _) = block(x2, return_routing=True)
        ids1 = block(x, return_routing=True)[1][0]
        assert not torch.equal(ids1, ids2)                   # the new rows route differently
        torch.cuda.synchronize()
        X = x.clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            block(X)                                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):         # a single chain of four kernels
            out = block(X)
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits(out.cpu(), want1, "the first replay")
        X.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits(out.cpu(), want2.cpu(), "a replay after x changed in place")
        block.router.weight.copy_(w2)
        want3, (ids3, _) = block(x2, return_routing=True)
        assert not torch.equal(ids3, ids2)
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits(out.cpu(), want3.cpu(), "a replay after router.weight changed in place")
