"""
functional.matmul_4bit_lora_grouped, nn.Linear4bitLoRA and nn.Linear4bitLoRAGroup on the GPU.

Every fused case (tests/lora_cases.py) runs on guarded allocations (tests/guard.py) under both fills -- the f32 workspace `t` is one of
them, so a t element read before it is written shows -- and must lie within the fused bound of tests/lora_bound.py per element around
a float64 evaluation with the CPU oracle's decoded weight, show exactly the expected calls in the binding's launch log and the
library's report, and equal matmul_4bit BIT FOR BIT on every member without an adapter.  tests/test_lora_host.py holds that each case
fails the bound if the adapter term is dropped.  The composed cases must show no fused launch, raise nothing and lie within the
composed bound.  Operands are made once per shape and shared.

Each case prints its worst err / bound ratio.  Measured on an MI355X: fused 0.44 at most (bf16, K = 1024, R = 3; f16 0.13), 0.04 and
less from K = 4096 up; composed 0.016.
"""
import functools

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _lora_native as ln
from mps_bitsandbytes_amd import functional as F
from tests import lora_cases as lc
from tests import nonfinite
from tests.guard import FILLS, guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.lora_bound import assert_lora_elementwise
from tests.test_gpu_elementwise import _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = lc.DT


@functools.lru_cache(maxsize=None)
def _member(N, K, dt, qt="nf4", nested=False, seed=0):
    """(packed, QuantState) on the GPU, and the oracle's decoded weight [N, K] on the GPU too (for the float64 reference)."""
    op, oa, ost2, Wd = lc.member(N, K, dt, qt, nested, 64, seed)
    st2 = None
    if nested:
        st2 = F.QuantState(absmax=ost2[0].to(DEV), shape=torch.Size([oa.numel()]), blocksize=ost2[1], quant_type="int8", dtype=torch.float32)
    st = F.QuantState(absmax=oa.to(DEV), shape=torch.Size([N, K]), blocksize=64, quant_type=qt, dtype=DT[dt], state2=st2)
    return op.to(DEV), st, Wd.to(DEV)


@functools.lru_cache(maxsize=None)
def _x(K, dt, seed=7, rows=1):
    return lc.x(K, dt, seed, rows).to(DEV)


@functools.lru_cache(maxsize=None)
def _bias(N, dt, seed):
    return lc.bias(N, dt, seed).to(DEV)


@functools.lru_cache(maxsize=None)
def _adapter(N, K, R, dt, seed):
    ad = lc.adapter(N, K, R, dt, seed)
    return None if ad is None else (ad[0].to(DEV), ad[1].to(DEV), ad[2])


def _group(Ns, K, dt, Rs, qt="nf4", nested=False, bias=()):
    members = [_member(N, K, dt, qt, nested, seed=i) for i, N in enumerate(Ns)]
    weights = [(p, st) for p, st, _ in members]
    biases = [_bias(N, dt, i) if i in bias else None for i, N in enumerate(Ns)]
    adapters = [_adapter(N, K, R, dt, i) for i, (N, R) in enumerate(zip(Ns, Rs))]
    return weights, adapters, biases, [wd for _, _, wd in members]


def _check(ys, X, decoded, biases, adapters, T, path, kernel):
    worst = 0.0
    for y, wd, b, ad in zip(ys, decoded, biases, adapters):
        worst = max(worst, assert_lora_elementwise(y, X, wd, b, ad, T, path, kernel))
    return worst


# ----------------------------------------------------------------------------- the fused cases
@pytest.mark.parametrize("Ns, K, qt, nested, bias, Rs, dt", [p[1:] for p in lc.FUSED_PARAMS], ids=[p[0] for p in lc.FUSED_PARAMS])
def test_fused_cases_lie_within_the_bound_on_poisoned_buffers(guarded_alloc, Ns, K, qt, nested, bias, Rs, dt):
    T = DT[dt]
    weights, adapters, biases, decoded = _group(Ns, K, dt, Rs, qt, nested, bias)
    X = _x(K, dt)
    plain = {i: F.matmul_4bit(X, weights[i][0], weights[i][1], biases[i]) for i, R in enumerate(Rs) if R is None}
    form = lc.report(Rs, K)
    worst = 0.0
    for fill in FILLS:
        guarded_alloc.begin(fill, where=f"matmul_4bit_lora_grouped fill 0x{fill:02X}")
        ln.reset_launch_log()
        gn.reset_launch_log()
        ys = F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert len(guarded_alloc.allocs) == 2 and guarded_alloc.allocs[1].view.dtype == torch.float32      # the outputs, and t
        assert guarded_alloc.allocs[1].view.numel() == sum(r or 0 for r in Rs)
        assert ln.launch_log == [(n, total, K, T) for n, total in lc.chunks(Rs)], ln.launch_log
        assert gn.launch_log == []
        assert ln.last_launch() == form, ln.last_launch()
        assert isinstance(ys, tuple) and len(ys) == len(Ns)
        for i, y in enumerate(ys):
            assert y.shape == (1, Ns[i]) and y.dtype == T
            if Rs[i] is None:
                assert torch.equal(y, plain[i]), f"member {i} of {Ns} (no adapter) differs from matmul_4bit under fill 0x{fill:02X}"
        worst = max(worst, _check(ys, X, decoded, biases, adapters, T, "fused", form))
    print(f"{form} {qt} {dt} N={Ns} R={Rs} K={K}: worst err / bound {worst:.3f}")


def test_two_calls_on_unchanged_inputs_give_equal_bits():
    Ns, K, dt, Rs = (5, 1, 130), 2112, "bf16", (16, None, 65)
    weights, adapters, biases, _ = _group(Ns, K, dt, Rs, bias=(1,))
    first = F.matmul_4bit_lora_grouped(_x(K, dt), weights, adapters, biases)
    ln.reset_launch_log()
    second = F.matmul_4bit_lora_grouped(_x(K, dt), weights, adapters, biases)
    assert ln.launch_log == [(3, 81, K, DT[dt])]
    for a, b in zip(first, second):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


# ----------------------------------------------------------------------------- what runs in the composed form
def _composed_case(name):
    """(A, weights, adapters, biases, decoded, dtype name) of a call the fused launches do not serve."""
    dt, K, Ns, Rs = "bf16", 1024, (4, 6), (3, 8)
    weights, adapters, biases, decoded = _group(Ns, K, dt, Rs, bias=(1,))
    A = _x(K, dt)
    if name == "M=2":
        A = _x(K, dt, 9, 2)
    elif name == "R=257":
        adapters = [adapters[0], _adapter(6, K, 257, dt, 1)]
    elif name == "f32 adapter":
        adapters = [adapters[0], (adapters[1][0].float(), adapters[1][1].float(), adapters[1][2])]
    else:
        assert name == "lora_B strided"
        wide = torch.zeros(6, 16, dtype=DT[dt], device=DEV)
        wide[:, ::2] = adapters[1][1]
        adapters = [adapters[0], (adapters[1][0], wide[:, ::2], adapters[1][2])]
        assert not adapters[1][1].is_contiguous()
    return A, weights, adapters, biases, decoded, dt


@pytest.mark.parametrize("name", ["M=2", "R=257", "f32 adapter", "lora_B strided"])
def test_everything_else_runs_the_composed_form(name):
    A, weights, adapters, biases, decoded, dt = _composed_case(name)
    ln.reset_launch_log()
    gn.reset_launch_log()
    ys = F.matmul_4bit_lora_grouped(A, weights, adapters, biases)
    assert ln.launch_log == [] and gn.launch_log == [], f"{name}: a fused launch"
    assert len(ys) == 2 and all(y.dtype == DT[dt] and y.shape == (A.shape[0], N) for y, N in zip(ys, (4, 6)))
    worst = _check(ys, A, decoded, biases, adapters, DT[dt], "composed", name)
    print(f"composed {name}: worst err / bound {worst:.3f}")


def test_a_wanted_gradient_runs_the_composed_form_and_matches_the_explicit_expression():
    dt, K, Ns, Rs = "bf16", 1024, (4, 6), (3, 8)
    T = DT[dt]
    weights, adapters, biases, decoded = _group(Ns, K, dt, Rs, bias=(1,))
    seeds = [lc.x(N, dt, 300 + i).to(DEV) for i, N in enumerate(Ns)]

    def leaves():
        A = _x(K, dt).clone().requires_grad_(True)
        ads = [(a.clone().requires_grad_(True), b.clone().requires_grad_(True), s) for a, b, s in adapters]
        return A, ads

    A, ads = leaves()
    ln.reset_launch_log()
    ys = F.matmul_4bit_lora_grouped(A, weights, ads, biases)
    assert ln.launch_log == [] and all(y.requires_grad for y in ys)
    _check([y.detach() for y in ys], A.detach(), decoded, biases, adapters, T, "composed", "gradient")
    torch.autograd.backward(ys, seeds)

    A2, ads2 = leaves()
    ref = []
    for (p, st), b, (la, lb, s) in zip(weights, biases, ads2):
        y = A2 @ F.dequantize_4bit(p, st).t()
        if b is not None:
            y = y + b
        ref.append(y + ((A2 @ la.t()) @ lb.t()) * s)
    torch.autograd.backward(ref, seeds)
    for y, r in zip(ys, ref):
        torch.testing.assert_close(y.detach(), r.detach())
    torch.testing.assert_close(A.grad, A2.grad)
    for (la, lb, _), (la2, lb2, _) in zip(ads, ads2):
        torch.testing.assert_close(la.grad, la2.grad)
        torch.testing.assert_close(lb.grad, lb2.grad)
    # a gradient wanted on an adapter alone is enough
    ln.reset_launch_log()
    ys = F.matmul_4bit_lora_grouped(_x(K, dt), weights, [ads[0], adapters[1]], biases)
    assert ln.launch_log == [] and [y.requires_grad for y in ys] == [True, False]


# ----------------------------------------------------------------------------- the forms of A
@pytest.mark.parametrize("form", ["[K]", "[1, 1, K]", "strided", "other dtype"])
def test_input_forms(form):
    Ns, K, dt, Rs = (5, 1, 130), 2112, "bf16", (16, None, 65)
    weights, adapters, biases, decoded = _group(Ns, K, dt, Rs, bias=(1,))
    X = _x(K, dt)
    if form == "[K]":
        A, lead = X.reshape(K), ()
    elif form == "[1, 1, K]":
        A, lead = X.reshape(1, 1, K), (1, 1)
    elif form == "strided":
        wide = torch.zeros(1, 2 * K, dtype=X.dtype, device=DEV)
        wide[:, ::2] = X
        A, lead = wide[:, ::2], (1,)
        assert not A.is_contiguous()
    else:
        A, lead = X.float(), (1,)          # the weight dtype is asked for explicitly below
    cd = torch.bfloat16 if form == "other dtype" else None
    want = F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
    ln.reset_launch_log()
    ys = F.matmul_4bit_lora_grouped(A, weights, adapters, biases, cd)
    assert ln.launch_log == [(3, 81, K, torch.bfloat16)]
    for y, r, N in zip(ys, want, Ns):
        assert y.shape == lead + (N,) and y.dtype == torch.bfloat16
        assert torch.equal(y.reshape(1, N), r)      # the same row through the same two launches: the same bits
    _check(ys, X, decoded, biases, adapters, torch.bfloat16, "fused", form)


# ----------------------------------------------------------------------------- the modules
def _lora_layer(N, K, dt, seed, r, bias):
    p, st, wd = _member(N, K, dt, seed=seed)
    base = bnb.Linear4bit(K, N, bias=bias, device=DEV, compute_dtype=DT[dt])
    base._set_quantized(p, st)
    layer = bnb.Linear4bitLoRA(base, r=r, lora_alpha=4.0)
    ad = _adapter(N, K, r, dt, seed)
    with torch.no_grad():
        layer.lora_A.copy_(ad[0])
        layer.lora_B.copy_(ad[1])
        if bias:
            base.bias.copy_(_bias(N, dt, seed))
    assert layer.scaling == ad[2]
    return layer, wd


def test_both_modules():
    K, dt = 1024, "bf16"
    T = DT[dt]
    built = [_lora_layer(N, K, dt, i, r, bias=i != 1) for i, (N, r) in enumerate(((8, 4), (4, 16), (6, 1)))]
    layers, decoded = [b[0] for b in built], [b[1] for b in built]
    group = bnb.Linear4bitLoRAGroup(layers)
    biases = [layer.base.bias for layer in layers]
    adapters = [(layer.lora_A.detach(), layer.lora_B.detach(), layer.scaling) for layer in layers]
    for shape in ((1, K), (K,), (1, 1, K), (3, K), (2, 3, K)):
        rows = 1
        for d in shape[:-1]:
            rows *= d
        x = lc.x(K, dt, 410 + len(shape), rows).to(DEV).reshape(shape)
        with torch.no_grad():
            ln.reset_launch_log()
            got = group(x)
            assert ln.launch_log == ([(3, 21, K, T)] if rows == 1 else []), (shape, ln.launch_log)
            ln.reset_launch_log()
            alone = layers[1](x)
            assert ln.launch_log == ([(1, 16, K, T)] if rows == 1 else []), (shape, ln.launch_log)
        assert isinstance(got, tuple) and len(got) == 3
        for y, layer in zip(got, layers):
            assert y.shape == ((1,) if len(shape) == 1 else shape[:-1]) + (layer.out_features,) and y.dtype == T      # as Linear4bit: [K] -> [1, N]
        assert alone.shape == got[1].shape
        path = "fused" if rows == 1 else "composed"
        _check([g.detach() for g in got], x.reshape(-1, K), decoded, [None if b is None else b.detach() for b in biases], adapters, T, path,
               f"group {shape}")
        _check([alone], x.reshape(-1, K), decoded[1:2], [None], adapters[1:2], T, path, f"layer {shape}")
        if rows == 1:
            assert torch.equal(alone, got[1])      # a row of a group of one is the row of a group of three
    # with gradients on (the adapters are parameters) the composed form runs and stays differentiable
    x = _x(K, dt)
    ln.reset_launch_log()
    got = group(x)
    assert ln.launch_log == [] and all(y.requires_grad for y in got)
    sum(y.float().sum() for y in got).backward()
    assert all(layer.lora_A.grad is not None and layer.lora_B.grad is not None for layer in layers)


# ----------------------------------------------------------------------------- graph capture
def test_two_fused_calls_captured_in_one_graph_replay_with_new_inputs():
    K, dt = 2112, "bf16"
    T = DT[dt]
    w1, a1, b1, _ = _group((5, 1, 130), K, dt, (16, None, 65), bias=(1,))
    w2, a2, b2, _ = _group((7, 9), K, dt, (2, 70), qt="fp4")
    A = _x(K, dt).clone()
    inputs = [lc.x(K, dt, 500 + i).to(DEV) for i in range(2)]
    eager = []
    for xin in inputs:
        eager.append(tuple(y.clone() for y in F.matmul_4bit_lora_grouped(xin, w1, a1, b1) + F.matmul_4bit_lora_grouped(xin, w2, a2, b2)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.matmul_4bit_lora_grouped(A, w1, a1, b1)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    ln.reset_launch_log()
    with torch.cuda.graph(graph, stream=stream):
        outs = F.matmul_4bit_lora_grouped(A, w1, a1, b1) + F.matmul_4bit_lora_grouped(A, w2, a2, b2)
    assert ln.launch_log == [(3, 81, K, T), (2, 72, K, T)]
    for xin, want in zip(inputs, eager):
        A.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        for y, r in zip(outs, want):
            assert torch.equal(y, r)


# ----------------------------------------------------------------------------- non-finite activations
@pytest.mark.parametrize("Ns, K, bias, Rs, dt", [((4,), 1088, (), (3,), "bf16"),                        # a partial (and the only) 2048-chunk
                                                 ((5, 1, 130), 2112, (1,), (16, None, 65), "f16")],     # the second chunk partial; two slices of B
                         ids=["K1088", "K2112"])
def test_nonfinite_activations_land_where_ieee_arithmetic_puts_them(guarded_alloc, Ns, K, bias, Rs, dt):
    """An Inf of either sign at every special place of the row (tests/nonfinite.py), one call each (k_lora_down + k_gemv4_group_lora): a
    member without an adapter keeps matmul_4bit's bits on the same planted input; a member with one has every element in the class
    (NaN, +Inf, -Inf, finite) of an explicit float64 IEEE evaluation of x . Wd^T + b + s (B . (A . x))."""
    T = DT[dt]
    weights, adapters, biases, decoded = _group(Ns, K, dt, Rs, bias=bias)
    for one in nonfinite.passes(1, K):
        X = nonfinite.planted(_x(K, dt), one)
        guarded_alloc.begin(FILLS[0], where=f"matmul_4bit_lora_grouped, X{one}")
        plain = {i: F.matmul_4bit(X, weights[i][0], weights[i][1], biases[i]) for i, R in enumerate(Rs) if R is None}
        ln.reset_launch_log()
        ys = F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert ln.launch_log == [(n, total, K, T) for n, total in lc.chunks(Rs)], ln.launch_log
        for i, (y, wd, b, ad) in enumerate(zip(ys, decoded, biases, adapters)):
            if ad is None:
                assert _same_bits(y, plain[i]), f"member {i} of {Ns} (no adapter) differs from matmul_4bit with X{one}"
            nonfinite.assert_classes(y, nonfinite.adapter_classes(X, wd, b, ad), f"gemv_lora member {i} of {Ns}, X{one}")
