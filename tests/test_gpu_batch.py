"""
functional.matmul_4bit_grouped, functional.matmul_4bit_lora_grouped and the three modules above them on 2 to 16 rows of input, on the GPU
(libmbnb_batch.so).

Every fused case (tests/batch_cases.py) runs on guarded allocations (tests/guard.py) under both fills -- the f32 workspace `t` is one of
them, so a t element read before it is written shows -- and must show exactly the expected calls in the binding's launch log and the
library's report.  A grouped case must equal matmul_4bit on the same member BIT FOR BIT (k_skinny4_group's body is a copy of
k_skinny4's: this is what holds the two together) and lie within the elementwise bound of tests/elementwise.py around a float64
product with the CPU oracle's decoded weight.  An adapter case must lie within the fused bound of tests/lora_bound.py per element and
equal matmul_4bit bit for bit on every member without an adapter; tests/test_batch_host.py holds that each such case fails the bound
in every row if the epilogue is dropped.  The cases that decline must show no new launch, raise nothing and keep matmul_4bit's bits
(the composed bound where they carry adapters).  Operands are made once per shape and shared.

Each case prints its worst err / bound ratio.  Measured on an MI355X: grouped 0.91 at most (bf16, K = 256: the rounding to bf16 itself;
f16 0.74 at K = 128), 0.05 at K = 16384; with adapters 0.85 at most (bf16, K = 256, R = 2), 0.04 and less at R = (63, 256); composed 0.014.
"""
import functools

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _batch_native as bn
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _lora_native as ln
from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F
from tests import batch_cases as bc
from tests import lora_cases as lc
from tests import nonfinite
from tests.elementwise import assert_linear_elementwise
from tests.guard import FILLS, guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.lora_bound import assert_lora_elementwise
from tests.test_gpu_elementwise import _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = bc.DT


@functools.lru_cache(maxsize=None)
def _member(N, K, dt, qt="nf4", nested=False, bs=64, seed=0):
    """(packed, QuantState) on the GPU, and the oracle's decoded weight [N, K] on the GPU too (for the float64 references)."""
    op, oa, ost2, Wd = lc.member(N, K, dt, qt, nested, bs, seed)
    st2 = None
    if nested:
        st2 = F.QuantState(absmax=ost2[0].to(DEV), shape=torch.Size([oa.numel()]), blocksize=ost2[1], quant_type="int8", dtype=torch.float32)
    st = F.QuantState(absmax=oa.to(DEV), shape=torch.Size([N, K]), blocksize=bs, quant_type=qt, dtype=DT[dt], state2=st2)
    return op.to(DEV), st, Wd.to(DEV)


@functools.lru_cache(maxsize=None)
def _x(K, dt, M, seed=7):
    return bc.x(K, dt, M, seed).to(DEV)


@functools.lru_cache(maxsize=None)
def _bias(N, dt, seed):
    return lc.bias(N, dt, seed).to(DEV)


@functools.lru_cache(maxsize=None)
def _adapter(N, K, R, dt, seed):
    ad = lc.adapter(N, K, R, dt, seed)
    return None if ad is None else (ad[0].to(DEV), ad[1].to(DEV), ad[2])


def _group(Ns, K, dt, qt="nf4", nested=False, bs=64, bias=(), Rs=None):
    members = [_member(N, K, dt, qt, nested, bs, seed=i) for i, N in enumerate(Ns)]
    weights = [(p, st) for p, st, _ in members]
    biases = [_bias(N, dt, i) if i in bias else None for i, N in enumerate(Ns)]
    adapters = None if Rs is None else [_adapter(N, K, R, dt, i) for i, (N, R) in enumerate(zip(Ns, Rs))]
    return weights, biases, [wd for _, _, wd in members], adapters


def _by_member(A, weights, biases, cd=None, variant="skinny MT1 NR1"):
    """matmul_4bit per member: what a grouped call promises bit for bit; its kernel form is the one the fused workgroup copies."""
    refs = []
    for (p, st), b in zip(weights, biases):
        refs.append(F.matmul_4bit(A, p, st, b, cd))
        if variant is not None:
            assert _native.last_variant() == variant, _native.last_variant()
    return refs


def _reset():
    bn.reset_launch_log()
    gn.reset_launch_log()
    ln.reset_launch_log()


# ----------------------------------------------------------------------------- the grouped cases
@pytest.mark.parametrize("Ns, K, qt, nested, bs, bias, Rs, dt, M", bc.ARGS, ids=bc.IDS)
def test_fused_group_equals_matmul_4bit_bit_for_bit(guarded_alloc, Ns, K, qt, nested, bs, bias, Rs, dt, M):
    T = DT[dt]
    weights, biases, decoded, _ = _group(Ns, K, dt, qt, nested, bs, bias)
    X = _x(K, dt, M)
    guarded_alloc.begin(FILLS[0], where="reference")
    refs = _by_member(X, weights, biases)
    guarded_alloc.check()
    form = bc.grouped_report(len(Ns), M)
    for fill in FILLS:
        guarded_alloc.begin(fill, where=f"matmul_4bit_grouped M={M} fill 0x{fill:02X}")
        _reset()
        ys = F.matmul_4bit_grouped(X, weights, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert len(guarded_alloc.allocs) == 1 and guarded_alloc.allocs[0].view.numel() == M * sum(Ns)      # ONE allocation: the outputs
        assert bn.launch_log == [(n, M, K, T) for n in bc.chunks(len(Ns))], bn.launch_log
        assert gn.launch_log == [] and ln.launch_log == []
        assert bn.last_launch() == form, bn.last_launch()
        assert isinstance(ys, tuple) and len(ys) == len(Ns)
        for i, (y, r) in enumerate(zip(ys, refs)):
            assert y.shape == r.shape == (M, Ns[i]) and y.dtype == r.dtype == T and y.is_contiguous()
            assert torch.equal(y, r), f"member {i} of {Ns} differs from matmul_4bit under fill 0x{fill:02X}"
    worst = 0.0
    for y, wd, b in zip(ys, decoded, biases):
        worst = max(worst, assert_linear_elementwise(y, X, wd, b, T, T, form))
    print(f"{form} {qt} {dt} bs={bs} N={Ns[:4]} K={K}: worst err / bound {worst:.3f}")


# ----------------------------------------------------------------------------- what declines
def _declined_case(name):
    """(A, weights, biases) of a call on 2 rows (17 for "M=17") that no fused launch serves."""
    dt, K, Ns = "bf16", 1024, (4, 6)
    if name in ("K=192", "K=16512"):
        K = int(name[2:])
    weights, biases, _, _ = _group(Ns, K, dt, bias=(1,))
    A = _x(K, dt, 17 if name == "M=17" else 2, seed=9)
    if name == "plain with nested":
        weights = [weights[0], _member(6, K, dt, nested=True, seed=1)[:2]]
    elif name == "packed+1":
        p, st = weights[1]
        buf = torch.empty(p.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = p.reshape(-1)
        weights = [weights[0], (buf[1:].view(p.shape), st)]
        assert weights[1][0].data_ptr() % 16 == 1 and weights[1][0].is_contiguous()
    elif name == "gradient":
        A = A.clone().requires_grad_(True)
    return A, weights, biases


DECLINED = ["M=17", "K=192", "K=16512", "plain with nested", "packed+1", "gradient"]


@pytest.mark.parametrize("name", DECLINED)
def test_what_declines_runs_member_by_member_with_matmul_4bits_bits(name):
    A, weights, biases = _declined_case(name)
    refs = _by_member(A.detach(), weights, biases, variant=None)
    before = bn.last_launch()
    _reset()
    ys = F.matmul_4bit_grouped(A, weights, biases)
    assert bn.launch_log == [] and gn.launch_log == [] and bn.last_launch() == before, f"{name}: a fused launch"
    assert len(ys) == len(refs)
    for y, r in zip(ys, refs):
        assert y.shape == r.shape and y.dtype == r.dtype and torch.equal(y.detach(), r)
    if name not in ("M=17", "gradient"):      # these reached the library, and it said why
        assert bn.last_error().startswith("mbnb_batch_gemm4: ")


# ----------------------------------------------------------------------------- the adapter cases
def _check_lora(ys, X, decoded, biases, adapters, T, path, kernel):
    worst = 0.0
    for y, wd, b, ad in zip(ys, decoded, biases, adapters):
        worst = max(worst, assert_lora_elementwise(y, X, wd, b, ad, T, path, kernel))
    return worst


@pytest.mark.parametrize("Ns, K, qt, nested, bs, bias, Rs, dt, M", bc.ARGS, ids=bc.IDS)
def test_fused_adapter_cases_lie_within_the_bound_on_poisoned_buffers(guarded_alloc, Ns, K, qt, nested, bs, bias, Rs, dt, M):
    T = DT[dt]
    weights, biases, decoded, adapters = _group(Ns, K, dt, qt, nested, bs, bias, Rs)
    X = _x(K, dt, M)
    plain = {i: F.matmul_4bit(X, weights[i][0], weights[i][1], biases[i]) for i, R in enumerate(Rs) if R is None}
    form = bc.lora_report(Rs, K, M)
    worst, seen = 0.0, []
    for fill in FILLS:
        guarded_alloc.begin(fill, where=f"matmul_4bit_lora_grouped M={M} fill 0x{fill:02X}")
        _reset()
        ys = F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert len(guarded_alloc.allocs) == 2 and guarded_alloc.allocs[1].view.dtype == torch.float32      # the outputs, and t
        assert guarded_alloc.allocs[0].view.numel() == M * sum(Ns) and guarded_alloc.allocs[1].view.numel() == M * sum(r or 0 for r in Rs)
        assert bn.launch_log == [(n, total, M, K, T) for n, total in lc.chunks(Rs)], bn.launch_log
        assert gn.launch_log == [] and ln.launch_log == []
        assert bn.last_launch() == form, bn.last_launch()
        assert isinstance(ys, tuple) and len(ys) == len(Ns)
        for i, y in enumerate(ys):
            assert y.shape == (M, Ns[i]) and y.dtype == T
            if Rs[i] is None:
                assert torch.equal(y, plain[i]), f"member {i} of {Ns} (no adapter) differs from matmul_4bit under fill 0x{fill:02X}"
        worst = max(worst, _check_lora(ys, X, decoded, biases, adapters, T, "fused", form))
        # t holds the down-projections: every element written (no fill pattern survives in both runs) and finite
        assert bool(torch.isfinite(guarded_alloc.allocs[1].view).all())
        seen.append([y.clone() for y in ys])
    for a, b in zip(*seen):      # a second call, on other buffers with another fill: equal bits
        assert torch.equal(a, b)
    print(f"{form} {qt} {dt} bs={bs} N={Ns[:4]} R={Rs[:4]} K={K}: worst err / bound {worst:.3f}")


def test_rows_do_not_leak_into_each_other():
    """Row m of a call equals the same row in a call whose other rows hold different data, with and without adapters."""
    Ns, K, dt, Rs, M = (5, 1, 130), 2176, "bf16", (16, None, 65), 5
    weights, biases, _, adapters = _group(Ns, K, dt, bias=(1,), Rs=Rs)
    X = _x(K, dt, M)
    other = _x(K, dt, M, seed=31)
    base = F.matmul_4bit_lora_grouped(X, weights, adapters, biases), F.matmul_4bit_grouped(X, weights, biases)
    for m in range(M):
        mixed = other.clone()
        mixed[m] = X[m]
        _reset()
        got = F.matmul_4bit_lora_grouped(mixed, weights, adapters, biases), F.matmul_4bit_grouped(mixed, weights, biases)
        assert bn.launch_log == [(3, 81, M, K, DT[dt]), (3, M, K, DT[dt])]
        for want_group, got_group in zip(base, got):
            for w, y in zip(want_group, got_group):
                assert torch.equal(w[m], y[m]), f"row {m} depends on the other rows"
    # and a batch of 2 holding rows 0 and 1 gives those rows of the batch of 5 (the summation order does not depend on M)
    for w, y in zip(base[0], F.matmul_4bit_lora_grouped(X[:2], weights, adapters, biases)):
        assert torch.equal(w[:2], y)


def _composed_case(name):
    dt, K, Ns, Rs = "bf16", 1024, (4, 6), (3, 8)
    weights, biases, decoded, adapters = _group(Ns, K, dt, bias=(1,), Rs=Rs)
    if name == "R=257":
        adapters = [adapters[0], _adapter(6, K, 257, dt, 1)]
    elif name == "f32 adapter":
        adapters = [adapters[0], (adapters[1][0].float(), adapters[1][1].float(), adapters[1][2])]
    else:
        assert name == "lora_B strided"
        wide = torch.zeros(6, 16, dtype=DT[dt], device=DEV)
        wide[:, ::2] = adapters[1][1]
        adapters = [adapters[0], (adapters[1][0], wide[:, ::2], adapters[1][2])]
        assert not adapters[1][1].is_contiguous()
    return _x(K, dt, 3, seed=9), weights, adapters, biases, decoded, dt


@pytest.mark.parametrize("name", ["R=257", "f32 adapter", "lora_B strided"])
def test_what_the_adapter_launch_does_not_take_lands_in_the_composed_form(name):
    A, weights, adapters, biases, decoded, dt = _composed_case(name)
    before = bn.last_launch()
    _reset()
    ys = F.matmul_4bit_lora_grouped(A, weights, adapters, biases)
    assert bn.launch_log == [] and ln.launch_log == [] and gn.launch_log == [] and bn.last_launch() == before, f"{name}: a fused launch"
    assert len(ys) == 2 and all(y.dtype == DT[dt] and y.shape == (3, N) for y, N in zip(ys, (4, 6)))
    worst = _check_lora(ys, A, decoded, biases, adapters, DT[dt], "composed", name)
    if name == "R=257":
        assert "R = 257" in bn.last_error()
    print(f"composed {name}: worst err / bound {worst:.3f}")


# ----------------------------------------------------------------------------- the forms of A
@pytest.mark.parametrize("form", ["[M, K]", "[2, 3, K]", "strided", "other dtype"])
def test_input_forms(form):
    Ns, K, dt, Rs, M = (5, 1, 130), 2176, "bf16", (16, None, 65), 6
    weights, biases, decoded, adapters = _group(Ns, K, dt, bias=(1,), Rs=Rs)
    X = _x(K, dt, M)
    if form == "[M, K]":
        A, lead = X, (M,)
    elif form == "[2, 3, K]":
        A, lead = X.reshape(2, 3, K), (2, 3)
    elif form == "strided":
        wide = torch.zeros(M, 2 * K, dtype=X.dtype, device=DEV)
        wide[:, ::2] = X
        A, lead = wide[:, ::2], (M,)
        assert not A.is_contiguous()
    else:
        A, lead = X.float(), (M,)          # the weight dtype is asked for explicitly below
    cd = torch.bfloat16 if form == "other dtype" else None
    refs = _by_member(A, weights, biases, cd)
    want = F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
    _reset()
    ys = F.matmul_4bit_grouped(A, weights, biases, cd)
    zs = F.matmul_4bit_lora_grouped(A, weights, adapters, biases, cd)
    assert bn.launch_log == [(3, M, K, torch.bfloat16), (3, 81, M, K, torch.bfloat16)]
    for y, z, r, w, N in zip(ys, zs, refs, want, Ns):
        assert y.shape == z.shape == r.shape == lead + (N,) and y.dtype == z.dtype == r.dtype == torch.bfloat16
        assert torch.equal(y, r)
        assert torch.equal(z.reshape(M, N), w)      # the same rows through the same two launches: the same bits
    _check_lora(zs, X, decoded, biases, adapters, torch.bfloat16, "fused", form)


# ----------------------------------------------------------------------------- the modules
def _layer(N, K, dt, seed, bias):
    p, st, wd = _member(N, K, dt, seed=seed)
    base = bnb.Linear4bit(K, N, bias=bias, device=DEV, compute_dtype=DT[dt])
    base._set_quantized(p, st)
    if bias:
        with torch.no_grad():
            base.bias.copy_(_bias(N, dt, seed))
    return base, wd


def _lora_layer(base, N, K, dt, seed, r):
    layer = bnb.Linear4bitLoRA(base, r=r, lora_alpha=4.0)
    ad = _adapter(N, K, r, dt, seed)
    with torch.no_grad():
        layer.lora_A.copy_(ad[0])
        layer.lora_B.copy_(ad[1])
    assert layer.scaling == ad[2]
    return layer


@pytest.mark.parametrize("shape", [(3, 1024), (2, 3, 1024)], ids=["3xK", "2x3xK"])
def test_the_three_modules(shape):
    K, dt = 1024, "bf16"
    T = DT[dt]
    spec = ((8, 4), (4, 16), (6, 1))
    built = [_layer(N, K, dt, i, bias=i != 1) for i, (N, _) in enumerate(spec)]
    bases, decoded = [b[0] for b in built], [b[1] for b in built]
    loras = [_lora_layer(base, N, K, dt, i, r) for i, (base, (N, r)) in enumerate(zip(bases, spec))]
    rows = 1
    for d in shape[:-1]:
        rows *= d
    x = _x(K, dt, rows, seed=410 + len(shape)).reshape(shape)
    with torch.no_grad():
        want = [base(x) for base in bases]
        _reset()
        got = bnb.Linear4bitGroup(bases)(x)
        assert bn.launch_log == [(3, rows, K, T)] and gn.launch_log == []
        _reset()
        with_adapters = bnb.Linear4bitLoRAGroup(loras)(x)
        assert bn.launch_log == [(3, 21, rows, K, T)] and ln.launch_log == []
        _reset()
        alone = loras[1](x)
        assert bn.launch_log == [(1, 16, rows, K, T)] and ln.launch_log == []
    for y, z, r, (N, _) in zip(got, with_adapters, want, spec):
        assert y.shape == z.shape == r.shape == shape[:-1] + (N,) and y.dtype == z.dtype == T
        assert torch.equal(y, r)
    assert torch.equal(alone, with_adapters[1])      # the rows of a group of one are the rows of a group of three
    adapters = [(layer.lora_A.detach(), layer.lora_B.detach(), layer.scaling) for layer in loras]
    biases = [None if base.bias is None else base.bias.detach() for base in bases]
    _check_lora(with_adapters, x.reshape(-1, K), decoded, biases, adapters, T, "fused", f"Linear4bitLoRAGroup {shape}")
    # with gradients on (the biases and adapters are parameters) nothing is fused
    _reset()
    bnb.Linear4bitGroup(bases)(x)
    ys = bnb.Linear4bitLoRAGroup(loras)(x)
    assert bn.launch_log == [] and all(y.requires_grad for y in ys)


# ----------------------------------------------------------------------------- graph capture
def test_two_calls_captured_in_one_linear_graph_replay_with_new_inputs():
    K, dt, M = 2176, "bf16", 4
    T = DT[dt]
    w1, b1, _, a1 = _group((5, 1, 130), K, dt, bias=(1,), Rs=(16, None, 65))
    w2, b2, _, _ = _group((7, 9), K, dt, qt="fp4")
    A = _x(K, dt, M).clone()
    inputs = [_x(K, dt, M, seed=500 + i) for i in range(2)]
    eager = []
    for xin in inputs:
        eager.append(tuple(y.clone() for y in F.matmul_4bit_lora_grouped(xin, w1, a1, b1) + F.matmul_4bit_grouped(xin, w2, b2)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.matmul_4bit_lora_grouped(A, w1, a1, b1)          # warm-up outside the capture
        F.matmul_4bit_grouped(A, w2, b2)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    _reset()
    with torch.cuda.graph(graph, stream=stream):
        outs = F.matmul_4bit_lora_grouped(A, w1, a1, b1) + F.matmul_4bit_grouped(A, w2, b2)
    assert bn.launch_log == [(3, 81, M, K, T), (2, M, K, T)]
    for xin, want in zip(inputs, eager):
        A.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        for y, r in zip(outs, want):
            assert torch.equal(y, r)


# ----------------------------------------------------------------------------- non-finite activations
_NONFINITE = [("single", (4,), 128, "nf4", 64, (), (3,), "bf16", 3),                    # one 128-k block: every position in it
              ("bs32", (5, 18), 1024, "nf4", 32, (), (3, 16), "f16", 5),
              ("ragged", (5, 1, 130), 2176, "fp4", 64, (1,), (16, None, 65), "bf16", 16)]   # 17 blocks: wave 0's second trip holds the tail


@pytest.mark.parametrize("Ns, K, qt, bs, bias, Rs, dt, M", [p[1:] for p in _NONFINITE], ids=[p[0] for p in _NONFINITE])
def test_nonfinite_activations_stay_in_their_rows(guarded_alloc, Ns, K, qt, bs, bias, Rs, dt, M):
    """The planting passes of tests/nonfinite.py on k_skinny4_group, and on k_lora_down_rows + k_skinny4_group_lora: per pass a NaN row, Inf
    rows and an untouched row.  Without an adapter a member keeps matmul_4bit's bits on the same planted input; with one, every element is
    in the class (NaN, +Inf, -Inf, finite) of an explicit float64 IEEE evaluation of x . Wd^T + b + s (B . (A . x)), and a row without a
    plant keeps, bit for bit, the value it has when no row is planted."""
    T = DT[dt]
    weights, biases, decoded, adapters = _group(Ns, K, dt, qt, False, bs, bias, Rs)
    X0 = _x(K, dt, M)
    base = F.matmul_4bit_grouped(X0, weights, biases), F.matmul_4bit_lora_grouped(X0, weights, adapters, biases)
    for one in nonfinite.passes(M, K):
        X = nonfinite.planted(X0, one)
        free = nonfinite.untouched_rows(M, one)
        assert free
        guarded_alloc.begin(FILLS[0], where=f"M={M}, X{one}")
        refs = _by_member(X, weights, biases)
        _reset()
        got = F.matmul_4bit_grouped(X, weights, biases), F.matmul_4bit_lora_grouped(X, weights, adapters, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert bn.launch_log == [(len(Ns), M, K, T)] + [(n, total, M, K, T) for n, total in lc.chunks(Rs)], bn.launch_log
        for i, (y, r) in enumerate(zip(got[0], refs)):
            assert _same_bits(y, r), f"skinny_group member {i} of {Ns} differs from matmul_4bit with X{one}"
        for i, (y, r, wd, b, ad) in enumerate(zip(got[1], refs, decoded, biases, adapters)):
            if ad is None:
                assert _same_bits(y, r), f"skinny_group_lora member {i} of {Ns} (no adapter) differs from matmul_4bit with X{one}"
            nonfinite.assert_classes(y, nonfinite.adapter_classes(X, wd, b, ad), f"skinny_group_lora member {i} of {Ns}, X{one}")
        for ys, bs_ in zip(got, base):
            for i, (y, y0) in enumerate(zip(ys, bs_)):
                assert torch.equal(y[free], y0[free]), f"member {i} of {Ns}: a row without a plant changed with X{one}"
