"""
functional.matmul_4bit_grouped and nn.Linear4bitGroup on the GPU.

Every fused case runs on guarded allocations (tests/guard.py) under both fills and must equal matmul_4bit on the same member BIT FOR
BIT (so every element was written and none outside), show exactly the expected calls in the binding's launch log, and lie within the
elementwise bound of tests/elementwise.py around a float64 product with the CPU oracle's decoded weight.  The member-by-member cases
must show no fused launch and raise nothing.  Weights, activations and the oracle's decode are made once per shape and shared.
"""
import functools

import pytest
import torch

import oracle
import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _native, synthetic
from mps_bitsandbytes_amd import functional as F
from tests import nonfinite
from tests.elementwise import assert_linear_elementwise
from tests.guard import FILLS, guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.test_gpu_elementwise import _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@functools.lru_cache(maxsize=None)
def _member(N, K, dt, qt="nf4", nested=False, bs=64, seed=0):
    """(packed, QuantState) on the GPU and the oracle's decoded weight [N, K]; made once per argument tuple, never modified."""
    T = DT[dt]
    W = synthetic.normal((N, K), T, seed=100 + seed)
    op, oa, ost2 = oracle.quantize_4bit(W, bs, qt, nested)
    Wd = oracle.dequantize_4bit(op, oa, (N, K), bs, qt, T, ost2)
    st2 = None
    if nested:
        st2 = F.QuantState(absmax=ost2[0].to(DEV), shape=torch.Size([oa.numel()]), blocksize=ost2[1], quant_type="int8", dtype=torch.float32)
    st = F.QuantState(absmax=oa.to(DEV), shape=torch.Size([N, K]), blocksize=bs, quant_type=qt, dtype=T, state2=st2)
    return op.to(DEV), st, Wd


@functools.lru_cache(maxsize=None)
def _x(K, dt, seed=7):
    return synthetic.normal_device((1, K), DT[dt], seed=seed)


@functools.lru_cache(maxsize=None)
def _bias(N, dt, seed):
    return synthetic.normal_device((N,), DT[dt], seed=200 + seed)


def _group(Ns, K, dt, qt="nf4", nested=False, bias=(), bs=64):
    members = [_member(N, K, dt, qt, nested, bs, seed=i) for i, N in enumerate(Ns)]
    weights = [(p, st) for p, st, _ in members]
    biases = [_bias(N, dt, i) if i in bias else None for i, N in enumerate(Ns)]
    return weights, biases, [wd for _, _, wd in members]


def _chunks(G):
    return [min(16, G - c) for c in range(0, G, 16)]


# ----------------------------------------------------------------------------- the fused cases
# (id, member Ns, K, quant types, nested, members with a bias, the form the library must report for the last call)
_KU = [(4096, "ku2/KU2"), (6144, "ku3/KU3"), (8192, "ku4/KU4"), (8256, "ku5/KU6"), (12288, "ku6/KU6"), (12352, "ku7/KU8"),
       (16384, "ku8/KU8")]
FUSED = [
    ("single", (4,), 1024, ("nf4", "fp4"), False, (), "G1 ku1/KU1"),                    # a group of one; KU1, half a chunk
    ("ragged", (5, 1, 130), 2112, ("nf4", "fp4"), False, (1,), "G3 ku2/KU2"),           # partial last chunk, dead rows, bias in the middle
    ("nested", (7, 64), 2304, ("fp4", "nf4"), True, (0,), "G2 ku2/KU2"),                # absmax2 blocks that span rows
] + [(f"K{K}", (3, 6), K, ("nf4",), False, (), "G2 " + form) for K, form in _KU] + [
    ("K16384-nested", (3, 6), 16384, ("nf4",), True, (), "G2 ku8/KU8"),
    ("sixteen", tuple(1 + i % 5 for i in range(16)), 1024, ("nf4",), False, (3,), "G16 ku1/KU1"),     # one call
    ("seventeen", tuple(1 + i % 5 for i in range(17)), 1024, ("nf4",), False, (16,), "G1 ku1/KU1"),   # two calls: 16 + 1
]
_FUSED_PARAMS = [pytest.param(Ns, K, qt, nested, bias, form, dt, id=f"{name}-{qt}-{dt}")
                 for name, Ns, K, qts, nested, bias, form in FUSED for qt in qts for dt in ("f16", "bf16")]


@pytest.mark.parametrize("Ns, K, qt, nested, bias, form, dt", _FUSED_PARAMS)
def test_fused_group_equals_matmul_4bit_bit_for_bit(guarded_alloc, Ns, K, qt, nested, bias, form, dt):
    T = DT[dt]
    weights, biases, decoded = _group(Ns, K, dt, qt, nested, bias)
    X = _x(K, dt)
    guarded_alloc.begin(FILLS[0], where="reference")
    refs = [F.matmul_4bit(X, p, st, b) for (p, st), b in zip(weights, biases)]
    assert _native.last_variant().startswith("gemv_lean"), _native.last_variant()
    guarded_alloc.check()
    for fill in FILLS:
        guarded_alloc.begin(fill, where=f"matmul_4bit_grouped fill 0x{fill:02X}")
        gn.reset_launch_log()
        ys = F.matmul_4bit_grouped(X, weights, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert gn.launch_log == [(n, K, T) for n in _chunks(len(Ns))], gn.launch_log
        assert gn.last_launch() == "gemv_group " + form
        assert isinstance(ys, tuple) and len(ys) == len(Ns)
        for i, (y, r) in enumerate(zip(ys, refs)):
            assert y.shape == r.shape == (1, Ns[i]) and y.dtype == r.dtype == T
            assert torch.equal(y, r), f"member {i} of {Ns} differs from matmul_4bit under fill 0x{fill:02X}"
    worst = 0.0
    for y, wd, b in zip(ys, decoded, biases):
        worst = max(worst, assert_linear_elementwise(y, X, wd, b, T, T, "gemv_group"))
    print(f"gemv_group {form} {qt} {dt} N={Ns} K={K}: worst err / bound {worst:.3f}")


# ----------------------------------------------------------------------------- the forms of A
@pytest.mark.parametrize("form", ["[K]", "[1, K]", "[1, 1, K]", "strided", "other dtype"])
def test_input_forms(form):
    Ns, K, dt = (5, 1, 130), 2112, "bf16"
    weights, biases, _ = _group(Ns, K, dt, bias=(1,))
    X = _x(K, dt)
    if form == "[K]":
        A, lead = X.reshape(K), ()
    elif form == "[1, K]":
        A, lead = X, (1,)
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
    refs = [F.matmul_4bit(A, p, st, b, cd) for (p, st), b in zip(weights, biases)]
    gn.reset_launch_log()
    ys = F.matmul_4bit_grouped(A, weights, biases, cd)
    assert gn.launch_log == [(3, K, torch.bfloat16)]
    for y, r, N in zip(ys, refs, Ns):
        assert y.shape == r.shape == lead + (N,) and y.dtype == r.dtype
        assert torch.equal(y, r)


# ----------------------------------------------------------------------------- what runs member by member
def _by_member_case(name):
    """(A, weights, biases, compute_dtype) of a call the fused launch does not serve."""
    dt, K, Ns = "bf16", 1024, (4, 6)
    cd = None
    if name == "M=2":
        weights, biases, _ = _group(Ns, K, dt)
        A = synthetic.normal_device((2, K), DT[dt], seed=9)
    elif name == "K=512":
        K = 512
        weights, biases, _ = _group(Ns, K, dt)
        A = _x(K, dt)
    elif name == "blocksize 128":
        weights, biases, _ = _group(Ns, K, dt, bs=128)
        A = _x(K, dt)
    elif name == "nf4 with fp4":
        weights = [_member(4, K, dt, "nf4")[:2], _member(6, K, dt, "fp4", seed=1)[:2]]
        biases, A = [None, None], _x(K, dt)
    elif name == "plain with nested":
        weights = [_member(4, K, dt)[:2], _member(6, K, dt, nested=True, seed=1)[:2]]
        biases, A = [None, None], _x(K, dt)
    elif name == "compute_dtype f32":
        weights, biases, _ = _group(Ns, K, dt)
        A, cd = _x(K, dt), torch.float32
    elif name == "f32 weight":
        weights, biases, _ = _group(Ns, K, "f32")
        A = _x(K, "f32")
    else:
        assert name == "packed+1"
        weights, biases, _ = _group(Ns, K, dt)
        p, st = weights[1]
        buf = torch.empty(p.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = p.reshape(-1)
        weights = [weights[0], (buf[1:].view(p.shape), st)]
        assert weights[1][0].data_ptr() % 16 == 1 and weights[1][0].is_contiguous()
        A = _x(K, dt)
    return A, weights, biases, cd


@pytest.mark.parametrize("name", ["M=2", "K=512", "blocksize 128", "nf4 with fp4", "plain with nested", "compute_dtype f32", "f32 weight",
                                  "packed+1"])
def test_everything_else_runs_member_by_member(name):
    A, weights, biases, cd = _by_member_case(name)
    refs = [F.matmul_4bit(A, p, st, b, cd) for (p, st), b in zip(weights, biases)]
    gn.reset_launch_log()
    ys = F.matmul_4bit_grouped(A, weights, biases, cd)
    assert gn.launch_log == [], f"{name}: a fused launch"
    assert len(ys) == len(refs)
    for y, r in zip(ys, refs):
        assert y.shape == r.shape and y.dtype == r.dtype and torch.equal(y, r)


def test_a_wanted_gradient_runs_member_by_member_and_sums_the_members_gradients():
    Ns, K, dt = (4, 6), 1024, "bf16"          # two members: the sum of two gradients has one order
    weights, biases, _ = _group(Ns, K, dt, bias=(1,))
    seeds = [synthetic.normal_device((1, N), DT[dt], seed=300 + i) for i, N in enumerate(Ns)]
    alone, refs = [], []
    for (p, st), b, s in zip(weights, biases, seeds):
        a = _x(K, dt).clone().requires_grad_(True)
        y = F.matmul_4bit(a, p, st, b)
        y.backward(s)
        alone.append(a.grad)
        refs.append(y.detach())
    A = _x(K, dt).clone().requires_grad_(True)
    gn.reset_launch_log()
    ys = F.matmul_4bit_grouped(A, weights, biases)
    assert gn.launch_log == []
    for y, r in zip(ys, refs):
        assert y.requires_grad and torch.equal(y, r)
    torch.autograd.backward(ys, seeds)
    assert torch.equal(A.grad, alone[0] + alone[1])


def test_a_mismatched_member_raises_what_matmul_4bit_raises():
    weights, biases, _ = _group((4, 6), 1024, "bf16")
    other = _member(4, 2112, "bf16")[:2]
    with pytest.raises(RuntimeError, match="mat1 and mat2 shapes cannot be multiplied"):
        F.matmul_4bit_grouped(_x(1024, "bf16"), [weights[0], other])
    assert F.matmul_4bit_grouped(_x(1024, "bf16"), []) == ()


# ----------------------------------------------------------------------------- the layer
def test_layer_group_equals_its_layers_called_alone():
    K, dt = 1024, torch.bfloat16
    layers = []
    for i, N in enumerate((8, 4, 6)):
        lin = torch.nn.Linear(K, N, bias=i != 1, dtype=dt, device=DEV)
        with torch.no_grad():
            lin.weight.copy_(synthetic.normal_device((N, K), dt, seed=400 + i))
        layers.append(lin)
    group = bnb.Linear4bitGroup.from_linears(layers, quant_type="fp4")
    assert [layer.quant_type for layer in group.layers] == ["fp4"] * 3
    q, k, v = group.layers
    for shape in ((1, K), (K,), (1, 1, K), (3, K), (2, 3, K)):
        x = synthetic.normal_device(shape, dt, seed=410 + len(shape))
        rows = x.numel() // K
        with torch.no_grad():
            want = (q(x), k(x), v(x))
            gn.reset_launch_log()
            got = group(x)
        assert gn.launch_log == ([(3, K, dt)] if rows == 1 else []), (shape, gn.launch_log)
        assert isinstance(got, tuple) and len(got) == 3
        for y, r in zip(got, want):
            assert y.shape == r.shape and torch.equal(y, r), shape
    # with gradients on (the biases are parameters) the layers run one by one and stay differentiable
    x = synthetic.normal_device((1, K), dt, seed=420)
    gn.reset_launch_log()
    got = group(x)
    assert gn.launch_log == [] and [y.requires_grad for y in got] == [True, False, True]
    for y, layer in zip(got, group.layers):
        assert torch.equal(y, layer(x))


# ----------------------------------------------------------------------------- graph capture
def test_two_grouped_calls_captured_as_one_chain_replay_with_new_inputs():
    K, dt = 2112, "bf16"
    w1, b1, _ = _group((5, 1, 130), K, dt, bias=(1,))
    w2, b2, _ = _group((7, 9), K, dt, qt="fp4")
    A = _x(K, dt).clone()
    inputs = [synthetic.normal_device((1, K), DT[dt], seed=500 + i) for i in range(2)]
    eager = []
    for xin in inputs:
        eager.append(tuple(y.clone() for y in F.matmul_4bit_grouped(xin, w1, b1) + F.matmul_4bit_grouped(xin, w2, b2)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.matmul_4bit_grouped(A, w1, b1)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    gn.reset_launch_log()
    with torch.cuda.graph(graph, stream=stream):
        outs = F.matmul_4bit_grouped(A, w1, b1) + F.matmul_4bit_grouped(A, w2, b2)
    assert gn.launch_log == [(3, K, DT[dt]), (2, K, DT[dt])]
    for xin, want in zip(inputs, eager):
        A.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        for y, r in zip(outs, want):
            assert torch.equal(y, r)


# ----------------------------------------------------------------------------- non-finite activations
@pytest.mark.parametrize("Ns, K, nested, bias, dt", [((5, 1, 130), 1088, False, (1,), "bf16"),      # a partial (and the only) 2048-chunk
                                                     ((7, 64), 2304, True, (0,), "f16")],           # ... the second one partial, nested absmax
                         ids=["K1088", "K2304-nested"])
def test_nonfinite_activations_keep_matmul_4bits_bits(guarded_alloc, Ns, K, nested, bias, dt):
    """An Inf of either sign at every special place of the row (tests/nonfinite.py), one launch each: every member keeps matmul_4bit's
    bits on the same planted input (NaN in the same places, every other element bit-equal), and NaN / +-Inf sit exactly where the
    operands put them -- an Inf past which the row's last chunk reads zeros must not become Inf * 0."""
    T = DT[dt]
    weights, biases, decoded = _group(Ns, K, dt, "nf4", nested, bias)
    for one in nonfinite.passes(1, K):
        X = nonfinite.planted(_x(K, dt), one)
        guarded_alloc.begin(FILLS[0], where=f"matmul_4bit_grouped, X{one}")
        refs = [F.matmul_4bit(X, p, st, b) for (p, st), b in zip(weights, biases)]
        assert _native.last_variant().startswith("gemv_lean"), _native.last_variant()
        gn.reset_launch_log()
        ys = F.matmul_4bit_grouped(X, weights, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert gn.launch_log == [(len(Ns), K, T)], gn.launch_log
        for i, (y, r, wd, b) in enumerate(zip(ys, refs, decoded, biases)):
            assert _same_bits(y, r), f"member {i} of {Ns} differs from matmul_4bit with X{one}"
            assert_linear_elementwise(y, X, wd, b, T, T, f"gemv_group, X{one}")
