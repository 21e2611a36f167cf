"""
functional.matmul_4bit_multilora_grouped and the two modules above it on the GPU (libmbnb_mlora.so): 2 to 16 rows, each with its own slot
of the members' adapter banks, the slots read on the device.

Every fused case (tests/mlora_cases.py) runs on guarded allocations (tests/guard.py) under both fills -- the f32 workspace `t` is one of
them, so a t element read before it is written shows, and the rows of t that belong to a row without an adapter must keep the fill --
with the ids in a guarded buffer of their own, and must show exactly the expected call in the binding's launch log and the library's
report.  Row m of every output must equal, BIT FOR BIT, row m of matmul_4bit_lora_grouped (its 2 ... 16 row path, libmbnb_batch.so) with
the one adapter (lora_A[s], lora_B[s], float(scaling[s])), s = ids[m], and matmul_4bit's row where ids[m] is outside the bank: the
summation chains of the two libraries are the same, and this is what holds them together.  Each element must lie within the fused
bound of tests/lora_bound.py around the float64 value formed with its row's adapter; tests/test_mlora_host.py holds that the next
slot's adapter, or none, would fail that bound in every such row.  What declines must show no launch and lie within the composed bound.
"""
import functools

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _batch_native as bn
from mps_bitsandbytes_amd import _mlora_native as mn
from mps_bitsandbytes_amd import functional as F
from tests import lora_cases as lc
from tests import mlora_cases as mc
from tests import nonfinite
from tests.elementwise import assert_bound_elementwise
from tests.guard import FILLS, guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.test_gpu_elementwise import _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = mc.DT


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
    return mc.x(K, dt, M, seed).to(DEV)


@functools.lru_cache(maxsize=None)
def _bias(N, dt, seed):
    return lc.bias(N, dt, seed).to(DEV)


@functools.lru_cache(maxsize=None)
def _bank(N, K, R, S, dt, seed):
    bank = mc.bank(N, K, R, S, dt, seed)
    return None if bank is None else tuple(t.to(DEV) for t in bank)


def _group(Ns, K, dt, qt="nf4", nested=False, bs=64, bias=(), Rs=None, S=3):
    members = [_member(N, K, dt, qt, nested, bs, seed=i) for i, N in enumerate(Ns)]
    weights = [(p, st) for p, st, _ in members]
    biases = [_bias(N, dt, i) if i in bias else None for i, N in enumerate(Ns)]
    banks = None if Rs is None else [_bank(N, K, R, S, dt, i) for i, (N, R) in enumerate(zip(Ns, Rs))]
    return weights, biases, [wd for _, _, wd in members], banks


def _ids(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _single(banks, s):
    """The members' adapters of slot s in the form matmul_4bit_lora_grouped takes."""
    return [None if b is None else (b[0][s], b[1][s], float(b[2][s])) for b in banks]


def _row_references(X, weights, biases, banks, ids, S):
    """Per row, what contract 2 names: the existing single-adapter call (fused: its launch log says so) per distinct slot, and
    matmul_4bit for the rows without an adapter.  One list of [M, N_g] tensors."""
    M = X.shape[0]
    plain = [F.matmul_4bit(X, p, st, b) for (p, st), b in zip(weights, biases)]
    want = [y.clone() for y in plain]
    for s in sorted(set(i for i in ids if 0 <= i < S)):
        bn.reset_launch_log()
        ys = F.matmul_4bit_lora_grouped(X, weights, _single(banks, s), biases)
        assert len(bn.launch_log) == (len(weights) + 15) // 16 and all(len(e) == 5 for e in bn.launch_log), bn.launch_log      # gemm4_lora entries
        rows = torch.tensor([i == s for i in ids], device=DEV)
        for w, y in zip(want, ys):
            w[rows] = y[rows]
    return want, plain


def _check_bound(ys, X, decoded, biases, banks, ids, T, path, kernel):
    worst = 0.0
    for y, wd, b, bank in zip(ys, decoded, biases, banks):
        r, S, R = mc.reference(X.reshape(-1, X.shape[-1]), wd, b, bank, ids)
        y2 = y.reshape(-1, y.shape[-1])
        assert y2.dtype == T and y2.shape == r.shape
        worst = max(worst, assert_bound_elementwise(y2, r, mc.bound(r, S, R, X.shape[-1], T, path), kernel,
                                                    "y[m] = X[m] . Wd^T + b + s (X[m] . A_s^T) . B_s^T"))
    return worst


# ----------------------------------------------------------------------------- the fused cases
@pytest.mark.parametrize("Ns, K, qt, nested, bs, bias, S, Rs, dt, M, pattern", mc.ARGS, ids=mc.IDS)
def test_fused_rows_equal_the_single_adapter_launch_bit_for_bit_on_poisoned_buffers(guarded_alloc, Ns, K, qt, nested, bs, bias, S, Rs, dt, M, pattern):
    T = DT[dt]
    weights, biases, decoded, banks = _group(Ns, K, dt, qt, nested, bs, bias, Rs, S)
    X = _x(K, dt, M)
    ids = mc.ids_for(pattern, M, S)
    have = [0 <= i < S for i in ids]
    guarded_alloc.begin(FILLS[0], where="reference")
    want, plain = _row_references(X, weights, biases, banks, ids, S)
    guarded_alloc.check()
    form = mc.report(Rs, K, M)
    total = sum(r or 0 for r in Rs)
    worst, seen = 0.0, []
    for fill in FILLS:
        guarded_alloc.begin(fill, where=f"matmul_4bit_multilora_grouped M={M} {pattern} fill 0x{fill:02X}")
        dev_ids = guarded_alloc.place("ids", _ids(ids))
        mn.reset_launch_log()
        bn.reset_launch_log()
        ys = F.matmul_4bit_multilora_grouped(X, weights, banks, dev_ids, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert len(guarded_alloc.allocs) == 3 and guarded_alloc.allocs[2].view.dtype == torch.float32      # the ids, the outputs, and t
        assert guarded_alloc.allocs[1].view.numel() == M * sum(Ns) and guarded_alloc.allocs[2].view.numel() == M * total
        assert mn.launch_log == [(n, tot, M, K, T) for n, tot in mc.chunks(Rs)], mn.launch_log
        assert bn.launch_log == [] and mn.last_launch() == form, mn.last_launch()
        assert torch.equal(dev_ids, _ids(ids))
        assert isinstance(ys, tuple) and len(ys) == len(Ns)
        for i, (y, w) in enumerate(zip(ys, want)):
            assert y.shape == (M, Ns[i]) and y.dtype == T and y.is_contiguous()
            for m in range(M):      # contract 2, row by row
                assert torch.equal(y[m], w[m]), (f"member {i} of {Ns}, row {m} (slot {ids[m]}) differs from "
                                                 f"{'matmul_4bit_lora_grouped' if have[m] and Rs[i] else 'matmul_4bit'} under fill 0x{fill:02X}")
            if Rs[i] is None:
                assert torch.equal(y, plain[i])
        worst = max(worst, _check_bound(ys, X, decoded, biases, banks, ids, T, "fused", form))
        # t: member g's [M, R_g] block holds the down-projection in the rows that have an adapter, and the fill in the others
        t, o = guarded_alloc.allocs[2].view, 0
        for R in Rs:
            if R is None:
                continue
            block = t[o:o + M * R].view(M, R)
            o += M * R
            for m in range(M):
                if have[m]:
                    assert bool(torch.isfinite(block[m]).all()) and not bool((block[m].view(torch.uint8) == fill).all()), (m, R)
                else:
                    assert bool((block[m].view(torch.uint8) == fill).all()), f"t row {m} of a row without an adapter was written"
        seen.append([y.clone() for y in ys])
    for a, b in zip(*seen):      # a second call, on other buffers with another fill: equal bits
        assert torch.equal(a, b)
    # what an unselected slot holds never reaches a row
    unused = sorted(set(range(S)) - set(ids))
    if unused:
        poisoned = []
        for bank in banks:
            if bank is None:
                poisoned.append(None)
                continue
            a, b, sc = (t.clone() for t in bank)
            for s in unused:
                a[s], b[s], sc[s] = float("nan"), float("nan"), float("nan")
            poisoned.append((a, b, sc))
        for y, w in zip(F.matmul_4bit_multilora_grouped(X, weights, poisoned, _ids(ids), biases), seen[0]):
            assert torch.equal(y, w), f"a NaN in the unselected slots {unused} changed an output"
    print(f"{form} {qt} {dt} bs={bs} N={Ns[:4]} R={Rs[:4]} S={S} ids={ids}: worst err / bound {worst:.3f}")


def test_rows_do_not_leak_into_each_other_and_ids_of_another_dtype_are_converted():
    Ns, K, dt, Rs, S, M = (5, 1, 130), 2176, "bf16", (3, None, 16), 3, 5
    weights, biases, _, banks = _group(Ns, K, dt, bias=(1,), Rs=Rs, S=S)
    X, other = _x(K, dt, M), _x(K, dt, M, seed=31)
    ids = [2, -1, 0, 1, 2]
    base = F.matmul_4bit_multilora_grouped(X, weights, banks, _ids(ids), biases)
    for m in range(M):
        mixed = other.clone()
        mixed[m] = X[m]
        mixed_ids = [(i + 1) % S for i in ids]
        mixed_ids[m] = ids[m]
        mn.reset_launch_log()
        got = F.matmul_4bit_multilora_grouped(mixed, weights, banks, torch.tensor(mixed_ids, device=DEV), biases)      # int64 ids
        assert mn.launch_log == [(3, 19, M, K, DT[dt])]
        for w, y in zip(base, got):
            assert torch.equal(w[m], y[m]), f"row {m} depends on the other rows"
    # a batch of 2 holding rows 0 and 1 gives those rows of the batch of 5 (the summation order does not depend on M)
    for w, y in zip(base, F.matmul_4bit_multilora_grouped(X[:2], weights, banks, _ids(ids[:2]), biases)):
        assert torch.equal(w[:2], y)


# ----------------------------------------------------------------------------- what declines
def _composed_case(name):
    """(A, weights, banks, biases, decoded, ids) of a call the fused launches do not serve."""
    dt, K, Ns, Rs, S = "bf16", 1024, (4, 6), (3, 8), 3
    M = {"M=17": 17, "one row": 1}.get(name, 3)
    if name == "R=65":
        Rs = (3, 65)
    weights, biases, decoded, banks = _group(Ns, K, dt, bias=(1,), Rs=Rs, S=S)
    A = _x(K, dt, M, seed=9)
    if name == "f32 bank":
        banks = [banks[0], (banks[1][0].float(), banks[1][1].float(), banks[1][2])]
    elif name == "lora_B strided":
        wide = torch.zeros(S, 6, 16, dtype=DT[dt], device=DEV)
        wide[:, :, ::2] = banks[1][1]
        banks = [banks[0], (banks[1][0], wide[:, :, ::2], banks[1][2])]
        assert not banks[1][1].is_contiguous()
    elif name == "packed+1":
        p, st = weights[1]
        buf = torch.empty(p.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = p.reshape(-1)
        weights = [weights[0], (buf[1:].view(p.shape), st)]
        assert weights[1][0].data_ptr() % 16 == 1 and weights[1][0].is_contiguous()
    elif name == "gradient":
        A = A.clone().requires_grad_(True)
        banks = [tuple(t.clone().requires_grad_(j < 2) for j, t in enumerate(bank)) for bank in banks]
    ids = [(m * 2) % (S + 1) - (m % 4 == 3) for m in range(M)]      # slots 0 ... S - 1, S and -1
    return A, weights, banks, biases, decoded, ids


@pytest.mark.parametrize("name", ["M=17", "one row", "R=65", "f32 bank", "lora_B strided", "packed+1", "gradient"])
def test_what_the_fused_launches_do_not_take_lands_in_the_composed_form(name):
    A, weights, banks, biases, decoded, ids = _composed_case(name)
    T = torch.bfloat16
    before = mn.last_launch()
    mn.reset_launch_log()
    ys = F.matmul_4bit_multilora_grouped(A, weights, banks, _ids(ids), biases)
    assert mn.launch_log == [] and mn.last_launch() == before, f"{name}: a fused launch"
    assert len(ys) == 2 and all(y.dtype == T and y.shape == (A.shape[0], N) for y, N in zip(ys, (4, 6)))
    detached = [tuple(t.detach() for t in bank) for bank in banks]
    worst = _check_bound([y.detach() for y in ys], A.detach(), decoded, biases, detached, ids, T, "composed", name)
    for (p, st), b, y in zip(weights, biases, ys):      # rows without an adapter: matmul_4bit's bits
        base = F.matmul_4bit(A.detach(), p, st, b)
        for m, s in enumerate(ids):
            if not 0 <= s < 3:
                assert torch.equal(y[m].detach(), base[m])
    if name == "packed+1":
        assert mn.last_error().startswith("mbnb_mlora_gemm4: ") and "not 16-byte aligned" in mn.last_error()
    if name == "gradient":
        # the explicit torch expression on the dequantised weight
        A2 = A.detach().clone().requires_grad_(True)
        banks2 = [tuple(t.detach().clone().requires_grad_(j < 2) for j, t in enumerate(bank)) for bank in banks]
        sel = _ids(ids)
        seeds = [lc.x(N, "bf16", 300 + i, A.shape[0]).to(DEV) for i, N in enumerate((4, 6))]
        ref = []
        for (p, st), b, (la, lb, sc) in zip(weights, biases, banks2):
            y2 = A2 @ F.dequantize_4bit(p, st).t()
            if b is not None:
                y2 = y2 + b
            for s in range(3):
                y2 = torch.where((sel == s).unsqueeze(-1), y2 + ((A2 @ la[s].t()) @ lb[s].t()) * sc[s], y2)
            ref.append(y2)
        torch.autograd.backward(ys, seeds)
        torch.autograd.backward(ref, seeds)
        torch.testing.assert_close(A.grad, A2.grad)      # (the values themselves are held by the composed bound above)
        for bank, bank2 in zip(banks, banks2):
            torch.testing.assert_close(bank[0].grad, bank2[0].grad)
            torch.testing.assert_close(bank[1].grad, bank2[1].grad)
    print(f"composed {name}: worst err / bound {worst:.3f}")


# ----------------------------------------------------------------------------- the modules
def _layer(N, K, dt, seed, bias, S, r):
    p, st, wd = _member(N, K, dt, seed=seed)
    base = bnb.Linear4bit(K, N, bias=bias, device=DEV, compute_dtype=DT[dt])
    base._set_quantized(p, st)
    if bias:
        with torch.no_grad():
            base.bias.copy_(_bias(N, dt, seed))
    layer = bnb.Linear4bitMultiLoRA(base, S, r, lora_alpha=4.0)
    bank = _bank(N, K, r, S, dt, seed)
    for s in range(S):
        layer.load_adapter(s, bank[0][s], bank[1][s], float(bank[2][s]))
    return layer, wd


@pytest.mark.parametrize("shape", [(3, 1024), (2, 3, 1024)], ids=["3xK", "2x3xK"])
def test_the_two_modules(shape):
    K, dt, S = 1024, "bf16", 3
    T = DT[dt]
    spec = ((8, 4), (4, 16), (6, 1))
    built = [_layer(N, K, dt, i, i != 1, S, r) for i, (N, r) in enumerate(spec)]
    layers, decoded = [b[0] for b in built], [b[1] for b in built]
    rows = 1
    for d in shape[:-1]:
        rows *= d
    x = _x(K, dt, rows, seed=410 + len(shape)).reshape(shape)
    flat = [2, -1, 0, 1, 3, 2][:rows]
    ids = _ids(flat).reshape(shape[:-1])
    with torch.no_grad():
        mn.reset_launch_log()
        ys = bnb.Linear4bitMultiLoRAGroup(layers)(x, ids)
        assert mn.launch_log == [(3, 21, rows, K, T)]
        mn.reset_launch_log()
        alone = layers[1](x, ids)
        assert mn.launch_log == [(1, 16, rows, K, T)]
        bases = [layer.base(x) for layer in layers]
    for y, base, (N, _) in zip(ys, bases, spec):
        assert y.shape == shape[:-1] + (N,) and y.dtype == T
        for m, s in enumerate(flat):
            assert torch.equal(y.reshape(rows, N)[m], base.reshape(rows, N)[m]) == (not 0 <= s < S), (m, s)
    assert torch.equal(alone, ys[1])      # the rows of a group of one are the rows of a group of three
    banks = [tuple(t.detach() for t in layer.bank()) for layer in layers]
    biases = [None if layer.base.bias is None else layer.base.bias.detach() for layer in layers]
    _check_bound(ys, x.reshape(-1, K), decoded, biases, banks, flat, T, "fused", f"Linear4bitMultiLoRAGroup {shape}")
    # with gradients on (the banks are parameters) nothing is fused
    mn.reset_launch_log()
    zs = bnb.Linear4bitMultiLoRAGroup(layers)(x, ids)
    assert mn.launch_log == [] and all(z.requires_grad for z in zs)
    _check_bound([z.detach() for z in zs], x.reshape(-1, K), decoded, biases, banks, flat, T, "composed", "composed modules")


# ----------------------------------------------------------------------------- graph capture
def test_two_calls_in_one_linear_graph_replay_with_new_ids_and_a_new_slot():
    K, dt, M, S = 2176, "bf16", 4, 3
    T = DT[dt]
    layers = [_layer(N, K, dt, i, i == 1, S, r)[0] for i, (N, r) in enumerate(((5, 3), (1, 16), (130, 3)))]
    group = bnb.Linear4bitMultiLoRAGroup(layers)
    w2, b2, _, k2 = _group((7, 9), K, dt, qt="fp4", Rs=(16, 3), S=S)
    k2 = [tuple(t.clone() for t in bank) for bank in k2]
    A = _x(K, dt, M).clone()
    ids = _ids([0, 1, 2, -1])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(stream):
            group(A, ids)          # warm-up outside the capture
            F.matmul_4bit_multilora_grouped(A, w2, k2, ids, b2)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        mn.reset_launch_log()
        with torch.cuda.graph(graph, stream=stream):
            outs = group(A, ids) + F.matmul_4bit_multilora_grouped(A, w2, k2, ids, b2)
        assert mn.launch_log == [(3, 22, M, K, T), (2, 19, M, K, T)]
        new = _bank(130, K, 3, S, dt, 5)      # another adapter for slot 1 of the third layer and of the second call's first member
        new2 = _bank(7, K, 16, S, dt, 6)
        for step, (new_ids, reload) in enumerate((([0, 1, 2, -1], False), ([1, 1, 3, 0], False), ([2, -5, 1, 1], True))):
            ids.copy_(_ids(new_ids))
            A.copy_(_x(K, dt, M, seed=500 + step))
            if reload:
                layers[2].load_adapter(1, new[0][2], new[1][2], 0.625)
                k2[0][0][1].copy_(new2[0][0])
                k2[0][1][1].copy_(new2[1][0])
                k2[0][2][1] = 1.75
            graph.replay()
            torch.cuda.synchronize()
            got = [y.clone() for y in outs]
            want = group(A, ids) + F.matmul_4bit_multilora_grouped(A, w2, k2, ids, b2)      # eager, with the new values
            for y, r in zip(got, want):
                assert torch.equal(y, r), f"replay {step} differs from an eager call"
        assert not torch.equal(got[2][3], layers[2].base(A)[3])      # the reloaded slot 1 is in use in row 3


# ----------------------------------------------------------------------------- non-finite activations
_NONFINITE = [("single", (4,), 128, (), (3,), "bf16"),                     # one 128-k block: every position in it
              ("ragged", (5, 1, 130), 2176, (1,), (3, None, 16), "f16")]    # 17 blocks: wave 0's second trip holds the tail


@pytest.mark.parametrize("Ns, K, bias, Rs, dt", [p[1:] for p in _NONFINITE], ids=[p[0] for p in _NONFINITE])
def test_nonfinite_activations_stay_in_their_rows(guarded_alloc, Ns, K, bias, Rs, dt):
    """The planting passes of tests/nonfinite.py on k_lora_down_sel + k_skinny4_mlora, five rows with the slots 0, -1, 1, S, 2: over the passes
    a NaN and an Inf land in rows with an adapter and in rows whose id is outside the bank.  A row without an adapter (and a member without
    a bank) keeps matmul_4bit's bits on the same planted input; a row with one has every element in the class (NaN, +Inf, -Inf, finite) of
    an explicit float64 IEEE evaluation of x . Wd^T + b + s (B . (A . x)) with its slot's adapter; a row without a plant keeps, bit for
    bit, the value it has when no row is planted."""
    T, S, M = DT[dt], 3, 5
    ids = [0, -1, 1, S, 2]
    have = [0 <= i < S for i in ids]
    weights, biases, decoded, banks = _group(Ns, K, dt, bias=bias, Rs=Rs, S=S)
    X0 = _x(K, dt, M)
    base = F.matmul_4bit_multilora_grouped(X0, weights, banks, _ids(ids), biases)
    planted_with, planted_without = set(), set()
    for one in nonfinite.passes(M, K):
        X = nonfinite.planted(X0, one)
        free = nonfinite.untouched_rows(M, one)
        assert free
        for r, _, _ in one:
            (planted_with if have[r] else planted_without).add(r)
        guarded_alloc.begin(FILLS[0], where=f"matmul_4bit_multilora_grouped, X{one}")
        plain = [F.matmul_4bit(X, p, st, b) for (p, st), b in zip(weights, biases)]
        dev_ids = guarded_alloc.place("ids", _ids(ids))
        mn.reset_launch_log()
        ys = F.matmul_4bit_multilora_grouped(X, weights, banks, dev_ids, biases)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert mn.launch_log == [(n, tot, M, K, T) for n, tot in mc.chunks(Rs)], mn.launch_log
        for i, (y, y0, r, wd, b, bank) in enumerate(zip(ys, base, plain, decoded, biases, banks)):
            want = nonfinite.adapter_classes(X, wd, b)
            for m in range(M):
                if bank is None or not have[m]:
                    assert _same_bits(y[m], r[m]), f"member {i} of {Ns}, row {m} (slot {ids[m]}) differs from matmul_4bit with X{one}"
                else:
                    s = ids[m]
                    want[m] = nonfinite.adapter_classes(X[m:m + 1], wd, b, (bank[0][s], bank[1][s], float(bank[2][s])))[0]
            nonfinite.assert_classes(y, want, f"skinny_mlora member {i} of {Ns}, X{one}")
            assert torch.equal(y[free], y0[free]), f"member {i} of {Ns}: a row without a plant changed with X{one}"
    assert planted_with and planted_without
