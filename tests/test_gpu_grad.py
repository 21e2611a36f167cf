"""Input and bias gradients of matmul_4bit / linear_int8 / linear_dense / matmul_fp8_e4m3 and of Linear4bit / Linear8bit / LinearFP8
on the MI355X: they exist; at dense shapes they are bit for bit the library's own forward machinery run on the transposed dequantised
weight; the transposed pass is bit for bit dequantize_*(...).t(); the reference's autograd (g9 goldens) and an f64 host product hold
under the per-dtype gates; inference is unchanged; and a two-layer QLoRA model trains its adapters as one on dequantised nn.Linear."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, synthetic
from mps_bitsandbytes_amd import functional as F
from tests.goldenio import DT, from_bits, rel_fro
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name: every torch.empty of functional.py comes back 0xFF)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"
TOL = {torch.float16: 2e-4, torch.bfloat16: 2e-3, torch.float32: 2e-6}     # the gates of test_gpu_parity.py


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_bits_but_nan_payload(a, b):
    """Bit-equal wherever a value is a number; NaN in the same places (the FP8 decoders of the library differ in NaN payload / sign only)."""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and _same_bits(torch.where(nan, 0, a), torch.where(nan, 0, b))


def _backward_kernel(x):
    """A list that receives mbnb_last_kernel() as seen right after x's gradient was computed: autograd runs a CUDA backward on its own
    device thread, and the library's last-kernel record is per thread."""
    seen = []
    x.register_hook(lambda g: seen.append(_native.last_kernel()))
    return seen


def _q4(N, K, dt, qt="nf4", bs=64, cs=False, seed=1):
    W = synthetic.normal_device((N, K), dt, seed=seed, std=0.05)
    return (W,) + F.quantize_4bit(W, blocksize=bs, compress_statistics=cs, quant_type=qt)


# ----------------------------------------------------------------------------------------------------- 1. the gradients exist
def _fwd_cases(dt=torch.bfloat16, M=6, N=256, K=128):
    """(name, forward(x, bias), weight dtype) for the four functions and the three modules."""
    W = synthetic.normal_device((N, K), dt, seed=5, std=0.05)
    packed, st = F.quantize_4bit(W, blocksize=64, quant_type="nf4")
    q8, s8 = F.quantize_rowwise(W)
    qf, sf = F.quantize_fp8_e4m3(W)
    Wd = F.dequantize_rowwise(q8, s8, dt)
    lin = torch.nn.Linear(K, N).to(dt).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
    m4 = bnb.Linear4bit.from_linear(lin)
    m8 = bnb.Linear8bit.from_linear(lin)
    m8n = bnb.Linear8bit.from_linear(lin, use_cache=False)
    mf = bnb.LinearFP8.from_linear(lin)
    return [("matmul_4bit", lambda x, b: F.matmul_4bit(x, packed, st, b)),
            ("linear_int8", lambda x, b: F.linear_int8(x, q8, s8, b)),
            ("linear_dense", lambda x, b: F.linear_dense(x, Wd, b)),
            ("matmul_fp8_e4m3", lambda x, b: F.matmul_fp8_e4m3(x, qf, sf, b, dt)),
            ("Linear4bit", lambda x, b: m4(x)), ("Linear8bit", lambda x, b: m8(x)),
            ("Linear8bit(use_cache=False)", lambda x, b: m8n(x)), ("LinearFP8", lambda x, b: mf(x))], (m4, m8, m8n, mf)


@pytest.mark.parametrize("lead", [(6,), (2, 3), ()])
def test_gradients_exist_for_every_function_and_module(lead):
    dt, N, K = torch.bfloat16, 256, 128
    cases, modules = _fwd_cases(dt, N=N, K=K)
    for name, fwd in cases:
        if name in ("linear_dense", "Linear4bit", "Linear8bit", "Linear8bit(use_cache=False)", "LinearFP8") and lead == ():
            continue    # 1-D inputs: the functions whose reference counterparts take them (matmul_4bit, matmul_fp8_e4m3, linear_int8)
        x = synthetic.normal(lead + (K,), dt, seed=7).to(DEV).requires_grad_(True)
        bias = synthetic.normal((N,), dt, seed=8).to(DEV).requires_grad_(True)
        y = fwd(x, bias)
        assert y.grad_fn is not None, name
        y.backward(synthetic.normal(tuple(y.shape), y.dtype, seed=9).to(DEV))
        assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype, name
        assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0, name
        if not name[0].isupper():
            assert bias.grad is not None and bias.grad.shape == bias.shape and bias.grad.dtype == bias.dtype, name
    for m in modules if lead != () else ():
        assert m.bias.grad is not None and m.bias.grad.shape == (N,) and m.bias.grad.dtype == dt


def test_linear8bit_cached_branch_has_gradients():
    """Linear8bit's large-batch branch (the cached dequantised weight through linear_dense) and its linear_int8 branch."""
    dt, M, N, K = torch.float16, 512, 4096, 128
    lin = torch.nn.Linear(K, N).to(dt).to(DEV)
    m = bnb.Linear8bit.from_linear(lin)
    assert F.dense_path_applies(M, N, K)
    for rows in (M, 8):
        x = synthetic.normal((rows, K), dt, seed=10).to(DEV).requires_grad_(True)
        y = m(x)
        y.backward(synthetic.normal((rows, N), dt, seed=11).to(DEV))
        assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    assert m._weight_cache is not None and m.bias.grad.shape == (N,)


# --------------------------------------------------------------------- 2. dense shapes: the bits of the library's forward machinery
@pytest.mark.parametrize("M,N,K,dt,qt,cs", [(4096, 4096, 4096, torch.bfloat16, "nf4", False), (1024, 11008, 4096, torch.bfloat16, "nf4", True),
                                            (1024, 4096, 11008, torch.bfloat16, "nf4", False), (512, 4096, 4096, torch.float16, "fp4", False)])
def test_dense_grad_equals_linear_dense_on_the_transposed_weight(M, N, K, dt, qt, cs):
    W, packed, st = _q4(N, K, dt, qt, 64, cs, seed=21)
    x = synthetic.normal_device((M, K), dt, seed=22).requires_grad_(True)
    dY = synthetic.normal_device((M, N), dt, seed=23)
    kern = _backward_kernel(x)
    F.matmul_4bit(x, packed, st).backward(dY)
    assert kern[0].startswith("grad_t+dense"), kern
    want = F.linear_dense(dY, F.dequantize_4bit(packed, st).t().contiguous()).to(x.dtype)
    assert _same_bits(x.grad, want)


@pytest.mark.parametrize("kind", ["int8", "fp8", "cache"])
def test_dense_grad_equals_linear_dense_for_8bit_weights(kind):
    M, N, K, dt = 1024, 4096, 4096, torch.bfloat16
    W = synthetic.normal_device((N, K), dt, seed=31, std=0.05)
    x = synthetic.normal_device((M, K), dt, seed=32).requires_grad_(True)
    dY = synthetic.normal_device((M, N), dt, seed=33)
    kern = _backward_kernel(x)
    if kind == "fp8":
        q, s = F.quantize_fp8_e4m3(W)
        F.matmul_fp8_e4m3(x, q, s, None, dt).backward(dY)
        Wd = F.dequantize_fp8_e4m3(q, s, dt)
    else:
        q, s = F.quantize_rowwise(W)
        Wd = F.dequantize_rowwise(q, s, dt)
        (F.linear_int8(x, q, s) if kind == "int8" else F.linear_dense(x, Wd)).backward(dY)
    assert kern[0].startswith("grad_t+dense"), kern
    assert _same_bits(x.grad, F.linear_dense(dY, Wd.t().contiguous()))


# --------------------------------------------------------------------------------- 3. the transposed pass, bit for bit
@pytest.mark.parametrize("N,K,qt,bs,dt,cs,nan", [(256, 70, "nf4", 64, torch.float16, False, False), (128, 127, "fp4", 32, torch.bfloat16, True, False),
                                                 (100, 127, "nf4", 8, torch.bfloat16, False, True), (4096, 4096, "nf4", 64, torch.bfloat16, True, False),
                                                 (4160, 1000, "fp4", 128, torch.float16, False, True), (72, 4104, "nf4", 256, torch.float16, True, False)])
def test_transposed_pass_equals_dequantize_t(N, K, qt, bs, dt, cs, nan):
    W, packed, st = _q4(N, K, dt, qt, bs, cs, seed=41)
    if nan:     # NaN blocks: a NaN absmax poisons its block in both decoders alike
        st.absmax.view(-1)[3::17] = float("nan")
    Wt = F._dequantize_t(packed, st)
    assert _native.last_kernel() == "grad_t"
    assert _same_bits(Wt, F.dequantize_4bit(packed, st).t().contiguous())


@pytest.mark.parametrize("N,K,dt", [(256, 128, torch.float16), (100, 72, torch.bfloat16), (4096, 4096, torch.bfloat16)])
def test_transposed_pass_equals_dequantize_t_for_8bit_and_dense(N, K, dt):
    W = synthetic.normal_device((N, K), dt, seed=51, std=0.05)
    q, s = F.quantize_rowwise(W)
    assert _same_bits(F._dequantize_t(q, scales=s, fmt="int8", dtype=dt), F.dequantize_rowwise(q, s, dt).t().contiguous())
    qf, sf = F.quantize_fp8_e4m3(W)
    qf.view(-1)[5::97] = 0x7F        # the reference's NaN byte
    qf.view(-1)[7::89] = 0xFF
    assert _same_bits_but_nan_payload(F._dequantize_t(qf, scales=sf, fmt="fp8", dtype=dt), F.dequantize_fp8_e4m3(qf, sf, dt).t().contiguous())
    assert _same_bits(F._dequantize_t(W, fmt="dense"), W.t().contiguous())


# ---------------------------------------------------------------------------------------------- 4. the reference's autograd (g9)
def _g9():
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "manifest_grad.json")) as f:
        cases = json.load(f)["g9"]
    return cases, np.load(os.path.join(here, "g9_grad.npz"))


G9_CASES, G9 = _g9()


@pytest.mark.parametrize("case", G9_CASES, ids=[f"{c['kind']}{c['id']}" for c in G9_CASES])
def test_g9_reference_gradients(case):
    """x.grad and bias.grad of the reference's CPU autograd (tests/golden/make_golden_grad.py), the same synthetic operands."""
    seed, lead, N, K = case["seed"], tuple(case["lead"]), case["N"], case["K"]
    if case["kind"] == "matmul_4bit":
        wdt, tag = DT[case["w_dtype"]], f"m{case['id']}"
        W = synthetic.normal((N, K), wdt, seed=seed, std=0.05)
        bdt = case["bias_dtype"]
        x = synthetic.normal(lead + (K,), DT[case["x_dtype"]], seed=seed + 2).to(DEV).requires_grad_(True)
        cdt = None if case["compute_dtype"] is None else DT[case["compute_dtype"]]
        if case["via"] == "fn":
            packed, st = F.quantize_4bit(W.to(DEV), blocksize=case["blocksize"], compress_statistics=case["compress_statistics"],
                                         quant_type=case["quant_type"])
            bias = None if bdt is None else synthetic.normal((N,), DT[bdt], seed=seed + 1).to(DEV).requires_grad_(True)
            y = F.matmul_4bit(x, packed, st, bias, compute_dtype=cdt)
        else:
            lin = torch.nn.Linear(K, N, bias=True).to(wdt)
            with torch.no_grad():
                lin.weight.copy_(W)
                lin.bias.copy_(synthetic.normal((N,), DT[bdt], seed=seed + 1).to(wdt))
            mod = bnb.Linear4bit.from_linear(lin.to(DEV), compute_dtype=cdt, quant_type=case["quant_type"], blocksize=case["blocksize"],
                                             compress_statistics=case["compress_statistics"])
            bias = mod.bias
            y = mod(x)
        gate = TOL[wdt]
    else:
        dt, tag = DT[case["dtype"]], f"q{case['id']}"
        lin = torch.nn.Linear(K, N, bias=case["bias"])
        with torch.no_grad():
            lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=seed, std=0.05))
            if case["bias"]:
                lin.bias.copy_(synthetic.normal((N,), torch.float32, seed=seed + 1))
        lin = lin.to(dt).to(DEV)
        mod = (bnb.Linear8bit if case["kind"] == "linear8bit" else bnb.LinearFP8).from_linear(lin)
        bias = mod.bias
        x = synthetic.normal(lead + (K,), dt, seed=seed + 2).to(DEV).requires_grad_(True)
        y = mod(x)
        gate = TOL[dt]
    G = synthetic.normal(tuple(y.shape), torch.float32, seed=seed + 3).to(DEV)
    (y.float() * G).sum().backward()
    want = from_bits(G9[f"{tag}_xgrad"], x.dtype).view(x.shape)
    assert x.grad.dtype == want.dtype and x.grad.shape == want.shape
    err = rel_fro(x.grad, want)
    assert err <= gate, f"x.grad rel-err {err:.3e} > {gate:.0e}"
    if bias is not None:
        bwant = from_bits(G9[f"{tag}_bgrad"], bias.dtype)
        assert bias.grad.dtype == bwant.dtype and bias.grad.shape == bwant.shape
        err = rel_fro(bias.grad, bwant)
        assert err <= gate, f"bias.grad rel-err {err:.3e} > {gate:.0e}"


# ---------------------------------------------------------------------------------------------- 5. oracle sweep around the dispatch edges
def _sweep_cases():
    rng = np.random.default_rng(2026)
    Ns = [63, 64, 127, 128, 4032, 4160]
    Ms = [1, 2, 7, 31, 64, 255, 256, 300, 1024, 2048]
    Ks = [65, 127, 128, 200, 333, 512, 1001]
    out = []
    for i in range(40):
        N = Ns[i % len(Ns)]
        M = int(Ms[rng.integers(len(Ms))])
        K = int(Ks[rng.integers(len(Ks))])
        dt = (torch.float16, torch.bfloat16)[i % 2]
        fmt = ("nf4", "fp4", "int8", "nf4", "fp4")[i % 5]
        bs = (32, 64, 128, 16)[(i // 2) % 4]
        if fmt == "int8" and K % 8:
            K += 8 - K % 8
        out.append((i, M, N, K, dt, fmt, bs))
    return out


@pytest.mark.parametrize("i,M,N,K,dt,fmt,bs", _sweep_cases())
def test_grad_oracle_sweep(i, M, N, K, dt, fmt, bs):
    W = synthetic.normal((N, K), dt, seed=600 + i, std=0.05)
    x = synthetic.normal((M, K), dt, seed=700 + i).to(DEV).requires_grad_(True)
    dY = synthetic.normal((M, N), dt, seed=800 + i)
    seen = _backward_kernel(x)
    if fmt == "int8":
        oq, os_ = oracle.quantize_rowwise(W)
        Wd = oracle.dequantize_rowwise(oq, os_, dt)
        y = F.linear_int8(x, oq.to(DEV), os_.to(DEV))
    else:
        op, oa, _ = oracle.quantize_4bit(W, bs, fmt)
        Wd = oracle.dequantize_4bit(op, oa, (N, K), bs, fmt, dt)
        st = F.QuantState(absmax=oa.to(DEV), shape=torch.Size([N, K]), blocksize=bs, quant_type=fmt, dtype=dt)
        y = F.matmul_4bit(x, op.to(DEV), st)
    y.backward(dY.to(DEV))
    kern = seen[0]
    dense = N % 64 == 0 and N >= 128 and (fmt == "int8" or bs >= 32)
    assert kern.startswith("grad_t+dense" if dense else "grad_generic"), (kern, dense)
    rows = torch.arange(0, M, max(1, M // 48))
    ref = (dY[rows].double() @ Wd.double()).to(dt)
    err = rel_fro(x.grad[rows.to(DEV)], ref)
    assert err <= TOL[dt], f"rel-err {err:.3e} ({kern})"


def test_generic_kernel_without_workspace_and_for_f32():
    """No workspace (NULL / 0) is valid and costs speed, never the result; f32 weights always take the generic kernel."""
    N, K, M = 256, 192, 40
    for dt in (torch.bfloat16, torch.float32):
        W, packed, st = _q4(N, K, dt, "nf4", 64, True, seed=61)
        dY = synthetic.normal_device((M, N), dt, seed=62)
        lib = _native.lib()
        keep: list = []
        desc = F._absmax_desc(st.absmax, st.state2, keep)
        code = _native.DTYPE_CODE[dt]
        dX = torch.empty(M, K, dtype=dt, device=DEV)
        assert lib.mbnb_linear_grad_input(dY.data_ptr(), M, N, _native.NF4, packed.data_ptr(), ctypes.byref(desc), None, K, K, 64, code, code,
                                          dX.data_ptr(), None, 0, 0, _native.stream_ptr(DEV)) == 0
        assert _native.last_kernel() == "grad_generic"
        ref = (dY.double() @ F.dequantize_4bit(packed, st).double()).to(dt)
        assert rel_fro(dX, ref) <= TOL[dt]
        if dt == torch.bfloat16:     # with the workspace: the dense path, within the same gate
            x = torch.zeros(M, K, dtype=dt, device=DEV, requires_grad=True)
            kern = _backward_kernel(x)
            F.matmul_4bit(x, packed, st).backward(dY)
            assert kern[0].startswith("grad_t+dense"), kern
            assert rel_fro(x.grad, ref) <= TOL[dt]


# ---------------------------------------------------------------------------------------------- 6. inference unchanged
def test_inference_is_unchanged(monkeypatch):
    dt, N, K = torch.bfloat16, 256, 128
    cases, _ = _fwd_cases(dt, N=N, K=K)
    x0 = synthetic.normal((300, K), dt, seed=71).to(DEV)
    b0 = synthetic.normal((N,), dt, seed=72).to(DEV)
    for name, fwd in cases:
        with torch.no_grad():
            y_ng = fwd(x0, b0)
            assert y_ng.grad_fn is None, name
        with torch.inference_mode():
            assert fwd(x0, b0).grad_fn is None, name
        y_plain = fwd(x0, b0)       # grad mode on, nothing requires grad (the modules' bias Parameters aside)
        y_grad = fwd(x0.clone().requires_grad_(True), b0.clone().requires_grad_(True))
        assert y_grad.grad_fn is not None, name
        assert _same_bits(y_grad.detach(), y_ng) and _same_bits(y_plain.detach(), y_ng), name
    # only the bias requires grad: no dX is computed
    W, packed, st = _q4(N, K, dt, seed=73)
    bias = b0.clone().requires_grad_(True)
    calls = []
    grad_input = F._grad_input
    monkeypatch.setattr(F, "_grad_input", lambda *a: calls.append(a) or grad_input(*a))
    y = F.matmul_4bit(x0, packed, st, bias)
    y.backward(torch.ones_like(y))
    assert calls == [], "dX was computed although the input does not require grad"
    assert x0.grad is None and bias.grad is not None
    F.matmul_4bit(x0.clone().requires_grad_(True), packed, st, bias).backward(torch.ones_like(y))
    assert len(calls) == 1       # the spy sees the dX of an input that requires grad
    assert torch.equal(bias.grad, y.new_full((N,), 600.0).to(dt))


# ---------------------------------------------------------------------------------------------- 7. QLoRA end to end
def test_qlora_two_layers_match_dequantized_nn_linear():
    """Two stacked Linear4bit layers with bf16 LoRA adapters against the same model on nn.Linear holding the dequantised weights
    (torch's own GEMM): every adapter's gradient within 1e-2 relative Frobenius -- the lower adapter's included, which needs dX of the
    upper base layer."""
    dt, M, H, r = torch.bfloat16, 512, 1024, 16
    torch.manual_seed(0)
    bases = []
    for i in range(2):
        lin = torch.nn.Linear(H, H).to(dt).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(synthetic.normal_device((H, H), dt, seed=80 + i, std=0.03))
            lin.bias.copy_(synthetic.normal_device((H,), dt, seed=90 + i, std=0.1))
        bases.append(bnb.Linear4bit.from_linear(lin, quant_type="nf4", blocksize=64, compress_statistics=True))
    refs = []
    for b in bases:
        lin = torch.nn.Linear(H, H).to(dt).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(b.dequantize())
            lin.bias.copy_(b.bias)
        lin.requires_grad_(False)
        b.bias.requires_grad_(False)
        refs.append(lin)

    def adapters():
        return [(synthetic.normal_device((r, H), dt, seed=100 + i, std=0.05).requires_grad_(True),
                 synthetic.normal_device((H, r), dt, seed=110 + i, std=0.05).requires_grad_(True)) for i in range(2)]

    def run(layers, ad):
        h = synthetic.normal_device((M, H), dt, seed=120)
        for layer, (A, B) in zip(layers, ad):
            h = layer(h) + (h @ A.t()) @ B.t()
        (h.float() * synthetic.normal_device((M, H), torch.float32, seed=121)).sum().backward()
        return [t.grad for pair in ad for t in pair]

    got, want = run(bases, adapters()), run(refs, adapters())
    for name, g, w in zip(("A0", "B0", "A1", "B1"), got, want):
        err = rel_fro(g, w)
        assert err <= 1e-2, f"{name}: rel-err {err:.3e}"
