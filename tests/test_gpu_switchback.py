"""
SwitchBackLinear and libmbnb_train.so on the GPU.  Every output and workspace the Python API allocates comes back 0xFF-poisoned
(tests/poison.py), so an element no kernel writes, or a pad column of the weight gradient left unwritten, reads as NaN.

- exact: the Wd pass against the reference's rule (weight_int8.to(T) * (weight_scales[:, None] / 127.0).to(T)) and the goldens; codes and
  scales after from_linear / sync_weights; the bias output == round_T(no-bias output + b) on the same route;
- element by element against float64 (tests/elementwise.py): every case of tests/switchback_cases.py, dX and db through autograd;
- goldens of the reference's CPU path (tests/golden/g11_switchback.npz) within the project's tolerances; a training loop.
"""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _train_native, synthetic
from mps_bitsandbytes_amd import functional as F
from mps_bitsandbytes_amd.optim import AdamW8bit
from tests import forms, guard, switchback_cases
from tests.forms import memo as _memo
from tests.elementwise import UNIT, assert_bound_elementwise, assert_linear_elementwise
from tests.goldenio import DT, HERE, from_bits, rel_fro
from tests.guard import guarded_alloc  # noqa: F401  (the fixture, by name: it replaces poisoned_alloc's proxy in the tests that ask for it)
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name: every torch.empty of functional.py comes back 0xFF)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"


def _wd_rule(q, s, T):
    """The reference's forward weight, computed by torch on the tensors given (SwitchBackFunction.forward)."""
    return q.to(T) * (s.unsqueeze(1) / 127.0).to(T)


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _nan_bits(t):
    """_bits with every NaN as the dtype's default NaN: the contract says where a NaN is, not which one."""
    t = t.detach().cpu()
    return _bits(torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t))


def _weights(N, K, seed):
    W = synthetic.normal((N, K), torch.float32, seed=seed, std=0.02)
    q, s = F.quantize_rowwise(W.to(DEV))
    return q, s


# ----------------------------------------------------------------------------- every case of the table
_SENTINEL = {}


def _sentinel(case):
    """A call of the library's other entry point, on a generic kernel that sets no variant: the case's own name and variant cannot be
    left over from the call before."""
    if not _SENTINEL:
        _SENTINEL["x"] = torch.ones(3, 8, device=DEV)
        _SENTINEL["q"] = torch.ones(5, 8, dtype=torch.int8, device=DEV)
        _SENTINEL["s"] = torch.ones(5, device=DEV)
    if case["op"] in ("forward", "dequant"):
        F._linear_grad_weight(_SENTINEL["x"], _SENTINEL["x"])
        name = "grad_w_generic"
    else:
        F._switchback_forward(_SENTINEL["x"], _SENTINEL["q"], _SENTINEL["s"])
        name = "switchback_generic"
    assert _train_native.last_kernel() == name
    assert _train_native.last_variant() == "", "a call whose launcher sets no variant reports the previous call's"


def _Run(case, proxy=None, fill=None):
    return forms.Run(switchback_cases, _train_native, _sentinel, case, proxy, fill)


def _case_weights(case, N, K, seed):
    """(codes, scales) on the device; the larger weights of the FORMS cases are drawn on the device."""
    if N * K <= 1 << 23 or not any(case is c for c in switchback_cases.FORMS):
        return _weights(N, K, seed)
    return F.quantize_rowwise(synthetic.normal_device((N, K), torch.float32, seed=seed, std=0.02, device=DEV))


def _run_case(case, proxy=None, fill=None):
    T = DT[case["dt"]]
    K, seed = case["K"], 1500 + case["K"] % 97
    flags = _train_native.FORCE_GENERIC if case.get("generic") else 0
    lead = tuple(case["lead"]) if "lead" in case else (case.get("M", 0),)
    run = _Run(case, proxy, fill)
    nonfinite = case.get("special") == "nonfinite"
    if case["op"] == "dequant":
        q, s = _case_weights(case, case["N"], K, seed)
        if nonfinite:
            s[3], s[5], s[7] = float("nan"), float("inf"), float("-inf")
            q[5, 2] = 0          # 0 * Inf
        want = _memo(("wd", run.id), lambda: _nan_bits(_wd_rule(q.cpu(), s.cpu(), T)))
        run.begin()
        wd = F._switchback_dequant(run.put("w", q), s, T)
        run.end()
        assert torch.equal(_nan_bits(wd), want)
        if nonfinite:
            assert bool(torch.isnan(wd[3]).all()) and bool(torch.isnan(wd[5, 2])) and bool(torch.isinf(wd[7, q[7] != 0]).all())
        return
    if case["op"] == "transpose":
        M = case["M"]
        x = synthetic.normal((M, K), T, seed=seed).to(DEV)
        run.begin()
        x = run.put("x", x)
        xt = F._transpose_pad(x)
        run.end()
        Mp = _train_native.padded_rows(M)
        assert Mp == switchback_cases.padded_rows(M) and xt.shape == (K, Mp)
        assert torch.equal(_bits(xt[:, :M]), _bits(x.t()))
        assert not bool(_bits(xt[:, M:]).any()), "pad columns must be written as zeros"
        return
    if case["op"] == "forward":
        N = case["N"]
        q, s = _case_weights(case, N, K, seed)
        x = synthetic.normal(lead + (K,), T, seed=seed + 1, std=1.0).to(DEV)
        b = synthetic.normal((N,), T, seed=seed + 2).to(DEV) if case.get("bias") else None
        if nonfinite:
            s[3], s[5], s[7] = float("nan"), float("inf"), float("-inf")
            x[2, 9], x[4, 11], x[6, 13] = float("nan"), float("inf"), float("-inf")
        wd = _memo(("fwd", run.id), lambda: _wd_rule(q.cpu(), s.cpu(), T))
        run.begin()
        x, q, b = run.put("x", x), run.put("w", q), run.put("bias", b)
        y0 = F._switchback_forward(x, q, s, None, flags)
        if b is None:
            run.end()
        else:           # the bias-free call of a case with a bias: its own name and variant, by the restated conditions
            got = (_train_native.last_kernel(), _train_native.last_variant())
            assert got == switchback_cases.model(dict(case, bias=False)), f"{run.id} without its bias: the library reports {got}"
        assert y0.shape == lead + (N,) and y0.dtype == T
        assert_linear_elementwise(y0, x.cpu(), wd, None, T, T, case["kernel"])
        if b is not None:
            _sentinel(case)             # so that the second call's name cannot be the first one's
            if proxy is not None:       # the second call's allocations: the same plan again
                proxy.plan = run.plan()
            y = F._switchback_forward(x, q, s, b, flags)
            run.end()
            assert torch.equal(_nan_bits(y), _nan_bits(y0 + b)), "the bias is one more rounding of the bias-free product"
        return
    # grad_w: dW = dY^T . X, checked as y = X' . Wd'^T with X' = dY^T [N, M], Wd' = X^T [K, M]
    N = case["N"]
    dy = synthetic.normal(lead + (N,), T, seed=seed + 3).to(DEV)
    x = synthetic.normal(lead + (K,), T, seed=seed + 4).to(DEV)
    run.begin()
    dy, x = run.put("dy", dy), run.put("x", x)
    dW = F._linear_grad_weight(dy, x, flags)
    run.end()
    assert dW.shape == (N, K) and dW.dtype == T
    assert_linear_elementwise(dW, dy.reshape(-1, N).t().cpu(), x.reshape(-1, K).t().cpu(), None, T, T, case["kernel"])


@pytest.mark.parametrize("case", [c for c in switchback_cases.CASES if not switchback_cases.needs_plan(c)], ids=switchback_cases.case_id)
def test_case_elementwise(case):
    _run_case(case)


# every case that launches no GEMM again, inside guard bands and under two fills (tests/guard.py): an element the kernel never wrote holds
# the fill and cannot equal the reference under both; a store outside a buffer changes a band.  The cases that place one of functional.py's
# own allocations off its alignment run here only.
@pytest.mark.parametrize("fill", guard.FILLS, ids=lambda f: f"fill{f:02X}")
@pytest.mark.parametrize("case", [c for c in switchback_cases.CASES if not switchback_cases.launches_gemm(c)], ids=switchback_cases.case_id)
def test_case_guarded(case, fill, guarded_alloc):
    _run_case(case, guarded_alloc, fill)
    assert guarded_alloc.allocs, "nothing went through the guarded proxy"


def test_grad_weight_of_no_tokens_is_zero():
    for T in (torch.bfloat16, torch.float32):
        dW = F.linear_grad_weight(torch.empty(0, 1024, dtype=T, device=DEV), torch.empty(0, 2048, dtype=T, device=DEV))
        assert dW.shape == (1024, 2048) and not bool(dW.any())


def test_forward_same_bits_with_and_without_grad_mode():
    m = bnb.SwitchBackLinear.from_linear(torch.nn.Linear(512, 3072).to(torch.bfloat16).to(DEV))
    for M in (1, 512):
        x = synthetic.normal((M, 512), torch.bfloat16, seed=7 + M).to(DEV)
        y_grad = m(x.clone().requires_grad_(True))
        with torch.no_grad():
            y_nograd = m(x)
        assert torch.equal(_bits(y_grad), _bits(y_nograd))


# ----------------------------------------------------------------------------- module: exact buffers, gradients
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_from_linear_and_sync_weights_exact(dt):
    lin = torch.nn.Linear(1000, 300).to(DT[dt])
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((300, 1000), torch.float32, seed=31, std=0.02))
    m = bnb.SwitchBackLinear.from_linear(lin, device=DEV)
    w = lin.weight.data
    s_ref = w.float().abs().max(dim=-1).values.clamp(min=1e-8)
    q_ref = torch.clamp(torch.round(w.float() * (127.0 / s_ref.unsqueeze(-1))), -127, 127).to(torch.int8)
    assert torch.equal(m.weight_int8.cpu(), q_ref) and torch.equal(_bits(m.weight_scales), _bits(s_ref))
    with torch.no_grad():
        m.weight_fp.mul_(1.5)
    m.sync_weights()
    wf = m.weight_fp.data.cpu()
    s2 = wf.float().abs().max(dim=-1).values.clamp(min=1e-8)
    q2 = torch.clamp(torch.round(wf.float() * (127.0 / s2.unsqueeze(-1))), -127, 127).to(torch.int8)
    assert torch.equal(m.weight_int8.cpu(), q2) and torch.equal(_bits(m.weight_scales), _bits(s2))


@pytest.mark.parametrize("M,N,K,dt", [(7, 40, 100, "f16"), (512, 3072, 512, "bf16"), (1, 4096, 1024, "f16"), (300, 1024, 2048, "bf16")])
def test_autograd_gradients_elementwise(M, N, K, dt):
    """dX = dY . weight_fp, dW = dY^T . X, db = sum of dY over rows, from loss.backward()."""
    T = DT[dt]
    lin = torch.nn.Linear(K, N).to(T)
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=41, std=0.02))
        lin.bias.copy_(synthetic.normal((N,), torch.float32, seed=42))
    m = bnb.SwitchBackLinear.from_linear(lin, device=DEV)
    x = synthetic.normal((M, K), T, seed=43).to(DEV).requires_grad_(True)
    G = synthetic.normal((M, N), T, seed=44).to(DEV)
    y = m(x)
    y.backward(G)
    wfp = m.weight_fp.detach().cpu()
    assert x.grad.dtype == T and m.weight_fp.grad.dtype == T and m.bias.grad.dtype == T
    assert_linear_elementwise(x.grad, G.cpu(), wfp.t().contiguous(), None, T, T, "dX")
    assert_linear_elementwise(m.weight_fp.grad, G.cpu().t(), x.detach().cpu().t(), None, T, T, "dW")
    r = G.cpu().double().sum(0)
    bound = (M + 2) * 2.0 ** -23 * G.cpu().double().abs().sum(0) + UNIT[T] * r.abs() + 2.0 ** -24
    assert_bound_elementwise(m.bias.grad, r, bound, "db", "db = sum dY")
    assert m.weight_int8.grad is None and m.weight_scales.grad is None


def test_mixed_dtypes_raise_in_backward_as_the_reference():
    m = bnb.SwitchBackLinear.from_linear(torch.nn.Linear(64, 32).half(), device=DEV)
    x = synthetic.normal((4, 64), torch.bfloat16, seed=5).to(DEV).requires_grad_(True)
    y = m(x)                                   # bf16 product + f16 bias: torch promotes to f32, as the reference's forward does
    assert y.dtype == torch.float32
    with pytest.raises(RuntimeError, match="same dtype"):
        y.sum().backward()
    x32 = synthetic.normal((4, 64), torch.float32, seed=6).to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="same dtype"):
        m(x32).sum().backward()


# ----------------------------------------------------------------------------- goldens of the reference's CPU path
def _golden():
    import json
    import os
    with open(os.path.join(HERE, "manifest_switchback.json")) as f:
        man = json.load(f)["g11"]
    return man, np.load(os.path.join(HERE, "g11_switchback.npz"))


def _linear(N, K, dt, has_bias, seed):
    lin = torch.nn.Linear(K, N, bias=has_bias)
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=seed, std=0.05))
        if has_bias:
            lin.bias.copy_(synthetic.normal((N,), torch.float32, seed=seed + 1))
    return lin.to(DT[dt])


def test_golden_from_linear_and_wd_bits():
    man, z = _golden()
    for c in (c for c in man if c["kind"] == "from_linear"):
        i = c["id"]
        m = bnb.SwitchBackLinear.from_linear(_linear(c["N"], c["K"], c["dtype"], True, c["seed"]), device=DEV)
        assert m.compute_dtype == DT[c["compute_dtype"]]
        assert torch.equal(m.weight_int8.cpu(), torch.from_numpy(z[f"fl{i}_q"]))
        assert torch.equal(_bits(m.weight_scales), torch.from_numpy(z[f"fl{i}_s"].view(np.int32)))
        for t in ("f16", "bf16", "f32"):
            wd = F._switchback_dequant(m.weight_int8, m.weight_scales, DT[t])
            assert torch.equal(_bits(wd), _bits(from_bits(z[f"fl{i}_wd_{t}"], DT[t]))), (i, t)


def test_golden_forward_and_gradients():
    man, z = _golden()
    tol = {"f16": 2e-3, "bf16": 1e-2}
    for c in (c for c in man if c["kind"] == "forward_backward"):
        i, N, K, T = c["id"], c["N"], c["K"], DT[c["dtype"]]
        m = bnb.SwitchBackLinear.from_linear(_linear(N, K, c["dtype"], c["bias"], c["seed"]), device=DEV)
        x = synthetic.normal(tuple(c["lead"]) + (K,), T, seed=c["seed"] + 2).to(DEV).requires_grad_(True)
        y = m(x)
        G = synthetic.normal(tuple(y.shape), torch.float32, seed=c["seed"] + 3).to(DEV)
        (y.float() * G).sum().backward()
        yr, wr = c["y_rows"], c["wgrad_rows"]
        y2, xg = y.detach().reshape(-1, N), x.grad.reshape(-1, K)
        pairs = [("y", y2 if yr is None else y2[yr]), ("xgrad", xg if yr is None else xg[yr]),
                 ("wgrad", m.weight_fp.grad if wr is None else m.weight_fp.grad[wr])]
        if c["bias"]:
            pairs.append(("bgrad", m.bias.grad))
        for name, got in pairs:
            want = from_bits(z[f"fb{i}_{name}"], T).reshape(got.shape)
            err = rel_fro(got, want)
            assert err < tol[c["dtype"]], (i, name, err)


def test_golden_training_loop_and_loss_falls():
    """Three SGD steps with SwitchBackLinearCallback.sync() after each: the reference's weights, codes and losses within tolerance."""
    man, z = _golden()
    c = next(c for c in man if c["kind"] == "loop")
    m = bnb.SwitchBackLinear.from_linear(_linear(c["N"], c["K"], "f16", True, c["seed"]), device=DEV)
    m.train()
    cb = bnb.SwitchBackLinearCallback(m)
    opt = torch.optim.SGD([m.weight_fp, m.bias], lr=c["lr"])
    x = synthetic.normal((c["M"], c["K"]), torch.float16, seed=c["seed"] + 2).to(DEV)
    target = synthetic.normal((c["M"], c["N"]), torch.float16, seed=c["seed"] + 3).to(DEV)
    losses = []
    for step in range(c["steps"]):
        opt.zero_grad()
        loss = ((m(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        cb.sync()
        losses.append(float(loss.detach()))
        wfp = from_bits(z[f"loop{step}_wfp"], torch.float16)
        assert rel_fro(m.weight_fp, wfp) < 1e-3, step
        dq = (m.weight_int8.cpu().int() - torch.from_numpy(z[f"loop{step}_q"]).int()).abs()
        assert int(dq.max()) <= 1 and float((dq > 0).float().mean()) < 0.01, step
    want = from_bits(z["loop_loss"], torch.float16).float()
    assert np.allclose(losses, want.numpy(), rtol=2e-3)
    assert losses[-1] < losses[0]


def test_training_with_adamw8bit_loss_falls():
    torch.manual_seed(0)
    lin = torch.nn.Linear(256, 128).to(torch.bfloat16)
    m = bnb.SwitchBackLinear.from_linear(lin, device=DEV)
    m.train()
    cb = bnb.SwitchBackLinearCallback(m)
    opt = AdamW8bit([m.weight_fp, m.bias], lr=5e-3)
    x = synthetic.normal((64, 256), torch.bfloat16, seed=61).to(DEV)
    target = synthetic.normal((64, 128), torch.bfloat16, seed=62).to(DEV)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((m(x).float() - target.float()) ** 2).mean()
        loss.backward()
        opt.step()
        cb.sync()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0], losses
