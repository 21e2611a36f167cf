"""
Non-finite inputs at every special place of the contraction, on every GEMM-family kernel, element by element.

The cases are those of tests/kernel_cases.py and tests/gemm_variant_cases.py, run by the builders of tests/test_gpu_elementwise.py on
poisoned allocations; the plan is tests/nonfinite.py (held on the host by tests/test_nonfinite_host.py).

Activations.  Every case whose op is fed a floating activation -- matmul_4bit, linear_int8, matmul_fp8, linear_dense, mbnb_gemm_dense,
and the input gradient, whose "activation" is dY and whose contraction runs over N -- runs once per planting pass: the weight, its
oracle decode and the bias are built once, only the activation changes (the planted values replace elements after the case's own
scaling; the three plants of a `bad="x"` case are left to tests/test_gpu_elementwise.py).  Each pass must dispatch to the case's
kernel name and variant (the plant did not change the path), and assert_linear_elementwise holds every element: NaN, +Inf and -Inf
exactly where the operands put them (an Inf times an exact-zero decoded weight is a NaN; an Inf in a row leaves every other row
alone), every finite element within the bound of tests/elementwise.py.  No tolerance is introduced here.

Weights.  Every 4-bit case runs with a NaN absmax in block 0 of row 0 and again with one in the last block of row N - 1 (a nested
absmax: a NaN in the first and in the last group of absmax2, the expected weight being the oracle's decode of the same state); every
int8 case with a NaN row scale at row 0 and at row N - 1; every FP8 case with byte 0x7F at [0, 0] and at [N - 1, K - 1]; matmul_int8
with a NaN in A_scales at rows 0 and M - 1 and in B_scales at columns N - 1 and 0.  These are the blocks that a clamped chunk, a
clamped dead row or a padded tile re-reads: every other row and column must stay within its bound.  The transposed dequantise pass
(grad_t) has no activation and takes the weight plants only.

Left out: outlier_linear and the embeddings.  outlier_linear quantises its activation row-wise to int8 before any kernel of this
family sees it, and the conversion of a NaN (or of Inf / Inf) to int8 is platform-defined; the embeddings have an
integer index for an activation.  matmul_int8's operands are integers: only its scales can be non-finite.
"""
import time

import pytest
import torch

from mps_bitsandbytes_amd import synthetic
from mps_bitsandbytes_amd import functional as F
from tests import gemm_variant_cases, kernel_cases, nonfinite
from tests.elementwise import assert_linear_elementwise
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name)
from tests.test_gpu_elementwise import (DEV, DT, KIND, _activation, _backward, _bias, _forward, _gemm_dense_operands, _launch,
                                        _quantized, _run_matmul_int8, _same_bits, _state_4bit, _state_8bit)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

NAN = float("nan")
CASES = [c for c in kernel_cases.CASES + gemm_variant_cases.CASES
         if c["op"] in nonfinite.ACTIVATION_OPS or c["op"] in nonfinite.WEIGHT_OPS]


def _without_x(c):
    """The case without the three activation plants of bad="x" (a pass plants one value per row)."""
    c = dict(c)
    bad = c.pop("bad", "").replace("x", "")
    if bad:
        c["bad"] = bad
    return c


class _Planter:
    """The activation X of a case ([..., L], perhaps a view into a larger buffer) and its planting passes, applied in place."""

    def __init__(self, X, L):
        self.X2 = X.view(-1, L)
        assert self.X2.data_ptr() == X.data_ptr()
        self.x0 = self.X2.clone()

    def plant(self, one):
        self.X2.copy_(self.x0)
        for r, k, v in one:
            self.X2[r, k] = v

    def restore(self):
        self.X2.copy_(self.x0)


def _weight_plants(kind, quant, N, K):
    """The planted quantisations of a weight: [(what, quant)]."""
    out = []
    if kind == "4bit":
        op, oa, ost2 = quant
        for what, i in (("first", 0), ("last", -1)):
            if ost2 is None:
                a = oa.clone()
                a[i] = NAN
                out.append((f"a NaN absmax in the {what} block", (op, a, None)))
            else:
                a2 = ost2[0].clone()
                a2[i] = NAN
                out.append((f"a NaN absmax2 in the {what} group", (op, oa, (a2, ost2[1]))))
    elif kind == "int8":
        q, s = quant
        for what, i in (("first", 0), ("last", N - 1)):
            s2 = s.clone()
            s2[i] = NAN
            out.append((f"a NaN scale of the {what} row", (q, s2)))
    else:
        q, s = quant
        for what, (i, k) in (("first", (0, 0)), ("last", (N - 1, K - 1))):
            q2 = q.clone()
            q2.view(N, K)[i, k] = 0x7F
            out.append((f"FP8 byte 0x7F in the {what} element", (q2, s)))
    return out


def _linear_parts(c, monkeypatch):
    """(pl, check, weights): the activation's planter, check(Wd, fwd, what) -> max ratio of one launch on the activation as it
    stands, and weights(plant or None) -> (Wd, fwd)."""
    op, N, K, dt = c["op"], c["N"], c["K"], DT[c["dt"]]
    if c.get("fused"):
        monkeypatch.setattr(F, "DECODE_ONCE", False)
    out = DT.get(c.get("out"))
    if op == "gemm_dense":
        X, Wfull, b, call = _gemm_dense_operands(c)

        def check(Wd, fwd, what):
            y, kern = _launch(c, call)
            return assert_linear_elementwise(y, X, Wfull[:, :K], b, dt, DT[c.get("out", c["dt"])], f"{kern}, {what}")
        return _Planter(X, K), check, None, None
    X = _activation(c, K, dt, seed=11)
    b = _bias(c, N, dt, seed=12)

    def check(Wd, fwd, what):
        y, kern = _launch(c, lambda: fwd(X, b, out))
        return assert_linear_elementwise(y, X, Wd, b, dt, out or dt, f"{kern}, {what}")
    if op == "linear_dense":
        Wd = synthetic.normal_device((N, K), dt, seed=13, std=0.05)
        return _Planter(X, K), check, (Wd, lambda X, b=None, out=None: F.linear_dense(X, Wd, b)), None
    kind = KIND[op]
    quant = _quantized(c, kind, N, K, dt, seed=13)
    return _Planter(X, K), check, _forward(c, kind, N, K, dt, quant), [(w, lambda q=q: _forward(c, kind, N, K, dt, q))
                                                                   for w, q in _weight_plants(kind, quant, N, K)]


def _grad_parts(c):
    M, N, K, dt, fmt = c["M"], c["N"], c["K"], DT[c["dt"]], c["fmt"]
    quant = _quantized(c, fmt, N, K, dt, seed=41)
    x = synthetic.normal_device((M, K), dt, seed=42)
    dY = _activation(dict(c, M=M), N, dt, seed=43)

    def check(Wd, fwd, what):
        dx, kern = _backward(c, fwd, x, dY)
        return assert_linear_elementwise(dx, dY, Wd.t().contiguous().to(DEV), None, dt, dt, f"{kern}, {what}")
    return _Planter(dY, N), check, _forward(c, fmt, N, K, dt, quant), [(w, lambda q=q: _forward(c, fmt, N, K, dt, q))
                                                                     for w, q in _weight_plants(fmt, quant, N, K)]


def _grad_t(c, errors):
    """The transposed dequantise pass under the weight plants: bit for bit the oracle's decode, transposed."""
    N, K, dt, fmt = c["N"], c["K"], DT[c["dt"]], c["fmt"]
    runs = 0
    for what, q in _weight_plants(fmt, _quantized(c, fmt, N, K, dt, seed=51), N, K):
        if fmt == "4bit":
            packed, st, Wd = _state_4bit(c, N, K, dt, *q)
            Wt, kern = _launch(c, lambda: F._dequantize_t(packed, st))
        else:
            qd, sd, Wd = _state_8bit(c, dt, fmt == "fp8", *q)
            Wt, kern = _launch(c, lambda: F._dequantize_t(qd, scales=sd, fmt=fmt, dtype=dt))
        runs += 1
        if not _same_bits(Wt, Wd.t().contiguous()):
            errors.append(f"{kern}, {what}: the transposed pass differs from the oracle's decode")
    return runs


def _describe(one):
    return "X" + ", ".join(f"[{r}, {k}] = {v}" for r, k, v in one)


@pytest.mark.parametrize("case", CASES, ids=[kernel_cases.case_id(c) for c in CASES])
def test_nonfinite_case(case, monkeypatch, poisoned_alloc):
    t0 = time.perf_counter()
    c = _without_x(case)
    op = c["op"]
    errors, worst, n_act, n_w = [], 0.0, 0, 0
    if op == "matmul_int8":
        M, N = c["M"], c["N"]
        for what, plant in (("A_scales[0], B_scales[N - 1]", lambda sa, sb: (sa.__setitem__(0, NAN), sb.__setitem__(N - 1, NAN))),
                            ("A_scales[M - 1], B_scales[0]", lambda sa, sb: (sa.__setitem__(M - 1, NAN), sb.__setitem__(0, NAN)))):
            try:
                worst = max(worst, _run_matmul_int8(c, plant)[1])
            except AssertionError as e:
                errors.append(f"NaN in {what}: {e}")
            n_w += 1
    elif op == "grad_t":
        n_w = _grad_t(c, errors)
    else:
        pl, check, base, planted = _grad_parts(c) if op == "grad" else _linear_parts(c, monkeypatch)
        Wd, fwd = base if base is not None else (None, None)
        for one in nonfinite.case_passes(c):
            pl.plant(one)
            try:
                worst = max(worst, check(Wd, fwd, _describe(one)))
            except AssertionError as e:
                errors.append(str(e))
            n_act += 1
        pl.restore()
        del Wd, fwd, base
        for what, make in planted or ():
            Wd, fwd = make()
            try:
                worst = max(worst, check(Wd, fwd, what))
            except AssertionError as e:
                errors.append(str(e))
            n_w += 1
            del Wd, fwd
    assert poisoned_alloc.poisoned > 0
    torch.cuda.synchronize()
    print(f"\nnonfinite {kernel_cases.case_id(case)}: {n_act} activation passes, {n_w} weight plants, max err / bound {worst:.3g}, "
          f"{time.perf_counter() - t0:.2f} s")
    assert not errors, f"{len(errors)} of {n_act + n_w} runs fail:\n" + "\n".join(errors[:6])
