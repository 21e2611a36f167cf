"""The numpy emulation of the 8-bit optimizer step (tests/optim_emul.py), without a GPU: it reproduces the reference's CPU optimizers
on both committed fixtures when chained from its own state, its comparator fails on every kind of single-bit departure, the case
table of tests/optim_cases.py reaches all 50 kernel instantiations, and the inputs meet the conditions the GPU tests rely on
(finite values, rounding ties, subnormal second moments, the fixture's size)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from mps_bitsandbytes_amd import synthetic
from tests import optim_cases, optim_data
from tests import optim_emul as emul
from tests.goldenio import DT, HERE, from_bits

NAME = {v: k for k, v in DT.items()}
USED = {}          # test id -> (elements that used the f32-Adam exception, elements that used the SGD-tail exception)


def _manifest(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


def _check_against_golden(tag, e, z, prefix, keys, rule, used):
    """One parameter after one step: codes and maxima bit-equal; the parameter bit-equal except for the two documented places
    where torch's CPU path is not consistent with itself, gated exactly as test_gpu_optim.test_golden_step_by_step gates them."""
    want_p = from_bits(z[prefix], DT[e.pdt]).flatten()
    d = np.abs(emul.bits(e.p).astype(np.int64) - emul.bits(want_p).astype(np.int64))
    n = d.size
    if rule in ("adam", "adamw") and e.pdt == "f32":
        assert int(d.max()) <= 1, f"{tag}: f32 Adam parameter {int(d.max())} ulp from the golden"
        used[0] += int((d != 0).sum())
    elif rule in ("sgd", "sgd_nesterov") and e.pdt != "f32":
        tail = n % 64
        assert n <= tail or int(d[:n - tail].max()) == 0, f"{tag}: vectorised part differs"
        assert int(d.max()) <= 1, f"{tag}: tail {int(d.max())} ulp"
        used[1] += int((d != 0).sum())
    else:
        emul.compare(tag, dict(p=e.p), dict(p=want_p), e.bs, e.pdt, e.before)
    want = dict(zip(("q1", "a1", "q2", "a2"), (from_bits(z[f"{prefix}_{k}"], torch.float32).flatten().numpy() for k in keys)))
    got = {k: v for k, v in e.result().items() if k != "p"}
    emul.compare(tag, got, want, e.bs, e.pdt, e.before)
    if d.max() != 0:           # the two exceptions must not compound: such a case restarts the PARAMETER from the golden
        e.p = want_p.clone()


def _g10_cases():
    return [c["id"] for c in _manifest("manifest_optim.json")["g10"]]


@pytest.mark.parametrize("cid", _g10_cases())
def test_emulation_reproduces_g10_chained(cid, capsys):
    """Every case of g10_optim.npz, chained: the emulation steps from its OWN codes and maxima, never from the golden's, and
    parameters, codes and maxima are the reference's bits after every step.  The two documented exceptions are gated
    as test_golden_step_by_step gates them -- f32 parameters under Adam <= 1 ulp, SGD's 16-bit parameters <= 1 ulp in the last
    numel % 64 elements -- and a parameter that used one is restarted from the golden for the next step, so that an exception
    cannot compound past 1 ulp (Adam's L2 decay and SGD's weight decay feed the parameter back into the moments).  The state is
    never restarted.  The max_grad_norm case clips with the same torch CPU op the reference called."""
    man = _manifest("manifest_optim.json")
    z = np.load(os.path.join(HERE, "g10_optim.npz"))
    case = man["g10"][cid]
    keys = man["state_keys"][case["opt"]]
    kw = dict(case["kwargs"])
    rule = "sgd_nesterov" if kw.get("nesterov") else case["opt"]
    defaults = {"adam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), "adamw": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
                "lion": dict(betas=(0.9, 0.99), weight_decay=0.0), "sgd": dict(dampening=0.0, weight_decay=0.0)}[case["opt"]]
    hp = {**defaults, **kw}
    pdt, gdt = DT[case["param_dtype"]], DT[case["grad_dtype"]]
    shapes, seed = [tuple(s) for s in case["shapes"]], case["seed"]
    es = [emul.EmuTensor(rule, hp, synthetic.normal(shp, pdt, seed=seed + 100 * j), hp.get("block_size", 256)) for j, shp in enumerate(shapes)]
    used = [0, 0]
    for s in range(1, case["steps"] + 1):
        grads = [None if s in case["none_steps"][j] else synthetic.normal(shapes[j], gdt, seed=seed + 100 * j + s) for j in range(len(shapes))]
        if hp.get("max_grad_norm") is not None:
            holders = [torch.nn.Parameter(torch.zeros(shp, dtype=pdt)) for shp in shapes]
            for h, g in zip(holders, grads):
                h.grad_dtype = None
                h.grad = g
            torch.nn.utils.clip_grad_norm_([h for h in holders if h.grad is not None], hp["max_grad_norm"])
            grads = [h.grad for h in holders]
        for j, (e, g) in enumerate(zip(es, grads)):
            if g is None:
                continue
            e.step(g)
            _check_against_golden(f"g10 case {cid} param {j} step {s}", e, z, f"c{cid}_p{j}_s{s}", keys, rule, used)
    USED[f"g10-{cid}"] = tuple(used)
    with capsys.disabled():
        print(f"\n  g10 case {cid}: {used[0]} elements used the f32-Adam exception, {used[1]} the SGD-tail exception", end="")


def _edge_params():
    return [pytest.param(c, id=optim_cases.case_id(c), marks=[pytest.mark.xfail(strict=True, reason=c["ref_xfail"])] if c.get("ref_xfail") else [])
            for c in optim_cases.EDGES]


@pytest.mark.parametrize("c", _edge_params())
def test_emulation_reproduces_g13_edges_chained(c, capsys):
    """Every case of g13_optim_edges.npz, chained from the emulation's own state, under the same rule as the g10 test above: bit-equal
    parameters, codes and maxima, the two documented exceptions gated at <= 1 ulp, a parameter that used one restarted from the
    golden for the next step.  A case with `ref_xfail` is a further place where torch's CPU path departs from its own arithmetic
    (DESIGN.md §10 lists it); it runs as a strict xfail, with no tolerance."""
    man = _manifest("manifest_optim_edges.json")
    z = np.load(os.path.join(HERE, "g13_optim_edges.npz"))
    keys = man["state_keys"][c["rule"]]
    es = optim_data.emulation(c)
    used = [0, 0]
    for s in range(1, c["steps"] + 1):
        if s in c.get("set_step", {}):
            for e in es:
                e.step_count = c["set_step"][s]
        for j, (e, g) in enumerate(zip(es, optim_data.step_grads(c, s))):
            if g is None:
                continue
            assert bool(torch.isfinite(g).all())
            e.step(g)
            _check_against_golden(f"g13 {optim_cases.case_id(c)} param {j} step {s}", e, z, f"e{c['edge']}_p{j}_s{s}", keys, c["rule"], used)
    with capsys.disabled():
        print(f"\n  g13 edge {c['edge']}: {used[0]} elements used the f32-Adam exception, {used[1]} the SGD-tail exception", end="")


def test_edges_fixture_is_small_and_matches_the_table():
    assert os.path.getsize(os.path.join(HERE, "g13_optim_edges.npz")) < (1 << 20)
    man = _manifest("manifest_optim_edges.json")
    assert [m["id"] for m in man["g13"]] == [optim_cases.case_id(c) for c in optim_cases.EDGES]
    assert [m["seed"] for m in man["g13"]] == [c["seed"] for c in optim_cases.EDGES]


def test_edges_cover_what_they_must():
    """The fixture's cases: all five rules on (bf16, f32); block sizes 1, 300, 2048 and one above numel; a zero block and a
    constant-tiny block; subnormal second moments; f16 near the top; Adam at steps 1000 and 10^6; two groups; None steps; 6 steps."""
    E = optim_cases.EDGES
    assert {c["rule"] for c in E if (c["pdt"], c["gdt"]) == ("bf16", "f32")} == set(optim_cases.RULES)
    sizes = {optim_cases.block_size_of(c, j) for c in E for j in range(len(c["shapes"]))}
    assert {1, 300, 2048} <= sizes
    assert any(optim_cases.block_size_of(c, 0) > optim_data.numel_of(c["shapes"][0]) for c in E)
    assert any(c["steps"] == 6 for c in E) and any(c.get("none_steps") for c in E) and any(c.get("group_kwargs") for c in E)
    assert any(sorted(c.get("set_step", {}).values()) == [999, 10 ** 6 - 1] for c in E)
    c = next(c for c in E if c.get("data") == "binades" and c.get("holes", True))
    g = optim_data.grad(c, 0, 1, optim_cases.block_size_of(c, 0)).flatten().float()
    bs = optim_cases.block_size_of(c, 0)
    assert bool((g[bs:2 * bs] == 0).all()) and bool((g[2 * bs:3 * bs] == 2.0 ** c["grange"][0]).all())
    top = next(c for c in E if c.get("data") == "top")
    assert top["pdt"] == "f16" and float(optim_data.param(top, 0).abs().float().min()) > 2.0e4
    # the subnormal case: after the rule, before requantisation, every second moment is a non-zero f32 subnormal
    sub = next(c for c in E if c.get("holes") is False)
    g = optim_data.grad(sub, 0, 1).flatten().float().numpy()
    s = emul.host_scalars("adamw", sub["kwargs"], 1, "f32", "f32")
    v = emul.fma(s.omb2 * g, g, np.zeros_like(g))
    tiny = np.finfo(np.float32).tiny
    assert int(((v > 0) & (v < tiny)).sum()) > 0.9 * v.size, int(((v > 0) & (v < tiny)).sum())


def test_all_inputs_are_finite():
    for c in optim_cases.CASES:
        if c is optim_cases.LARGE:
            continue
        for j in range(len(c["shapes"])):
            assert bool(torch.isfinite(optim_data.param(c, j)).all()), optim_cases.case_id(c)
        for s in range(1, c["steps"] + 1):
            for g in optim_data.step_grads(c, s):
                assert g is None or bool(torch.isfinite(g).all()), optim_cases.case_id(c)


def test_tie_cases_put_requantisation_arguments_exactly_on_a_half():
    """A condition on the inputs: on the first step of the ties cases the emulation's rint() sees at least 16 arguments that are
    exactly k + 1/2 for the signed codes and at least 16 for the unsigned ones, in every such case of the table."""
    seen = {"ties_s": 0, "ties_u": 0}
    for c in optim_cases.CASES:
        kind = c.get("data")
        if kind not in seen:
            continue
        e = optim_data.emulation(c)[0]
        tr = {}
        e.step(optim_data.step_grads(c, 1)[0], trace=tr)
        x = tr["r1"] if kind == "ties_s" else tr["r2"]
        ties = int((tr["valid"] & (np.abs(x - np.trunc(x)) == 0.5)).sum())
        assert ties >= 16, f"{optim_cases.case_id(c)}: {ties} ties"
        seen[kind] += 1
    assert seen["ties_s"] >= 2 and seen["ties_u"] >= 2, seen


# ----------------------------------------------------------------------------- the table closes over the library
def test_table_covers_all_50_instantiations():
    have = set()
    big_generic = set()
    for c in optim_cases.CASES:
        for j in range(len(c["shapes"])):
            k = optim_cases.kernel_of(c, j)
            have.add((c["rule"], c["pdt"], c["gdt"], k))
            if k == "generic" and optim_cases.block_size_of(c, j) > 256 and optim_data.numel_of(c["shapes"][j]) > 256:
                big_generic.add(c["rule"])
    want = {(r, p, g, k) for r in optim_cases.RULES for p, g in optim_cases.PAIRS for k in optim_cases.KERNELS}
    assert len(want) == 50
    assert want <= have, sorted(want - have)
    assert big_generic == set(optim_cases.RULES), big_generic      # the second trip of the generic kernel's loops, per rule
    src = open(os.path.join(os.path.dirname(HERE), "..", "mps_bitsandbytes_amd", "csrc", "optim_kernels.hip")).read()
    assert len(set(re.findall(r"launch<MBNB_OPTIM_(\w+), PT, GT>", src))) == len(optim_cases.RULES)
    assert src.count("__global__") == len(optim_cases.KERNELS)


def test_table_sizes():
    numels = {optim_data.numel_of(s) for c in optim_cases.CASES for s in c["shapes"]}
    assert {1, 3, 255, 256, 257, 1023, 1025, 65541, 4096 * 11008} <= numels
    L = optim_cases.LARGE
    assert (L["rule"], L["pdt"], L["gdt"], L["steps"], L["shapes"]) == ("adamw", "bf16", "bf16", 3, [(4096, 11008)])
    assert all(not c.get("xfail") for c in optim_cases.CASES)      # no known departure of the kernels; one would run as a strict xfail


# ----------------------------------------------------------------------------- teeth
def _stepped():
    c = optim_cases.EDGES[5]          # adamw bf16/bf16, 4099 elements, partial last block
    e = optim_data.emulation(c)[0]
    e.step(optim_data.step_grads(c, 1)[0])
    return e


def _copy(res):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in res.items()}


def test_comparator_passes_on_equal_results():
    e = _stepped()
    emul.compare("same", _copy(e.result()), e.result(), e.bs, e.pdt, e.before)


def test_comparator_fails_on_a_parameter_one_ulp_off():
    e = _stepped()
    got = _copy(e.result())
    b = emul.bits(got["p"]).copy()
    b[3000] += 1
    got["p"] = emul.from_bits(b, e.pdt)
    with pytest.raises(AssertionError, match=r"p: 1 of 4099 differ; first at element 3000 \(block 11, offset 184\).*operands before the step: p=0x"):
        emul.compare("teeth", got, e.result(), e.bs, e.pdt, e.before)


@pytest.mark.parametrize("key,delta", [("q1", 1), ("q1", -1), ("q2", 1), ("q2", -1)])
def test_comparator_fails_on_a_code_off_by_one(key, delta):
    e = _stepped()
    got = _copy(e.result())
    i = int(np.flatnonzero((got[key].astype(np.int64) > 1) & (got[key].astype(np.int64) < 100))[0])
    got[key][i] = int(got[key][i]) + delta
    with pytest.raises(AssertionError, match=rf"{key}: 1 of 4099 differ; first at element {i} "):
        emul.compare("teeth", got, e.result(), e.bs, e.pdt, e.before)


@pytest.mark.parametrize("key", ["a1", "a2"])
def test_comparator_fails_on_a_maximum_one_ulp_off(key):
    e = _stepped()
    got = _copy(e.result())
    got[key].view(np.uint32)[16] += 1
    with pytest.raises(AssertionError, match=rf"{key}: 1 of 17 differ; first at block 16 "):
        emul.compare("teeth", got, e.result(), e.bs, e.pdt, e.before)


def test_comparator_fails_on_a_code_written_past_numel():
    e = _stepped()
    n = e.p.numel()
    buf = np.full(4096 + n + 4096, 0xFF, dtype=np.uint8)
    buf[4096:4096 + n] = e.q1.view(np.uint8)
    got = dict(_copy(e.result()), q1=emul.Guarded(buf, 4096, n, np.int8))
    emul.compare("guarded", got, e.result(), e.bs, e.pdt, e.before)
    buf[4096 + n] = 0
    with pytest.raises(AssertionError, match=r"q1: guard byte written 0 bytes past its end: 0x00"):
        emul.compare("teeth", got, e.result(), e.bs, e.pdt, e.before)
    buf[4096 + n] = 0xFF
    buf[4095] = 7
    with pytest.raises(AssertionError, match=r"q1: guard byte written 1 bytes before the view"):
        emul.compare("teeth", got, e.result(), e.bs, e.pdt, e.before)


def test_comparator_accepts_any_nan_for_a_nan_and_nothing_else():
    want = dict(p=torch.tensor([1.0, float("nan")]), q1=np.zeros(2, np.int8), a1=np.array([np.nan], np.float32))
    got = dict(p=emul.from_bits(np.array([0x3F800000, 0xFFC00001], np.uint32), "f32"), q1=np.zeros(2, np.int8),
               a1=np.array([0x7FC00123], np.uint32).view(np.float32))
    emul.compare("nan", got, want, 256, "f32")
    got["p"] = torch.tensor([1.0, float("inf")])
    with pytest.raises(AssertionError, match="p: 1 of 2 differ; first at element 1 "):
        emul.compare("nan", got, want, 256, "f32")


def test_fma_is_a_single_rounding():
    """Against exact rational arithmetic on operands chosen to double-round under a plain float64 sum."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(20000).astype(np.float32)
    b = rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 20000) * 2.0 ** -24)).astype(np.float32)
    a[:4], b[:4] = np.float32(1 + 2 ** -23), np.float32(1 + 2 ** -23)
    c[:4] = np.array([2 ** -24, -2 ** -24, 2 ** -60, 2.0 ** 30], np.float32) * np.float32(1 + 2 ** -23)
    got = emul.fma(a, b, c)
    for i in list(range(64)) + list(range(64, 20000, 97)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                  # float(Fraction) is correctly rounded to double: find the f32 neighbours
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.float32(x).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)
