"""
The boundary data of tests/rounding_cases.py is sharp -- proven on the CPU, with the oracle and the numpy restatements alone.

- the restatements equal the oracle bit for bit on all builder data (the oracle is the arbiter; the restatements exist to be mutated);
- the data is SENSITIVE: the floors below count the elements whose output changes when the quotient (4-bit, FP8) or the product (int8)
  moves to a neighbouring f32 -- at least one per scale and boundary on average, at every exponent;
- both codes next to every boundary occur in the expected output at every exponent;
- every MUTANT of a restatement -- a reciprocal for the division, a threshold one ulp off, >= for >, the first guess of the neighbouring
  bin, 127 / am in one rounding, another rounding rule, another bump count ... -- changes at least 16 expected outputs on f32 data;
- the edge cases of the fast paths lie on the side they claim (shared_div_ok and FP8's `shared` restated in rounding_cases).

Every assertion prints its counts when it fails.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle
from tests import int8_decomp_emul as emul
from tests import rounding_cases as rc

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mps_bitsandbytes_amd", "csrc")
MIN_MUTANT = 16
QTS = ("nf4", "fp4")
DTS = ("f32", "f16", "bf16")


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(rc.DT[dt])


@functools.lru_cache(maxsize=None)
def _own(qt, dt):
    return rc.q4_own(qt, dt, 128)


@functools.lru_cache(maxsize=None)
def _given(qt, dt):
    return rc.q4_given(qt, dt, 8)


@functools.lru_cache(maxsize=None)
def _rows(dt):
    return rc.int8_rows(dt)


@functools.lru_cache(maxsize=None)
def _fp8(dt):
    return rc.fp8_rows(dt)


def _per(sens, d, n):
    """{exponent: [sensitive count per boundary]} of the non-edge blocks."""
    return {int(e): [int((sens & (d["tid"] == i) & (d["exp"][:, None] == e)).sum()) for i in range(n)] for e in np.unique(d["exp"]) if e != 999}


# ----------------------------------------------------------------------------------------------- the kernels' tables
def test_restated_thresholds_and_bins_are_the_kernels():
    src = open(os.path.join(CSRC, "quant_kernels.hip")).read()
    nf4 = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{8})u", re.search(r"NF4_THR_BITS\[15\] = \{(.*?)\};", src, re.S).group(1))]
    fp4 = [float(v.rstrip("f")) for v in re.search(r"FP4_THR\[7\] = \{(.*?)\};", src).group(1).split(",")]
    assert nf4 == [int(v) for v in rc.thresholds("nf4").view(np.uint32)]
    assert fp4 == [float(v) for v in rc.thresholds("fp4")]
    inc = open(os.path.join(CSRC, "code_bins.inc")).read()
    for name, qt in (("g_nf4_bins", "nf4"), ("g_fp4_bins", "fp4")):
        body = re.search(name + r"\[256\] = \{(.*?)\};", inc, re.S).group(1)
        assert [int(v) for v in re.findall(r"\d+", body)] == rc.code_bins(qt).tolist(), name


# ----------------------------------------------------------------------------------------------- 4-bit
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qt", QTS)
def test_q4_restatement_equals_the_oracle(qt, dt):
    for d, given in ((_own(qt, dt), False), (_given(qt, dt), True), (rc.fp4_ties_16bit(dt if dt != "f32" else "f16"), False)):
        if d["qt"] != qt:
            continue
        p, am, _ = oracle.quantize_4bit(_t(d["x"], d["dt"]).reshape(-1), d["bs"], qt, absmax=torch.from_numpy(d["am"]) if given else None)
        assert np.array_equal(am.numpy().view(np.uint32), d["am"].view(np.uint32)), "the absmax the builder states is not the block's"
        want = rc.unpack(p.numpy(), d["x"].shape)
        got = rc.q4_literal(d["x"], d["am"], qt)
        assert np.array_equal(want, got), f"{int((want != got).sum())} codes of the restatement differ from the oracle's"
        q = rc.quotient(d["x"], d["am"][:, None]).reshape(-1)
        small = np.abs(q) < 2.0 ** 22
        assert np.array_equal(rc.q4_counting(q, qt)[small], got.reshape(-1)[small]), "the counting form differs from the argmin"
        assert np.array_equal(rc.q4_counting(q, qt, bins=rc.code_bins(qt))[small], got.reshape(-1)[small]), "the 256-bin form differs from the argmin"


@pytest.mark.parametrize("qt", QTS)
@pytest.mark.parametrize("route,dt", [("own", "f32"), ("given", "f32"), ("given", "f16"), ("given", "bf16")])
def test_q4_sensitivity_floor_and_both_codes(qt, route, dt):
    """>= one sensitive element per absmax on average for every midpoint at every exponent: 512 with 512 mantissas.  (16-bit inputs with the
    block's own absmax cannot meet a floor: a 16-bit x and a 16-bit absmax almost never give a quotient next to an NF4 midpoint; the
    supplied-absmax data and FP4's exact ties carry them.)"""
    d = (_own if route == "own" else _given)(qt, dt)
    n = len(rc.midpoints(qt))
    per = _per(rc.q4_sensitive(d), d, n)
    print(f"\nsensitive {qt} {route} {dt}: " + "; ".join(f"2^{e}: min {min(v)} max {max(v)}" for e, v in per.items()))
    for e, v in per.items():
        assert min(v) >= rc.N_MANT, f"{qt} {route} {dt}, exponent {e}: sensitive elements per midpoint {v}, the floor is {rc.N_MANT}"
    codes = rc.q4_literal(d["x"], d["am"], qt)
    for e in per:
        for i, (lo, hi) in enumerate(rc.neighbour_codes(qt)):
            seen = set(np.unique(codes[(d["tid"] == i) & (d["exp"][:, None] == e)]).tolist())
            assert {lo, hi} <= seen, f"{qt} {route} {dt}, exponent {e}, midpoint {i}: codes {sorted(seen)}, both of {lo} and {hi} must occur"


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_fp4_midpoints_are_exact_ties_in_16_bits(dt):
    d = rc.fp4_ties_16bit(dt)
    q = rc.quotient(d["x"], d["am"][:, None])
    mid = rc.midpoints("fp4").astype(F32)
    assert np.array_equal(q[:, 1:15], np.broadcast_to(mid, (len(d["am"]), 14))), "x / absmax is not the midpoint itself"
    sig = sorted({bin(int(np.frexp(a)[0] * 8)).count("1") for a in d["am"]})
    assert sig == [1, 2, 3], f"absmax values of {sig} significant bits"
    assert rc.q4_sensitive(d)[:, 1:15].all()


def _q4_mutants(qt):
    return rc.Q4_MUTANTS + [("thr", i, s) for i in range(len(rc.thresholds(qt))) for s in (1, -1)]


def test_q4_mutant_count():
    assert sum(len(rc.thresholds(qt)) * 2 for qt in QTS) == 44


@pytest.mark.parametrize("qt", QTS)
def test_every_q4_mutant_changes_expected_outputs(qt):
    """On the f32 blocks with their own absmax (the route the kernels' shared division serves).  The first guess of the bin BELOW is no
    mutant: neighbouring thresholds are more than two bins apart, so the exact compare repairs that guess (asserted)."""
    d = _own(qt, "f32")
    want = rc.q4_literal(d["x"], d["am"], qt)
    counts = {str(m): int((rc.q4_mutant_codes(d, m) != want).sum()) for m in _q4_mutants(qt)}
    print(f"\n{qt} mutants: {counts}")
    weak = {m: c for m, c in counts.items() if c < MIN_MUTANT}
    assert not weak, f"{qt}: mutants the data does not catch {weak}; all counts {counts}"
    q = rc.quotient(d["x"], d["am"][:, None]).reshape(-1)
    assert np.array_equal(rc.q4_counting(q, qt, bins=rc.code_bins(qt), bin_shift=-1), want.reshape(-1))


@pytest.mark.parametrize("qt", QTS)
def test_q4_edges_are_where_they_claim(qt):
    d = _own(qt, "f32")
    pos = d["edge_pos"]
    assert len(pos) >= 6
    inside = [rc.shared_div_ok(a) for a in d["am"][pos]]
    assert not all(inside) and any(inside)
    first = {bits: i for i, bits in reversed(list(enumerate(d["am"][pos].view(np.uint32).tolist())))}
    assert rc.shared_div_ok(F32(2.0 ** 60)) and not rc.shared_div_ok(rc.up(F32(2.0 ** 60))) and rc.shared_div_ok(rc.up(F32(2.0 ** 60), -1))
    for v in (F32(2.0 ** 60), rc.up(F32(2.0 ** 60)), rc.up(F32(2.0 ** 60), -1), F32(1e-8), rc.up(F32(1e-8))):
        assert rc.bits(v) in first, f"no edge block with absmax {float(v)!r}"
    assert (d["x"][pos, 0] < F32(1e-8)).any(), "no block below the clamp"
    # an out-of-range block stands alone: the 8 blocks around it (a wave's span of 512 values and more) are in range
    out = [p for p in pos if not rc.shared_div_ok(d["am"][p])]
    for p in out:
        near = [k for k in range(p - 4, p + 5) if k != p and k not in out]
        assert all(rc.shared_div_ok(d["am"][k]) for k in near)
    g = _given(qt, "f32")
    e = g["am"][g["edge_pos"]]
    assert (e < F32(2.0 ** -60)).any() and (e == F32(2.0 ** -60)).any() and (e > F32(2.0 ** 60)).any()


# ----------------------------------------------------------------------------------------------- int8
@pytest.mark.parametrize("dt", DTS)
def test_int8_restatement_equals_the_oracle(dt):
    d = _rows(dt)
    x = _t(d["x"], dt)
    q, s = oracle.quantize_rowwise(x)
    want = rc.int8_codes(d["x"], d["am"][:, None])
    assert np.array_equal(s.numpy().view(np.uint32), d["am"].view(np.uint32))
    assert np.array_equal(q.numpy(), want), f"rows: {int((q.numpy() != want).sum())} codes differ"
    for given in (False, True):
        b = rc.int8_blocks(dt, 32, given=given)
        q, a = oracle.quantize_blockwise(_t(b["x"], dt).reshape(-1), 32, torch.from_numpy(b["am"]) if given else None)
        assert np.array_equal(a.numpy().view(np.uint32), b["am"].view(np.uint32))
        assert np.array_equal(q.numpy().reshape(b["x"].shape), rc.int8_codes(b["x"], b["am"][:, None])), f"blocks, given={given}"
    # double_quant: the rows' boundaries, and the same matrix transposed for the columns'
    sub = d["x"][::8]
    for m in (sub, np.ascontiguousarray(sub.T)):
        oc, orow, cs, rs, _ = oracle.double_quant(_t(m, dt))
        rm, cm = np.maximum(np.abs(m).max(axis=1), rc.CLAMP), np.maximum(np.abs(m).max(axis=0), rc.CLAMP)
        assert np.array_equal(rs.numpy(), rm) and np.array_equal(cs.numpy(), cm)
        assert np.array_equal(orow.numpy(), rc.int8_codes(m, rm[:, None])) and np.array_equal(oc.numpy(), rc.int8_codes(m, cm[None, :]))
    # the nested statistics of quantize_4bit(compress_statistics=True)
    c = rc.int8_absmax_blocks(dt, n=64)
    _, qa, (am2, _) = oracle.quantize_4bit(_t(c["x"], dt).reshape(-1), c["bs"], "nf4", True)
    assert np.array_equal(am2.numpy(), c["am2"])
    assert np.array_equal(qa.numpy().reshape(-1, 256), rc.int8_codes(c["absmax"].reshape(-1, 256), c["am2"][:, None]))


@pytest.mark.parametrize("dt", DTS)
def test_colrow_and_coo_data_on_the_emulation_chains(dt):
    x = rc.colrow_matrix(dt)
    xt = _t(x, dt)
    rm, cm = emul.colrow_stats(xt)
    assert np.array_equal(rm[1:], x[1:, 0]) and np.array_equal(cm, x[0]), "the statistics are not the ones the matrix was built for"
    s = emul.colrow_scale(rm, cm)
    assert np.array_equal(emul.colrow_codes(xt, s), rc.int8_codes(x, s))
    sens = rc.int8_sensitive(x, s)[1:, 1:]
    print(f"\ncolrow {dt}: {int(sens.sum())} of {sens.size} elements sensitive")
    if dt == "f32":
        assert sens.sum() >= sens.size // 5, f"{int(sens.sum())} of {sens.size}"       # one of the 5 steps around each half-integer
    v = rc.coo_values(dt)[:4]
    for row in v:
        q, scale = emul.coo_quantize(_t(row, dt))
        with np.errstate(all="ignore"):
            want = np.clip(np.rint(row / (np.abs(row).max() / F32(127.0))), -127, 127).astype(np.int8)
        assert np.array_equal(q.numpy(), want)


def test_int8_sensitivity_floor():
    """f32: at least one sensitive element per (absmax, half-integer) pair on average, at every exponent."""
    d = _rows("f32")
    sens = rc.int8_sensitive(d["x"], d["am"][:, None])
    p = rc.int8_product(d["x"], d["am"][:, None])
    ties = np.abs(p - np.trunc(p)) == 0.5
    per = {int(e): (int(sens[d["exp"] == e].sum()), int(ties[d["exp"] == e].sum())) for e in np.unique(d["exp"]) if e != 999}
    print(f"\nint8 rows f32: (sensitive, exact ties) per exponent {per}")
    for e, (n, _) in per.items():
        assert n >= rc.N_MANT * 254, f"exponent {e}: {n} sensitive elements, the floor is {rc.N_MANT * 254}"
    codes = rc.int8_codes(d["x"], d["am"][:, None])
    for e in per:
        assert set(np.unique(codes[d["exp"] == e]).tolist()) == set(range(-127, 128)), f"exponent {e}: not every code occurs"
    c = rc.int8_absmax_blocks("f32")
    n = int(rc.int8_sensitive(c["absmax"].reshape(-1, 256), c["am2"][:, None]).sum())
    assert n >= rc.N_MANT * 127, f"nested statistics: {n} sensitive absmax values"


def test_every_int8_mutant_changes_expected_outputs():
    d = _rows("f32")
    want = rc.int8_codes(d["x"], d["am"][:, None])
    counts = {m: int((rc.int8_codes(d["x"], d["am"][:, None], m) != want).sum()) for m in rc.INT8_MUTANTS}
    print(f"\nint8 mutants: {counts}")
    assert min(counts.values()) >= MIN_MUTANT, counts
    g = rc.int8_blocks("f32", 32, given=True)
    codes = rc.int8_codes(g["x"], g["am"][:, None])
    p = rc.int8_product(g["x"], g["am"][:, None])
    assert ((np.abs(p) > 127.5) & (np.abs(codes) == 127)).sum() >= MIN_MUTANT, "the clamp is not met"


# ----------------------------------------------------------------------------------------------- FP8
@pytest.mark.parametrize("dt", DTS)
def test_fp8_restatement_equals_the_oracle(dt):
    d = _fp8(dt)
    q, s = oracle.quantize_fp8_e4m3(_t(d["x"], dt))
    assert np.array_equal(s.numpy().view(np.uint32), d["s"].view(np.uint32))
    got = rc.fp8_codes(d["x"], d["s"][:, None])
    assert np.array_equal(q.numpy(), got), f"{int((q.numpy() != got).sum())} codes differ"


def test_fp8_sensitivity_floor_and_both_codes():
    """The floor (the issue measured none for FP8) is the 4-bit one: one sensitive element per scale and boundary on average."""
    d = _fp8("f32")
    sens = rc.fp8_sensitive(d["x"], d["s"][:, None])
    codes = rc.fp8_codes(d["x"], d["s"][:, None])
    nb = len(rc.fp8_boundaries())
    for e in (int(v) for v in np.unique(d["exp"]) if v != 999):
        rows = d["exp"] == e
        per = [int(sens[rows][:, d["bid"] == i].sum()) for i in range(nb)]
        print(f"\nfp8 f32 2^{e}: sensitive per boundary min {min(per)} max {max(per)} total {sum(per)}")
        assert sum(per) >= rc.N_MANT * nb, f"exponent {e}: {sum(per)} sensitive, the floor is {rc.N_MANT * nb}"
        for i, (b, _, _, kind) in enumerate(rc.fp8_boundaries()):
            seen = np.unique(codes[rows][:, d["bid"] == i] & 0x7F)
            if kind != "dead":
                assert per[i] >= rc.N_MANT, f"exponent {e}, boundary {b}: {per[i]} sensitive"
                assert len(seen) >= 2, f"exponent {e}, boundary {b}: only the codes {seen}"


def test_every_fp8_mutant_changes_expected_outputs():
    d = _fp8("f32")
    want = rc.fp8_codes(d["x"], d["s"][:, None])
    counts = {m: int((rc.fp8_codes(d["x"], d["s"][:, None], m) != want).sum()) for m in rc.FP8_MUTANTS}
    print(f"\nfp8 mutants: {counts}")
    assert min(counts.values()) >= MIN_MUTANT, counts


def test_fp8_edges_are_where_they_claim():
    d = _fp8("f32")
    edge = d["s"][d["exp"] == 999]
    for v in (F32(2.0 ** -20), F32(2.0 ** 60)):
        assert (edge == v).any() and rc.fp8_shared(v, F32(1.0)), f"no row whose scale is {float(v)!r}"
    below = edge[(edge < F32(2.0 ** -20)) & (edge >= rc.up(F32(2.0 ** -20), -4))]
    above = edge[(edge > F32(2.0 ** 60)) & (edge <= rc.up(F32(2.0 ** 60), 4))]
    assert len(below) and len(above), "no neighbour outside the shared division's range of scales"
    assert not any(rc.fp8_shared(v, F32(1.0)) for v in np.concatenate([below, above]))
    assert (edge == F32(1e-12)).any(), "no row at the clamp of the scale"
    last = d["x"][:, -1]
    assert (np.abs(last) == F32(2.0 ** -90)).any() and ((np.abs(last) < F32(2.0 ** -90)) & (last != 0)).any()
    assert rc.fp8_shared(F32(1.0), F32(2.0 ** -90)) and not rc.fp8_shared(F32(1.0), rc.up(F32(2.0 ** -90), -1)) and rc.fp8_shared(F32(1.0), F32(0.0))
