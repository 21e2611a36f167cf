"""
Host-side closure of tests/nn_cases.py over csrc/nn_kernels.hip, without a GPU: the table is well formed, every value model(case) can take
has a case, every THRESHOLDS row has a case on each side, every offset operand stands in a pair that differs by that offset alone, the
literals the launchers compare a size with and their pointer tests are the ones the table claims (a scratch copy of the source with one
more branch fails), and the expectation builders of tests/nn_expect.py agree with plain torch restatements.
"""
import os
import re

import pytest
import torch

import oracle
from tests import forms, gemm_variant_cases, nn_cases, nn_expect
from tests.nn_cases import ALIGNMENT_FREE, ALIGNMENT_TESTED, CASES, LIMIT_CLAIMS, LIMIT_COUNTS, THRESHOLDS, case_id, derived, model
from tests.test_elementwise_host import CSRC

SRC = os.path.join(CSRC, "nn_kernels.hip")


def _src():
    with open(SRC) as f:
        return f.read()


def launchers(src):
    """The source without its comments and without its kernels: the top-level definitions that are not __global__."""
    chunks = re.split(r"(?<=\n\})\n", forms.code(src))
    return "\n".join(ch for ch in chunks if "__global__" not in ch)


def limit_counts(src):
    return forms.limit_counts(launchers(src), "int embedding_4bit_dispatch(")


def unclaimed_limits(src):
    counts = limit_counts(src)
    return sorted(k for k in set(counts) | set(LIMIT_COUNTS) if counts.get(k) != LIMIT_COUNTS.get(k))


def alignment_masks(src):
    return [int(m) for m in re.findall(r"& (\d+)\) == 0", launchers(src))]


# ----------------------------------------------------------------------------------------------- the table
def test_cases_are_well_formed():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    emb_keys = {"op", "dim", "bs", "qt", "dt", "idx", "off"}
    lin_keys = {"op", "M", "N", "K", "dt", "n_out", "bias", "oob", "off", "ws", "err"}
    for c in CASES:
        assert c["dt"] in nn_cases.DTS
        for operand, off in c.get("off", {}).items():
            assert operand in nn_cases.OPERANDS[c["op"]] and 0 < off <= 16, case_id(c)
            if operand in ("out", "x", "ow"):
                assert off % nn_cases.ESIZE[c["dt"]] == 0, case_id(c)
        if nn_cases.is_emb(c):
            assert set(c) <= emb_keys, case_id(c)
            assert c["idx"] in ("many", "one", "i32", "pad", "oob") and c["dim"] >= 1
            if c["op"] == "embedding_4bit":
                assert c["dim"] % 2 == 0 and c["bs"] > 0 and c["qt"] in ("nf4", "fp4")
            assert c["dim"] <= 4104                                   # tiny: 11 rows of at most 4104 columns
        else:
            assert set(c) <= lin_keys and c["op"] in nn_cases.LIN_OPS, case_id(c)
            assert c.get("ws") in (None, "exact", "n0", "two", "short") and (("ws" in c) == (c["op"] == "outlier_abi"))
            assert ("err" in c) == (model(c)[0] == "error"), case_id(c)
            if "err" in c:
                assert c["op"] == "outlier_abi" and model(c) == ("error", c["err"])
            if c.get("oob"):
                assert c["n_out"] > 0 and set(nn_cases.index_list(c)) - set(nn_cases.positions(c)) == {-1, c["K"]}
            pos = nn_cases.positions(c)
            assert len(set(pos)) == len(pos) == c["n_out"] and all(0 <= p < c["K"] for p in pos)
            # no LLM-sized operand but the two MFMA-sized cases and the mask limit's 2 x 65536
            assert c["M"] * c["K"] <= 1 << 19 and c["N"] * c["K"] <= 1 << 20, case_id(c)


def test_the_outlier_positions_reach_every_hiding_place():
    """0 and 1 together, K - 1, an even / odd pair in another group of 8, a column of the scalar tail, an unsorted order."""
    lin = [c for c in CASES if not nn_cases.is_emb(c) and c["n_out"] >= 5]
    assert lin
    for c in lin:
        pos, K = nn_cases.positions(c), c["K"]
        assert {0, 1, K - 1} <= set(pos) and pos != sorted(pos), case_id(c)
        if K >= 16:
            assert {10, 11} <= set(pos)
        if K % 8 and c["n_out"] >= 6 or K % 8 and K - 1 >= K // 8 * 8:
            assert any(p >= K // 8 * 8 for p in pos), case_id(c)
    assert any(c["K"] % 8 and c["n_out"] >= 5 for c in lin)
    assert nn_cases.positions(dict(K=203, n_out=6))[:6] == [1, 0, 202, 11, 10, 200]


def test_every_value_of_the_model_has_a_case():
    emb = {(c["op"], c["dt"]) + model(c) for c in CASES if nn_cases.is_emb(c)}
    for op in nn_cases.EMB_OPS:
        for dt in nn_cases.DTS:
            for form in ("vec", "scalar"):
                assert any(e[:3] == (op, dt, form) for e in emb), (op, dt, form)
        for form in ("vec", "scalar"):
            for threads in (64, 128, 256):
                # the scalar form at 1024 and more columns: by a pointer or a width that is no multiple of 8 -- no case needs a wide row for it
                if form == "vec":
                    assert any(e[0] == op and e[2:] == (form, threads) for e in emb), (op, form, threads)
    for qt in ("nf4", "fp4"):
        for dt in nn_cases.DTS:
            assert {model(c)[0] for c in CASES if c["op"] == "embedding_4bit" and c["qt"] == qt and c["dt"] == dt} == {"vec", "scalar"}
    assert any(c["op"] == "embedding_4bit" and c["bs"] % 8 and model(c)[0] == "vec" for c in CASES), "one_am false on the vector path"
    assert any(c["op"] == "embedding_4bit" and c["bs"] % 2 and model(c)[0] == "vec" for c in CASES), "a byte whose nibbles lie in two blocks, on the vector path"
    assert any(c["op"] == "embedding_4bit" and c["bs"] > c["dim"] for c in CASES) and any(c["op"] == "embedding_4bit" and c["dim"] % c["bs"] for c in CASES)
    lin = [(c, derived(c)) for c in CASES if not nn_cases.is_emb(c)]
    ok = [(c, d) for c, d in lin if not d["error"]]
    # each quantiser form x the dtypes it is instantiated for
    have = {(d["quant"], c["dt"]) for c, d in ok}
    assert have == {("regs", "f16"), ("regs", "bf16")} | {(f, dt) for f in ("two_pass_vec", "two_pass_scalar") for dt in nn_cases.DTS}, have
    # xo present and absent, in every quantiser form that can write it
    assert {(d["quant"], d["xo"]) for c, d in ok if d["is16"] and c["n_out"]} >= {("regs", True), ("regs", False), ("two_pass_vec", True), ("two_pass_scalar", True)}
    # the epilogue: fused, none, the add launch with each of vec_out and ow_vec on and off, in every dtype
    epis = {d["epi"] for c, d in ok}
    assert {"fused", "none"} <= epis
    for dt in nn_cases.DTS:
        adds = {d["epi"][1:] for c, d in ok if d["add"] and c["dt"] == dt}
        assert {(True, True), (True, False), (False, False)} <= adds, (dt, adds)
    assert {c["dt"] for c, d in ok if d["epi"] == "fused"} == {"f16", "bf16"}
    assert {d["kernel"] for c, d in ok} == {"i8_generic", "i8_mfma128", "i8_dense+outliers"}
    assert {c["err"] for c, d in lin if d["error"]} == {"too small", "too large for the LDS column mask"}


def test_the_model_agrees_with_the_gemm_tables_restatement_where_the_workspace_has_room():
    n = 0
    for c in CASES:
        if c["op"] == "outlier_linear" and not nn_cases.offset(c, "ws") % 16 and not c.get("oob"):
            d = dict(M=c["M"], N=c["N"], K=c["K"], dt=c["dt"])
            assert model(c)[3:] == gemm_variant_cases._outlier(c, d), case_id(c)
            n += 1
    assert n > 40


def test_every_threshold_has_a_case_on_each_side():
    rows = [t[0] for t in THRESHOLDS]
    assert len(rows) == len(set(rows))
    for what, ops, first, second in THRESHOLDS:
        cs = [(c, derived(c)) for c in CASES if c["op"] in ops]
        assert any(first(c, d) for c, d in cs), f"{what} {ops}: no case on the first side"
        assert any(second(c, d) for c, d in cs), f"{what} {ops}: no case on the second side"


def test_every_offset_operand_stands_in_a_pair_that_differs_by_that_offset_alone():
    offset = {(c["op"], k) for c in CASES for k in c.get("off", {})}
    assert offset == set(ALIGNMENT_TESTED) | ALIGNMENT_FREE
    for (op, operand), (aligned, off) in ALIGNMENT_TESTED.items():
        ps = nn_cases.pairs(op, operand)
        assert ps, (op, operand)
        for c, b in ps:
            assert {k: v for k, v in c.items() if k != "off"} == b and set(c["off"]) == {operand}
            assert nn_cases.form_of(c, operand) != nn_cases.form_of(b, operand), case_id(c)
        assert any((nn_cases.form_of(b, operand), nn_cases.form_of(c, operand)) == (aligned, off) for c, b in ps), (op, operand)
    for op, operand in ALIGNMENT_FREE:
        ps = nn_cases.pairs(op, operand)
        assert ps and all(model(c) == model(b) for c, b in ps), (op, operand)
    by_off = {(c["op"], k, v) for c in CASES for k, v in c.get("off", {}).items()}
    assert {("embedding_4bit", "packed", 1), ("embedding_4bit", "packed", 2), ("embedding_8bit", "w", 4)} <= by_off
    assert {("embedding_4bit", "out", v) for v in (2, 4, 8)} | {("embedding_8bit", "out", v) for v in (2, 4, 8)} <= by_off


# ----------------------------------------------------------------------------------------------- the source
def test_every_limit_of_the_launchers_is_claimed_by_a_threshold_or_listed_as_having_no_case():
    assert unclaimed_limits(_src()) == [], limit_counts(_src())
    rows = {t[0] for t in THRESHOLDS}
    assert set(LIMIT_CLAIMS) == set(LIMIT_COUNTS)
    for lit, claim in LIMIT_CLAIMS.items():
        for one in (claim if isinstance(claim, list) else [claim]):
            assert one in rows or (isinstance(one, tuple) and one[0] == "no case" and one[1]), (lit, one)
    assert f"mask_lds > {nn_cases.MASK_MAX_BYTES}" in _src() and f"K <= {nn_cases.REGS_MAX_K}" in _src()
    # the grid.y limit this table leaves to the GEMM table is held there
    assert any(t[0] == "k_outlier_add: 65535 row groups in grid.y" for t in gemm_variant_cases.THRESHOLDS)


def test_the_pointer_tests_are_the_ones_the_table_knows():
    src = _src()
    assert alignment_masks(src) == nn_cases.ALIGNMENT_MASKS
    assert len(re.findall(r"reinterpret_cast<uintptr_t>", launchers(src))) == len(nn_cases.ALIGNMENT_MASKS) == gemm_variant_cases.ALIGNMENT_TEST_COUNTS["nn_kernels.hip"]
    assert len(ALIGNMENT_TESTED) == len(nn_cases.ALIGNMENT_MASKS)
    # the kernels themselves test no pointer
    assert "uintptr_t" not in "".join(ch for ch in re.split(r"(?<=\n\})\n", forms.code(src)) if "__global__" in ch)


def test_the_gemm_table_keeps_its_entries_for_this_file():
    assert gemm_variant_cases.ALIGNMENT_TEST_COUNTS["nn_kernels.hip"] == 7 and gemm_variant_cases.INTEGER_LIMITS["nn_kernels.hip"] == [8192]
    assert len(gemm_variant_cases.ALIGNMENT_TEST_COUNTS) == 9 and len(gemm_variant_cases.INTEGER_LIMITS) == 9


def test_the_closure_fails_on_a_launcher_branch_without_a_case():
    src = _src()
    a = src.replace("if (vec_ok && K <= 8192)", "if (vec_ok && K <= 8192 && M < 4096)")
    assert a != src and unclaimed_limits(a) == ["4096"]
    b = src.replace("const bool vec_out = (N % 2 == 0) &&", "const bool vec_out = (N % 4 == 0) &&")
    assert b != src and unclaimed_limits(b) == ["% 2", "% 4"]
    c = src.replace(" && ((reinterpret_cast<uintptr_t>(ow) & 15) == 0)", "")
    assert c != src and alignment_masks(c) != nn_cases.ALIGNMENT_MASKS
    d = src.replace("const unsigned threads = dim >= 2048 ? 256 :", "const unsigned threads = dim >= 4096 ? 512 : dim >= 2048 ? 256 :", 1)
    assert d != src and unclaimed_limits(d) == ["4096"]
    # a comparison inside a kernel is not the launchers' business
    e = src.replace("if (n0 >= N) continue;", "if (n0 >= N || N > 77777) continue;")
    assert e != src and unclaimed_limits(e) == []


# ----------------------------------------------------------------------------------------------- the expectation builders
def _plain_quantize_rowwise(x):
    """functional.quantize_rowwise's arithmetic in plain torch: absmax clamped at 1e-8, x * (127 / absmax) rounded half to even, clamped."""
    xf = x.float()
    am = xf.abs().amax(1).clamp_min(1e-8)
    q = torch.clamp(torch.round(xf * (127.0 / am)[:, None]), -127, 127).to(torch.int8)
    return q, am


_SMALL = [c for c in CASES if not nn_cases.is_emb(c) and (c["M"], c["N"]) == (5, 6) and c["K"] in (200, 203) and c["n_out"] == 5 and not c.get("off") and not c.get("ws")]


def test_three_small_cases_are_there_for_the_builders():
    assert len({(c["dt"], c["K"]) for c in _SMALL}) >= 3 and any(c.get("oob") for c in _SMALL)


@pytest.mark.parametrize("case", _SMALL, ids=case_id)
def test_the_masked_quantise_expectation_against_a_plain_restatement(case):
    c = case
    ops = nn_expect.linear_operands(c)
    x, pos, K, M = ops["x"], ops["pos"], c["K"], c["M"]
    xq, scales, xo = nn_expect.workspace_expected(c, ops)
    # the inputs are what the table promises: x64 in the outlier columns, the three special rows, weights nonzero in those columns
    keep = [k for k in range(K) if k not in pos]
    assert float(x[:M - 3, pos].float().abs().mean()) > 16 * float(x[:M - 3, keep].float().abs().mean())
    assert not bool(x[M - 1].any()) and not bool(x[M - 2, keep].any()) and bool(x[M - 2, pos].all())
    top = int(x[M - 3, keep].float().abs().argmax())
    assert keep[top] - 1 in pos or keep[top] + 1 in pos
    assert bool((ops["q"][:, pos] != 0).any(0).all())
    # the reference quantises the compacted columns: the same codes and scales, and zeros in the outlier columns
    qc, sc = _plain_quantize_rowwise(x[:, keep])
    assert torch.equal(xq[:, keep], qc) and torch.equal(scales, sc) and not bool(xq[:, pos].any())
    assert float(scales[M - 1]) == float(scales[M - 2]) == float(torch.tensor(1e-8, dtype=torch.float32))
    # a quantiser that ignores the mask gives other scales in every ordinary row
    assert bool((oracle.quantize_rowwise(x)[1][:M - 3] > 4 * scales[:M - 3]).all())
    lst = nn_cases.index_list(c)
    if xo is not None:
        assert xo.shape == (M, 16) and xo.dtype == x.dtype
        for j, k in enumerate(lst):
            assert torch.equal(xo[:, j], x[:, k] if 0 <= k < K else torch.zeros(M, dtype=x.dtype))
        assert not bool(xo[:, len(lst):].any())
    else:
        assert c["dt"] == "f32"
    # the output reference does not see the weight inside the outlier columns, nor the entries out of range
    ref = nn_expect.reference_output(c, ops)
    q2 = ops["q"].clone()
    q2[:, pos] = 0
    assert torch.equal(ref, oracle.outlier_linear(x, q2, ops["s"], torch.tensor(pos), ops["ow"], ops["b"]))
    oi, ow = nn_expect.given_indices(c, ops)
    inr = (oi >= 0) & (oi < K)
    assert oi[inr].tolist() == pos and torch.equal(ow[:, inr], ops["ow"]) and oi.numel() == nn_cases.n_entries(c)


@pytest.mark.parametrize("case", _SMALL[:3], ids=case_id)
def test_the_bound_follows_the_masked_row_and_holds_the_oracle_against_float64(case):
    """The bound's own arithmetic on the CPU: it does not grow with the outlier activations' size beyond their own term, and the exact float64
    value of what both sides compute lies inside it around the oracle."""
    from tests.test_gpu_elementwise import outlier_masked_bound
    c = case
    ops = nn_expect.linear_operands(c)
    dt, pos = nn_expect.DT[c["dt"]], ops["pos"]
    x, ow, b = ops["x"], ops["ow"], ops["b"]
    Wd = oracle.dequantize_rowwise(ops["q"], ops["s"], dt)
    ref = nn_expect.reference_output(c, ops)
    bound = outlier_masked_bound(x, Wd, pos, ow, b, ref, dt)
    xq, scales, _ = nn_expect.workspace_expected(c, ops)
    exact = (xq.double() * (scales.double() / 127.0)[:, None]) @ (ops["q"].double() * (ops["s"].double() / 127.0)[:, None]).t()
    exact = exact + x[:, pos].double() @ ow.double().t() + (0 if b is None else b.double())
    assert bool(((exact - ref.double()).abs() <= bound).all())
    # a contraction that reads the int8 weight inside one outlier column is far outside it
    wrong = exact + x[:, pos[:1]].double() @ (ops["q"][:, pos[:1]].double() * (ops["s"].double() / 127.0)[:, None]).t()
    assert bool(((wrong - ref.double()).abs() > bound)[:c["M"] - 3].any(1).all())


def test_the_workspace_splitter_against_the_librarys_query():
    from mps_bitsandbytes_amd import _native
    q = _native.lib().mbnb_outlier_linear_workspace_bytes if _native.available() else None
    for M, K, n in [(5, 200, 5), (17, 200, 17), (1, 8, 0), (33, 203, 33), (2, 65536, 2), (1536, 256, 40)]:
        want = ((M * K + 255) // 256 + (4 * M + 255) // 256 + (2 * 16 * ((max(n, 16) + 15) // 16) * M + 255) // 256) * 256      # tests/test_native_abi.py's formula
        assert nn_cases.ws_query(M, K, n) == want
        if q is not None:
            assert q(M, K, n) == want
        off_s, off_x, end_x = nn_cases.regions(M, K, n)
        assert off_s % 256 == 0 and off_x % 256 == 0 and off_s >= M * K and off_x - off_s >= 4 * M and end_x <= nn_cases.ws_query(M, K, n)
        ws = torch.full((nn_cases.ws_query(M, K, n),), 0x5A, dtype=torch.uint8)
        ws[:M * K] = 1
        ws[off_s:off_s + 4 * M] = 2
        ws[off_x:end_x] = 3
        xq, scales, xo, pads = nn_expect.split_workspace(ws, M, K, n, 0x5A)
        assert pads and bool((xq == 1).all()) and xq.shape == (M, K) and scales.numel() == M and bool((xo == 3).all()) and xo.numel() == end_x - off_x
        for at in {M * K, off_s - 1, off_s + 4 * M, off_x - 1, end_x, ws.numel() - 1} - set(range(M * K)) - set(range(off_s, off_s + 4 * M)) - set(range(off_x, end_x)) - {ws.numel()}:
            w2 = ws.clone()
            w2[at] = 0
            assert not nn_expect.split_workspace(w2, M, K, n, 0x5A)[3], (M, K, n, at)
    # the n = 0 query leaves a 17-column call no room from five rows on; the first two regions alone pass the ABI's own check
    assert nn_cases.ws_query(17, 200, 0) < nn_cases.layout_bytes(17, 200, 17) and nn_cases.ws_query(4, 200, 0) == nn_cases.layout_bytes(4, 200, 17)


@pytest.mark.parametrize("case", [c for c in CASES if nn_cases.is_emb(c) and c["dim"] <= 100 and c["dt"] == "f16" and not c.get("off")], ids=case_id)
def test_the_embedding_expectation_against_a_plain_restatement(case):
    c = case
    a, b = nn_expect.embedding_operands(c)
    want = nn_expect.embedding_expected(c, a, b)
    idx, pad = nn_expect.indices(c)
    flat = idx.reshape(-1).to(torch.int64)
    dim = c["dim"]
    if c["op"] == "embedding_4bit":
        from mps_bitsandbytes_amd.functional import create_fp4_map, create_normal_map
        if dim >= 70:
            assert set((a & 15).reshape(-1).tolist()) == set(range(16)) == set((a >> 4).reshape(-1).tolist())
        code = (create_normal_map() if c["qt"] == "nf4" else create_fp4_map()).float()
        nib = torch.stack([a & 15, a >> 4], dim=-1).reshape(nn_cases.NUM, dim).long()
        table = (code[nib] * b.repeat_interleave(c["bs"], dim=1)[:, :dim]).to(torch.float16)
    else:
        assert int(a.min()) == -128 and int(a.max()) == 127
        table = a.to(torch.float16) * (b / 127.0).to(torch.float16)[:, None]
    for t, r in enumerate(flat.tolist()):
        row = want.reshape(-1, dim)[t]
        if r < 0 or r >= nn_cases.NUM or r == pad:
            assert not bool(row.any())
        else:
            assert torch.equal(row.view(torch.int16), table[r].view(torch.int16)), (t, r)
    if c["idx"] == "many":
        assert 0 in flat.tolist() and bool(want.reshape(-1, dim)[flat.tolist().index(0)].any()), "row 0 without a padding_idx is looked up"
