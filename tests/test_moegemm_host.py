"""CPU-side checks of the grouped GEMM over MXFP4 experts (libmbnb_moegemm.so, functional.matmul_mxfp4_experts_grouped / _glu / _sum;
DESIGN.md §32), without a GPU: the C ABI (the header, the binding and the library agree; the library exports exactly its header and
needs no other libmbnb_*; every argument error is a status before any device access), the numpy plan of tests/moegemm_cases.py and
the tile bound, the restated glu and routed-sum bodies, the Python surface and the case tables."""
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _moegemm_native as gn, _moemlp_native as mlpn, _mx_native as mxn, _router_native as rn
from mps_bitsandbytes_amd import functional as F
from tests import moegemm_cases as cases
from tests.test_moe_host import _assert_exact_in_any_order, _normal_or_zero, _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_moegemm.h")
CSRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc")
SOURCE = os.path.join(CSRC, "moegemm_kernels.hip")
NAMES = sorted(["mbnb_moegemm_abi_version", "mbnb_moegemm_last_error", "mbnb_moegemm_last_launch", "mbnb_moegemm_plan_bytes", "mbnb_moegemm_plan",
                "mbnb_moegemm_experts", "mbnb_moegemm_gate_up_glu", "mbnb_moegemm_workspace_bytes", "mbnb_moegemm_down_sum"])
INF = float("inf")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_header_binding_and_library_agree():
    lib = gn.lib()
    assert gn.available()
    header = open(HEADER).read()
    assert gn.ABI_VERSION == 1 and lib.mbnb_moegemm_abi_version() == 1
    assert int(re.search(r"#define MBNB_MOEGEMM_ABI_VERSION (\d+)", header).group(1)) == 1
    assert int(re.search(r"#define MBNB_MOEGEMM_ROW_TILE (\d+)", header).group(1)) == gn.ROW_TILE and gn.ROW_TILE % 16 == 0
    assert int(re.search(r"#define MBNB_MOEGEMM_MAX_EXPERTS (\d+)", header).group(1)) == gn.MAX_EXPERTS == 1024
    assert int(re.search(r"#define MBNB_MOEGEMM_MAX_PAIRS (\d+)", header).group(1)) == gn.MAX_PAIRS >= 65536
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_moegemm_\w+)\s*\(", code)))
    assert declared == sorted(gn.EXPORTED_SYMBOLS) == NAMES
    for name, n in (("plan_bytes", 2), ("plan", 6), ("experts", 18), ("gate_up_glu", 19), ("workspace_bytes", 2), ("down_sum", 21)):
        n_args = len(re.search(r"mbnb_moegemm_" + name + r"\(([^)]*)\)", code).group(1).split(","))
        assert n_args == len(gn._SIGNATURES["mbnb_moegemm_" + name][1]) == n, name
    # mbnb_moe_mxfp4_experts's arguments plus the plan, and so for the two of the MLP
    assert gn._SIGNATURES["mbnb_moegemm_experts"][1][:15] == moen._SIGNATURES["mbnb_moe_mxfp4_experts"][1][:15]
    assert gn._SIGNATURES["mbnb_moegemm_gate_up_glu"][1][:16] == mlpn._SIGNATURES["mbnb_moemlp_gate_up_glu"][1][:16]
    assert gn._SIGNATURES["mbnb_moegemm_down_sum"][1][:18] == mlpn._SIGNATURES["mbnb_moemlp_down_sum"][1][:18]
    assert (gn.ERR_ARG, gn.ERR_SHAPE, gn.ERR_WORKSPACE) == (mlpn.ERR_ARG, mlpn.ERR_SHAPE, mlpn.ERR_WORKSPACE)
    assert re.search(r"MBNB_MOEGEMM_ERR_ARG = -1, MBNB_MOEGEMM_ERR_SHAPE = -2, MBNB_MOEGEMM_ERR_WORKSPACE = -3", header)
    assert lib.mbnb_moegemm_last_launch() == b"" or lib.mbnb_moegemm_last_launch().startswith(b"mx_")
    # the ABIs of the libraries this one stands beside did not move
    for mod, version, count in ((moen, 1, 4), (mlpn, 1, 6), (rn, 1, 4), (mxn, 2, None)):
        assert mod.ABI_VERSION == version == getattr(mod.lib(), mod._PREFIX + "_abi_version")()
        assert count is None or len(mod.EXPORTED_SYMBOLS) == count
        assert not [n for n in mod.EXPORTED_SYMBOLS if "moegemm" in n]


def test_the_library_exports_exactly_its_header_and_needs_no_other_library_of_ours():
    assert _exported(gn.LIB_PATH) == NAMES
    assert not [n for n in _exported(moen.LIB_PATH) + _exported(mlpn.LIB_PATH) + _exported(mxn.LIB_PATH) if n.startswith("mbnb_moegemm")]
    needed = subprocess.run(["readelf", "-d", gn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed
    assert not hasattr(gn, "_REQUIRES")


def test_the_makefile_the_build_and_the_source():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*moegemm$", makefile, flags=re.M) and re.search(r"^moegemm_SRCS\s*:=\s*moegemm_kernels\.hip$", makefile, flags=re.M)
    assert "moegemm" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1) and "libmbnb_moegemm.so" in makefile
    assert "-ffp-contract=off" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    after = entry[entry.index("_router_native.lib()"):]
    assert re.search(r"^\s+_moegemm_native\.lib\(\)", after, flags=re.M) and "fourteenth" in entry and "libmbnb_moegemm.so" in entry
    src = open(SOURCE).read()
    for path in (SOURCE, HEADER, gn.__file__):
        text = open(path).read()
        assert "set_kernel_name" not in text and "set_kernel_variant" not in text, path
        assert "atomic" not in text.lower() and "asm" not in text, path
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes == ["../../include/mbnb_moegemm.h", "host.h", "mx_decode.h"]
    assert "mbnb_moegemm_last_launch" in src and "last_launch()" in src
    for kernel in ("k_plan_count", "k_plan_fill", "k_mx_experts_grouped", "k_routed_sum"):
        assert kernel in src, kernel
    shared = open(os.path.join(CSRC, "mx_decode.h")).read()
    for name in ("decode8_16", "mfma16", "scale_value", "load_bias", "store_out", "lane_rank", "check_expert_call"):    # called, not restated
        assert not re.search(r"^(?:__device__ __forceinline__|static(?: inline)?) [\w ]+ " + name + r"\(", src, flags=re.M), name
        assert re.search(r"\b" + name + r"(?:<\w+>)?\(", src) and name in shared, name
    assert "_loader" in open(gn.__file__).read() and "CDLL" not in open(gn.__file__).read()
    assert f"#define MBNB_MOEGEMM_ROW_TILE {cases.R}" in open(HEADER).read() and re.search(r"constexpr int kNT = (\d+);", src).group(1) == str(cases.C // 16)


def _body(text, head):
    """the text between the braces that follow `head`, whitespace normalised"""
    i = text.index("{", text.index(head))
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return " ".join(text[i + 1:j - 1].split())


def test_the_restated_bodies_are_those_of_the_mlp_library():
    mine, theirs = open(SOURCE).read(), open(os.path.join(CSRC, "moemlp_kernels.hip")).read()
    head = "__device__ __forceinline__ float glu(float g, float u, float alpha, float limit)"
    assert _body(mine, head) == _body(theirs, head) and "expf(-t)" in _body(mine, head)
    loop = "for (int a = 0; a < A; ++a)"
    assert _body(mine, loop) == _body(theirs, loop) and "__builtin_fmaf(load_bias(rw, rw_dtype, p), ws[p * N + n], acc)" in _body(mine, loop)
    whole = "void k_routed_sum("
    assert _body(mine, whole) == _body(theirs, whole)


def test_argument_errors_are_a_status_before_any_device_access():
    lib = gn.lib()
    err = lambda: lib.mbnb_moegemm_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first
    BIG = 1 << 40

    def exp(x=P, T=4, A=2, slot=0, K=64, xd=1, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, out=P, od=1, plan=P, pb=BIG):
        return lib.mbnb_moegemm_experts(x, T, A, slot, K, xd, w, s, E, N, ids, bias, bd, out, od, plan, pb, None)

    def glu(x=P, T=4, A=2, K=64, xd=1, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, alpha=1.702, limit=7.0, out=P, od=1, plan=P, pb=BIG):
        return lib.mbnb_moegemm_gate_up_glu(x, T, A, K, xd, w, s, E, N, ids, bias, bd, alpha, limit, out, od, plan, pb, None)

    def down(x=P, T=4, A=2, K=64, xd=1, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, rw=P, rd=2, out=P, od=1, ws=P, wb=BIG, plan=P, pb=BIG):
        return lib.mbnb_moegemm_down_sum(x, T, A, K, xd, w, s, E, N, ids, bias, bd, rw, rd, out, od, ws, wb, plan, pb, None)

    for f in (exp, glu, down):
        assert f(xd=7) == gn.ERR_ARG and b"dtype" in err()
        assert f(xd=-1) == gn.ERR_ARG and b"dtype" in err()
        assert f(od=3) == gn.ERR_ARG and b"dtype" in err()
        assert f(bias=P, bd=9) == gn.ERR_ARG and b"dtype" in err()
        assert f(xd=2) == gn.ERR_ARG and b"16-bit activations" in err()
        assert f(K=80) == gn.ERR_SHAPE and b"multiple" in err()
        assert f(K=0) == gn.ERR_SHAPE and f(K=-32) == gn.ERR_SHAPE
        assert f(E=0) == gn.ERR_SHAPE and f(E=-1) == gn.ERR_SHAPE
        assert f(N=0) == gn.ERR_SHAPE and f(N=-3) == gn.ERR_SHAPE
        assert f(T=-1) == gn.ERR_SHAPE and f(A=-1) == gn.ERR_SHAPE
        # MAX_EXPERTS and MAX_PAIRS pass the shape checks (the next refusal is the NULL ids); one more does not
        assert f(E=gn.MAX_EXPERTS, ids=None) == gn.ERR_ARG and b"NULL" in err()
        assert f(E=gn.MAX_EXPERTS + 1) == gn.ERR_SHAPE and b"experts" in err()
        assert f(T=gn.MAX_PAIRS // 4, A=4, ids=None) == gn.ERR_ARG and b"NULL" in err()
        assert f(T=gn.MAX_PAIRS, A=1, ids=None) == gn.ERR_ARG and b"NULL" in err()
        assert f(T=gn.MAX_PAIRS + 1, A=1) == gn.ERR_SHAPE and b"pairs" in err()
        assert f(T=1, A=gn.MAX_PAIRS + 1) == gn.ERR_SHAPE and b"pairs" in err()
        assert f(T=2 ** 40, A=2 ** 40) == gn.ERR_SHAPE and b"pairs" in err()
        # sizes within one launch (under them the grid, ceil(N / C) x max_tiles, stays below 2^31)
        assert f(E=2 ** 10, K=2 ** 10, N=2 ** 20) == gn.ERR_SHAPE and b"exceed" in err()
        assert f(E=4, K=2 ** 10, N=2 ** 30) == gn.ERR_SHAPE and b"exceed" in err()
        assert f(E=1, K=32, T=gn.MAX_PAIRS, A=1, N=2 ** 19) == gn.ERR_SHAPE and b"exceed" in err()
        assert f(ids=P + 2) == gn.ERR_ARG and b"misaligned" in err() and b"ids" in err()
        assert f(w=P + 2) == gn.ERR_ARG and b"misaligned" in err()
        assert f(x=P + 8) == gn.ERR_ARG and b"misaligned" in err()
        assert f(out=P + 1) == gn.ERR_ARG and b"misaligned" in err()
        assert f(out=P + 2, od=2) == gn.ERR_ARG and b"misaligned" in err()
        assert f(bias=P + 2, bd=2) == gn.ERR_ARG and b"misaligned" in err()
        for name in ("x", "w", "s", "ids", "out"):
            assert f(**{name: None}) == gn.ERR_ARG and b"NULL" in err(), name
        # the plan: NULL or short is the workspace status, exactly plan_bytes passes, and it lies on 16 bytes
        need = lib.mbnb_moegemm_plan_bytes(8, 3)
        assert need == cases.plan_bytes(8, 3) == 256
        assert f(plan=None) == gn.ERR_WORKSPACE and b"plan" in err()
        assert f(pb=need - 1) == gn.ERR_WORKSPACE and f(pb=0) == gn.ERR_WORKSPACE and f(pb=-1) == gn.ERR_WORKSPACE
        assert f(pb=need, ids=P + 2) == gn.ERR_ARG and b"ids" in err()
        assert f(plan=P + 8) == gn.ERR_ARG and b"misaligned" in err() and b"plan" in err()
        # empty work: a no-op success, pointers unread
        assert f(T=0, x=None, w=None, s=None, ids=None, out=None, plan=None, pb=0) == 0
        assert f(A=0, x=None, w=None, s=None, ids=None, out=None, plan=None, pb=0) == 0
    assert glu(N=2 ** 40) == gn.ERR_SHAPE
    for bad in (INF, -INF, float("nan")):
        assert glu(alpha=bad) == gn.ERR_ARG and b"alpha" in err(), bad
    for bad in (0.0, -0.0, -7.0, -INF, float("nan")):
        assert glu(limit=bad) == gn.ERR_ARG and b"limit" in err(), bad
    assert glu(limit=INF, alpha=0.0, ids=None) == gn.ERR_ARG and b"NULL" in err()
    assert down(rd=3) == gn.ERR_ARG and b"dtype" in err() and down(rd=-1) == gn.ERR_ARG
    assert down(rw=None) == gn.ERR_ARG and b"NULL" in err()
    assert down(rw=P + 2, rd=2) == gn.ERR_ARG and b"misaligned" in err()
    need = lib.mbnb_moegemm_workspace_bytes(8, 8)
    assert need == 256
    assert down(wb=need - 1) == gn.ERR_WORKSPACE and b"workspace" in err()
    assert down(wb=0) == gn.ERR_WORKSPACE and down(ws=None) == gn.ERR_WORKSPACE and b"workspace" in err()
    assert down(ws=P + 8) == gn.ERR_ARG and b"misaligned" in err() and b"workspace" in err()
    assert down(wb=need, ids=P + 2) == gn.ERR_ARG and b"ids" in err()

    # the plan's own entry point
    def plan(ids=P, n=8, E=3, out=P, pb=BIG):
        return lib.mbnb_moegemm_plan(ids, n, E, out, pb, None)

    assert plan(n=-1) == gn.ERR_SHAPE and plan(n=gn.MAX_PAIRS + 1) == gn.ERR_SHAPE and b"pairs" in err()
    assert plan(E=0) == gn.ERR_SHAPE and plan(E=gn.MAX_EXPERTS + 1) == gn.ERR_SHAPE and b"experts" in err()
    assert plan(n=gn.MAX_PAIRS, E=gn.MAX_EXPERTS, ids=None) == gn.ERR_ARG and b"NULL" in err()
    assert plan(out=None) == gn.ERR_WORKSPACE and plan(pb=255) == gn.ERR_WORKSPACE and b"plan" in err()
    assert plan(pb=256, ids=P + 2) == gn.ERR_ARG and b"misaligned" in err()
    assert plan(out=P + 8) == gn.ERR_ARG and b"misaligned" in err()
    assert plan(n=0, ids=None, out=None, pb=0) == 0
    with pytest.raises(RuntimeError, match="status -3"):
        gn.check(-3, "unit")


def test_plan_bytes_and_workspace_bytes():
    f, w = gn.lib().mbnb_moegemm_plan_bytes, gn.lib().mbnb_moegemm_workspace_bytes
    for P, E in ((0, 1), (1, 1), (63, 5), (64, 5), (65, 5), (1024, 128), (16384, 32), (16384, 128), (2049, 1024), (gn.MAX_PAIRS, gn.MAX_EXPERTS)):
        assert f(P, E) == cases.plan_bytes(P, E) == gn.plan_bytes(P, E), (P, E)
        assert cases.plan_words(P, E) == E + 2 + 3 * gn.max_tiles(P, E) + P
    assert f(-1, 3) == gn.ERR_SHAPE and f(gn.MAX_PAIRS + 1, 3) == gn.ERR_SHAPE and f(8, 0) == gn.ERR_SHAPE and f(8, gn.MAX_EXPERTS + 1) == gn.ERR_SHAPE
    assert [w(1, 1), w(1, 64), w(1, 65), w(16, 2880), w(16384, 2880), w(0, 8)] == [256, 256, 512, 16 * 2880 * 4, 16384 * 2880 * 4, 0]
    assert gn.workspace_bytes(15, 17) == 1024
    assert w(gn.MAX_PAIRS, 8) == gn.MAX_PAIRS * 32 and w(gn.MAX_PAIRS + 1, 8) == gn.ERR_SHAPE and w(-1, 8) == gn.ERR_SHAPE and w(1, 0) == gn.ERR_SHAPE
    assert w(gn.MAX_PAIRS, 2 ** 19) == gn.ERR_SHAPE
    with pytest.raises(RuntimeError, match="status -2"):
        gn.plan_bytes(gn.MAX_PAIRS + 1, 3)
    # the sizes the Python layer asks for stay below ~200 MB at N = 2880
    assert w(F.MOE_GROUPED_MAX_PAIRS, 2880) < 200e6 and F.MOE_GROUPED_MAX_PAIRS * 2880 * 2 < 200e6 and F.MOE_GROUPED_MAX_PAIRS == 16384


# ----------------------------------------------------------------------------- the plan
def _check_plan(plan, ids, E, r):
    flat = np.asarray(ids).reshape(-1).astype(np.int64)
    P = flat.size
    counts, tiles, order = plan["counts"], plan["tiles"], plan["sorted"]
    assert sorted(order.tolist()) == list(range(P))
    inside = (flat >= 0) & (flat < E)
    assert plan["n_listed"] == int(inside.sum()) == int(counts.sum())
    listed = order[:plan["n_listed"]]
    assert (np.diff(flat[listed]) >= 0).all() and inside[listed].all()
    same = np.diff(flat[listed]) == 0
    assert (np.diff(listed)[same] > 0).all() and (np.diff(order[plan["n_listed"]:]) > 0).all()
    assert plan["n_tiles"] == len(tiles) == sum(-(-int(c) // r) for c in counts) <= cases.max_tiles(P, E, r)
    covered = []
    for e, first, rows in tiles.tolist():
        assert 1 <= rows <= r and (flat[order[first:first + rows]] == e).all()
        covered += list(range(first, first + rows))
    assert covered == list(range(plan["n_listed"]))
    assert (np.diff(tiles[:, 0]) >= 0).all() if len(tiles) else True


def test_the_tile_bound_holds_for_every_count_vector():
    """Exhaustively over every count vector of P <= 9 pairs on E <= 4 experts (the rest outside) at R of 1 to 4; the bound is met with
    equality, so no smaller one of this form holds"""
    tight = 0
    for r, E in itertools.product((1, 2, 3, 4), (1, 2, 3, 4)):
        for counts in itertools.product(range(10), repeat=E):
            if sum(counts) > 9:
                continue
            for outside in (0, 1):
                P = sum(counts) + outside
                n = sum(-(-c // r) for c in counts)
                assert n <= cases.max_tiles(P, E, r), (r, counts, outside)
                tight += n == cases.max_tiles(P, E, r)
    assert tight > 0
    rng = np.random.default_rng(42000)
    for i in range(200):                                     # random routings at the real R, skewed ones among them
        E = int(rng.choice((1, 2, 5, 32, 128, 1024)))
        P = int(rng.integers(1, 5000))
        ids = rng.integers(-1, E + 1, size=P)
        if i % 3 == 0:
            ids = np.where(rng.random(P) < 0.8, rng.integers(0, E), ids)
        plan = cases.plan_reference(ids, E)
        assert plan["n_tiles"] <= cases.max_tiles(P, E) and plan["n_tiles"] == len(plan["tiles"])
    worst = np.concatenate([np.repeat(np.arange(32), 1), np.zeros(64 * 7, dtype=np.int64)])       # every expert once, the rest in whole tiles
    assert cases.plan_reference(worst, 32)["n_tiles"] == 32 + 7 == cases.max_tiles(worst.size, 32) - (1 if worst.size // 64 > 7 else 0)


def test_the_numpy_plan_on_small_routings_and_on_the_listed_cases():
    for r in (1, 2, 3):
        for E in (1, 2, 3):
            for ids in itertools.product(range(-1, E + 1), repeat=4):
                _check_plan(cases.plan_reference(np.array(ids), E, r), np.array(ids), E, r)
    table = cases.plan_cases()
    assert {ids.size for _, ids in table} >= {1, 63, 64, 65, 1024, 1025, 2049} and {E for E, _ in table} == {1, 2, 5, 9, 128, 1024}
    seen = set()
    for E, ids in table:
        assert ids.dtype == np.int32
        plan = cases.plan_reference(ids, E)
        _check_plan(plan, ids, E, cases.R)
        seen |= set(plan["counts"].tolist())
        words = np.full(cases.plan_words(ids.size, E), -7, dtype=np.int32)           # the layout round trip
        words[:E], words[E], words[E + 1] = plan["counts"], plan["n_tiles"], plan["n_listed"]
        words[E + 2:E + 2 + 3 * plan["n_tiles"]] = plan["tiles"].reshape(-1)
        words[E + 2 + 3 * cases.max_tiles(ids.size, E):] = plan["sorted"]
        assert cases.same_plan(cases.plan_from_words(words, ids.size, E), plan)
    assert seen >= set(cases.EDGE_COUNTS) and cases.EDGE_COUNTS == (0, 1, 63, 64, 65, 129)
    assert any(plan_e == 9 and set(ids.tolist()) >= {-1, 9, 2 ** 31 - 1, -2 ** 31} for plan_e, ids in table)
    assert sum(1 for E, ids in table if cases.plan_reference(ids, E)["n_listed"] == 0) == 4
    assert any((np.count_nonzero(cases.plan_reference(ids, E)["counts"]) == 1 and E > 1 and ids.size > cases.R) for E, ids in table)


# ----------------------------------------------------------------------------- the Python surface
def test_signatures_and_exports():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.matmul_mxfp4_experts_grouped) == params(bnb.matmul_mxfp4_experts) + [("plan", None)]
    assert params(bnb.matmul_mxfp4_experts_grouped_glu) == params(bnb.matmul_mxfp4_experts_glu) + [("plan", None)]
    assert params(bnb.matmul_mxfp4_experts_grouped_sum) == params(bnb.matmul_mxfp4_experts_sum) + [("plan", None)]
    assert params(bnb.matmul_mxfp4_experts_grouped)[:6] == [("input", E), ("weight", E), ("weight_scales", E), ("expert_ids", E), ("bias", None), ("dtype", None)]
    assert params(bnb.moe_grouped_plan) == [("expert_ids", E), ("num_experts", E)]
    for name in ("matmul_mxfp4_experts_grouped", "matmul_mxfp4_experts_grouped_glu", "matmul_mxfp4_experts_grouped_sum", "moe_grouped_plan"):
        assert name in bnb.__all__ and getattr(bnb, name) is getattr(F, name), name
    assert len(bnb.__all__) == len(set(bnb.__all__))
    assert F.MOE_GROUPED_MIN_PAIRS is None or F.MOE_GROUPED_MIN_PAIRS >= 2048
    assert F.MOE_GROUPED_MAX_PAIRS <= gn.MAX_PAIRS and F._grouped_cuts(10, 4) == [(0, 10)] and F._grouped_cuts(4097, 4) == [(0, 4096), (4096, 4097)]
    assert F._grouped_cuts(3, 20000) == [(0, 1), (1, 2), (2, 3)] and F._grouped_cuts(0, 4) == []


def _cpu_operands(E=3, N=8, K=64, T=4, A=2, dtype=torch.bfloat16):
    return (torch.zeros(T, K, dtype=dtype), torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 32, dtype=torch.uint8),
            torch.zeros(T, A, dtype=torch.int32), torch.zeros(T, A))


def test_what_the_three_functions_refuse():
    x, w, s, ids, rw = _cpu_operands()
    h = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    plain, glu, ssum = bnb.matmul_mxfp4_experts_grouped, bnb.matmul_mxfp4_experts_grouped_glu, bnb.matmul_mxfp4_experts_grouped_sum
    for f, inp, tail in ((plain, x, ()), (plain, h, ()), (glu, x, ()), (ssum, h, (rw,))):
        with pytest.raises(ValueError, match="cuda"):        # well-formed operands: the refusal left is the CPU tensor
            f(inp, w, s, ids, *tail)
        with pytest.raises(ValueError, match="cuda"):        # the checkpoint's blocks layout, int64 ids, a bias
            f(inp, w.reshape(3, 8, 2, 16), s, ids.long(), *tail, torch.zeros(3, 8))
        with pytest.raises(ValueError, match="float16 or bfloat16"):
            f(inp.float(), w, s, ids, *tail)
        with pytest.raises(ValueError, match="blocks layout"):
            f(inp, w.reshape(3, 8, 4, 8), s, ids, *tail)
        with pytest.raises(ValueError, match="uint8"):
            f(inp, w.to(torch.int8), s, ids, *tail)
        with pytest.raises(ValueError, match="uint8"):
            f(inp, w[0], s[0], ids, *tail)
        with pytest.raises(ValueError, match="weight_scales"):
            f(inp, w, s[:, :, :1], ids, *tail)
        with pytest.raises(ValueError, match="expert_ids"):
            f(inp, w, s, ids.float(), *tail)
        with pytest.raises(ValueError, match="expert_ids"):
            f(inp, w, s, ids.reshape(-1), *tail)
        with pytest.raises(ValueError, match="does not match expert_ids"):
            f(inp[:3], w, s, ids, *tail)
        with pytest.raises(ValueError, match="bias"):
            f(inp, w, s, ids, *tail, torch.zeros(8))
        with pytest.raises(NotImplementedError, match="inference-only"):
            f(inp.clone().requires_grad_(), w, s, ids, *tail)
        with pytest.raises(NotImplementedError, match="inference-only"):
            f(inp, w, s, ids, *tail, torch.zeros(3, 8, requires_grad=True))
        with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
            f(inp.clone().requires_grad_(), w, s, ids, *tail)
        with pytest.raises(ValueError, match="1025 experts"):
            f(inp, torch.zeros(1025, 8, 32, dtype=torch.uint8), torch.zeros(1025, 8, 2, dtype=torch.uint8), ids, *tail)
    with pytest.raises(ValueError, match="does not match expert_ids"):
        glu(h, w, s, ids)
    with pytest.raises(ValueError, match="does not match expert_ids"):
        ssum(x, w, s, ids, rw)
    with pytest.raises(ValueError, match="come in pairs"):
        glu(x, w[:, :7], s[:, :7], ids)
    for bad in (dict(alpha=INF), dict(alpha=float("nan")), dict(limit=0.0), dict(limit=-1.0), dict(limit=float("nan"))):
        with pytest.raises(ValueError, match="alpha .* finite and limit"):
            glu(x, w, s, ids, **bad)
    with pytest.raises(ValueError, match="routing_weights"):
        ssum(h, w, s, ids, rw[:, :1])
    with pytest.raises(NotImplementedError, match="inference-only"):
        ssum(h, w, s, ids, rw.clone().requires_grad_())
    for bad in (ids.float(), ids.reshape(-1)):
        with pytest.raises(ValueError, match="expert_ids"):
            bnb.moe_grouped_plan(bad, 3)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="experts"):
            bnb.moe_grouped_plan(ids, bad)
    with pytest.raises(ValueError, match="cuda"):
        bnb.moe_grouped_plan(ids, 3)


def test_the_decode_functions_keep_their_route_without_a_threshold(monkeypatch):
    """_takes_grouped: never with None, from the threshold up otherwise, and never past the experts of the grouped library"""
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", None)
    assert not F._takes_grouped(10 ** 6, 32)
    monkeypatch.setattr(F, "MOE_GROUPED_MIN_PAIRS", 2048)
    assert not F._takes_grouped(2047, 32) and F._takes_grouped(2048, 32) and F._takes_grouped(2048, 1024) and not F._takes_grouped(2048, 1025)
    x, w, s, ids, rw = _cpu_operands(T=512, A=4)
    with pytest.raises(ValueError, match="cuda"):
        bnb.matmul_mxfp4_experts(x, w, s, ids)
    with pytest.raises(ValueError, match="cuda"):
        bnb.moe_mlp_mxfp4(x, torch.zeros(3, 16, 32, dtype=torch.uint8), torch.zeros(3, 16, 2, dtype=torch.uint8), None,
                          torch.zeros(3, 64, 4, dtype=torch.uint8), torch.zeros(3, 64, 1, dtype=torch.uint8), None, ids, rw)


# ----------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)))
def test_every_exact_case_is_exact_in_f32_in_any_order(index):
    """the conditions tests/test_moe_host.py asserts for its own cases, on these"""
    case = cases.EXACT_CASES[index]
    E, N, K, T, A, counts, x_dtype, _, _, per_slot = case
    x, w, bias, ids = cases.exact_operands(case, index)
    assert x.shape == ((T, A, K) if per_slot else (T, K)) and ids.shape == (T, A) and ids.dtype == np.int32
    assert np.bincount(ids.reshape(-1), minlength=E).tolist() == list(counts) and len(counts) == E and T * A <= gn.MAX_PAIRS
    rows = x.reshape(-1, K)
    assert (cases.to_dtype(rows, x_dtype).double().numpy() == rows).all()
    codes, scales = cases.quantize_experts(w)
    assert (cases.moe_cases.decode_experts(codes, scales) == w).all()
    w2, c2, s2 = w.reshape(E * N, K), codes.reshape(E * N, -1), scales.reshape(E * N, -1)
    unit = 2.0 ** -4
    total = np.abs(rows) @ np.abs(w2).T + (0 if bias is None else np.abs(bias).reshape(-1)[None, :])
    assert total.max() / unit < 2.0 ** 24, total.max()
    P, scaled = _walk(rows, c2, s2)
    assert (P % 2.0 ** -3 == 0).all() and (scaled % unit == 0).all() and np.abs(P).max() < 2.0 ** 20
    assert (scaled.sum(axis=2) == rows @ w2.T).all()
    assert _normal_or_zero(rows) and _normal_or_zero(P) and _normal_or_zero(scaled) and _normal_or_zero(rows @ w2.T)
    want = cases.moe_cases.reference_f64(x, w, bias, ids)
    assert want.shape == (T * A, N) and _normal_or_zero(want) and (want % unit == 0).all()


def test_the_case_tables_cover_every_listed_size():
    X = cases.EXACT_CASES
    C, R = cases.C, cases.R
    assert {c[1] for c in X} == {1, 15, 16, 17, C - 1, C, C + 1, 2 * C + 1} and {c[2] for c in X} == {32, 64, 96, 128, 160, 1056, 2080}
    assert {(c[6], c[7]) for c in X} == {(xd, od) for xd in cases.X16 for od in cases.DTYPES}
    assert {c[8] for c in X} == {True, False} == {c[9] for c in X}
    assert set().union(*(set(c[5]) for c in X)) >= {0, 1, R - 1, R, R + 1, 2 * R + 1}
    assert all(sum(c[5]) == c[3] * c[4] and len(c[5]) == c[0] for c in X)
    assert [nk for nk in cases.RANDOM_WEIGHTS] == [(17, 2080), (33, 1056)] and cases.RANDOM_E == 9
    assert [t * a for t, a in cases.RANDOM_PAIRS] == [70, 1200, 2049] and len(cases.RANDOM_CASES) == 12
    for ta in cases.RANDOM_PAIRS:
        uniform, skewed = (cases.random_routing(ta, r) for r in cases.RANDOM_ROUTINGS)
        cu, cs = (np.bincount(i[(i >= 0) & (i < 9)].reshape(-1), minlength=9) for i in (uniform, skewed))
        assert cs[0] > 0.6 * skewed.size and cu.max() < 0.3 * uniform.size and (uniform == 9).any() and (skewed == 9).any()
    for off in cases.OFFSETS:
        assert off["x"] % 16 == 0 and off["w_codes"] % 16 == 0 and off["ws"] % 16 == 0 and off["plan"] % 16 == 0
    assert {o["plan"] for o in cases.OFFSETS} == {0, 16, 32, 48}
    T, A, E, H, I = cases.ROUTE_SHAPE
    assert T * A >= 2048 and T * A > mlpn.MAX_PAIRS
    assert cases.experts_text(torch.bfloat16, False, 32, 4096) == "mx_grouped bf16 shared E32 P4096 R64"


# ----------------------------------------------------------------------------- the K walk and the column tiles
def test_the_walk_and_tile_tables_cover_what_they_name():
    C, R = cases.C, cases.R
    assert cases.WALK_KS is cases.moe_cases.WALK_KS and not set(cases.WALK_KS) & {c[2] for c in cases.EXACT_CASES}
    for table, n in ((cases.WALK_CASES, C + 1), (cases.WALK_GLU_CASES, C // 2 + 1), (cases.WALK_SUM_CASES, C + 1)):
        assert [c[2] for c in table] == list(cases.WALK_KS) and all(c[:2] == (3, n) and c[3:6] == (17, 4, (R + 1, 0, 3)) for c in table)
        assert {c[6] for c in table} == set(cases.X16) and {c[7] for c in table} == set(cases.DTYPES) and {c[8] for c in table} == {True, False}
        assert all(table[i][6] != table[i + 1][6] and table[i][7] != table[i + 1][7] for i in range(len(table) - 1))
    assert {c[9] for c in cases.WALK_CASES} == {True, False} and {c[9] for c in cases.WALK_SUM_CASES} == set(cases.DTYPES)
    assert {c[9] for c in cases.WALK_GLU_CASES} == {cases.moemlp_cases.LIMIT, INF}
    plan = cases.plan_reference(cases.exact_operands(cases.WALK_CASES[0], cases.WALK_SEED)[3], 3)
    assert plan["tiles"][:, 0].tolist() == [0, 0, 2] and plan["tiles"][:, 2].tolist() == [R, 1, 3]       # a full tile, a one-row tile
    assert cases.WALK_RANDOM_WEIGHTS == ((17, 2880), (C + 1, 992)) and cases.WALK_RANDOM_PAIRS == (35, 2)
    assert not set(cases.WALK_RANDOM_WEIGHTS) & set(cases.RANDOM_WEIGHTS)
    assert cases.TILE_CASES == [("glu", C - 2), ("glu", C), ("glu", C + 2), ("glu", 2 * C + 2), ("down", C - 1), ("down", C), ("down", C + 1), ("down", 2 * C + 1)]
    assert [n // 2 for f, n in cases.TILE_CASES if f == "glu"] == [23, 24, 25, 49] and cases.TILE_K == 160
    ids = cases.tile_ids()
    flat = ids.reshape(-1).astype(np.int64)
    assert ids.shape == (cases.TILE_T, cases.TILE_A) and ids.dtype == np.int32
    assert np.bincount(flat[(flat >= 0) & (flat < cases.TILE_E)], minlength=cases.TILE_E).tolist()[:5] == [0, 1, R - 1, R, R + 1]
    assert sorted(flat[(flat < 0) | (flat >= cases.TILE_E)].tolist()) == [-2 ** 31, -1, cases.TILE_E, 2 ** 31 - 1]
    assert cases.TILE_ALL_OUTSIDE == (("glu", 2 * C + 2), ("plain", 2 * C + 1), ("down", 2 * C + 1))
    (E1, N1, K1, T1, A1, c1), (E2, N2, K2, T2, A2, c2) = cases.MANY_CASES
    assert (E1, N1, K1) == (128, C + 1, 64) and (E2, N2, K2) == (gn.MAX_EXPERTS, 1, 32) == (mlpn.MAX_EXPERTS, 1, 32)
    for (E, N, K, T, A, counts) in cases.MANY_CASES:
        assert len(counts) == E and sum(counts) == T * A and counts[0] and counts[-1] and sum(1 for c in counts if c) < 8
    assert E1 * (C + 1) * 32 == 128 * 49 * 32                  # the largest weight of these tables, in bytes


def _close(rows, x_dtype, w, bias, ids, unit):
    """rows exact in their 16-bit type, weights that quantise to their own codes, every block's partial sum a multiple of the unit,
    the sum of the magnitudes below 2^24 units: every order of the f32 sums gives the float64 result"""
    E, N, K = w.shape
    flat = rows.reshape(-1, K)
    assert (cases.to_dtype(flat, x_dtype).double().numpy() == flat).all()
    codes, scales = cases.quantize_experts(w)
    assert (cases.moe_cases.decode_experts(codes, scales) == w).all()
    w2 = w.reshape(E * N, K)
    total = np.abs(flat) @ np.abs(w2).T + (0 if bias is None else np.abs(bias).reshape(-1)[None, :])
    assert total.max() / unit < 2.0 ** 24, total.max()
    blocks = np.einsum("mbk,nbk->mnb", flat.reshape(flat.shape[0], -1, 32), w2.reshape(E * N, -1, 32))
    assert (blocks % unit == 0).all() and _normal_or_zero(blocks) and (blocks.sum(axis=2) == flat @ w2.T).all()
    pre = cases.moe_cases.reference_f64(rows, w, bias, ids)
    assert (pre % unit == 0).all() and (pre.astype(np.float32) == pre).all()
    return pre


@pytest.mark.parametrize("index", range(len(cases.WALK_KS)))
def test_every_walk_case_of_the_three_forms_is_exact_in_f32_in_any_order(index):
    assert 3104 * 144 / 2.0 ** -4 < 2.0 ** 24                 # the worst case of lossless rows at the longest K
    case = cases.WALK_CASES[index]
    x, w, bias, ids = cases.exact_operands(case, cases.WALK_SEED + index)
    _assert_exact_in_any_order(case, x, w, bias, ids)
    case = cases.WALK_GLU_CASES[index]
    x, w, bias, ids = cases.glu_operands(case, cases.WALK_SEED + index)
    pre = _close(x, case[6], w, bias, ids, 2.0 ** -7)
    assert w.shape[1] == cases.C + 2 and (np.abs(pre) < 7.0).any() and (pre > 7.0).any() and (pre < -7.0).any()
    case = cases.WALK_SUM_CASES[index]
    h, w, bias, ids, rw = cases.sum_operands(case, cases.WALK_SEED + index)
    _close(h, case[6], w, bias, ids, 2.0 ** -7)
    for dtype in cases.DTYPES:
        assert (cases.to_dtype(rw, dtype).double().numpy() == rw).all()


def test_the_tile_and_many_expert_cases_are_exact_in_f32_in_any_order():
    for form, N in cases.TILE_CASES:
        rows, w, bias, ids, rw = cases.tile_operands(form, N)
        inside = np.where((ids >= 0) & (ids < cases.TILE_E), ids, 0)
        pre = _close(rows, torch.float16, w, bias, inside, 2.0 ** -7)
        _close(rows, torch.bfloat16, w, bias, inside, 2.0 ** -7)
        assert (bias != 0).all() and w.shape == (cases.TILE_E, N, cases.TILE_K)
        if form == "glu":
            assert (np.abs(pre) < 7.0).any() and (pre > 7.0).any() and (pre < -7.0).any()
    for index, case in enumerate(cases.MANY_CASES):
        for form in ("plain", "glu", "down"):
            rows, w, bias, ids, rw = cases.many_operands(case, index, form)
            _close(rows, torch.bfloat16, w, bias, ids, 2.0 ** -7)
            assert w.shape[1] == case[1] + (form == "glu") and np.bincount(ids.reshape(-1), minlength=case[0]).tolist() == list(case[5])


# ----------------------------------------------------------------------------- the kernel restated, and the mistakes the tables are for
def _call(form, rows, w, bias, ids, rw=None, alpha=0.0, limit=INF, scales=None):
    codes, s = cases.quantize_experts(w)
    return dict(form=form, x=rows, codes=codes, scales=s if scales is None else scales, ids=ids, bias=bias, rw=rw, alpha=alpha, limit=limit)


def _planted(ids, E):
    out = ids.copy()
    for (t, a), v in zip(cases.moe_cases.OUT_OF_RANGE_PLACES, cases.moe_cases.OUT_OF_RANGE):
        out[t, a] = np.int64(E if v == cases.moe_cases.IDS_SHAPE[0] else v).astype(np.int32)
    return out


def _nonfinite_calls(x, w, ids, blocks, bad_ks):
    """the bodies of the 0xFF, Inf and NaN tests of tests/test_gpu_moegemm.py as calls: one planted byte or value each"""
    mc = cases.moe_cases
    _, scales = cases.quantize_experts(w)
    out = []
    for b in blocks:
        planted = scales.copy()
        planted[mc.NAN_EXPERT, mc.NAN_COLUMN, b] = 255
        out.append(_call("plain", x, w, None, ids, scales=planted))
    for k in bad_ks:
        for v in mc.X_BAD_VALUES:
            xb = x.copy()
            xb[mc.X_BAD_TOKEN, k] = v
            out.append(_call("plain", xb, w, None, ids))
    return out


def _old_tables():
    """What the suite held before the walk and tile tables: EXACT_CASES (plain), the non-finite edges at K = 160, and the shapes at
    which the GLU and the down + sum forms ran (the bit rule's N = 16 and 32, 17 and 33; the edge tests' 16, 8 and 9, with the
    out-of-range ids), here on lossless operands"""
    mc, ml = cases.moe_cases, cases.moemlp_cases
    tables = {"EXACT_CASES": [_call("plain", *cases.exact_operands(c, i)) for i, c in enumerate(cases.EXACT_CASES)]}
    x, w, ids = mc.nan_operands()
    tables["non-finite, K = 160"] = _nonfinite_calls(x, w, ids, mc.NAN_BLOCKS, mc.X_BAD_KS)
    forms = []
    for i, (N, K) in enumerate(cases.RANDOM_WEIGHTS):
        T, A = cases.RANDOM_PAIRS[0]
        ids = cases.random_routing((T, A), "uniform")
        w = ml.emul.lossless(cases.RANDOM_E * N, K, seed=46000 + i).reshape(cases.RANDOM_E, N, K)
        bias = np.random.default_rng(46100 + i).integers(1, 9, size=(cases.RANDOM_E, N)).astype(np.float64)
        rw = np.random.default_rng(46200 + i).integers(1, 33, size=(T, A)) / 64.0
        forms.append(_call("glu", ml.emul.lossless(T, K, seed=46300 + i) * 0.125, w[:, :N - N % 2], bias[:, :N - N % 2], ids))
        forms.append(_call("down", (ml.emul.lossless(T * A, K, seed=46400 + i) * 0.125).reshape(T, A, K), w, bias, ids, rw))
    E, N, K, T, A = mc.IDS_SHAPE
    x, w, bias, ids = mc.ids_operands()
    rw = np.random.default_rng(46500).integers(1, 33, size=(T, A)) / 64.0
    h = np.repeat(x[:, None, :], A, axis=1)
    for planted in (_planted(ids, E), np.full((T, A), -1, dtype=np.int32)):
        forms += [_call("plain", x, w, bias, planted), _call("glu", x, w[:, :16], bias[:, :16], planted), _call("down", h, w, bias, planted, rw)]
    x, w, ids = mc.nan_operands()
    forms += [_call("glu", x, w[:, :8], None, ids), _call("down", np.repeat(x[:, None, :], ids.shape[1], axis=1), w, None, ids, np.ones(ids.shape))]
    tables["GLU and down, one column tile"] = forms
    return tables


def _new_tables():
    mc = cases.moe_cases
    tables = {"WALK_CASES": [_call("plain", *cases.exact_operands(c, cases.WALK_SEED + i)) for i, c in enumerate(cases.WALK_CASES)],
              "WALK_GLU_CASES": [_call("glu", *cases.glu_operands(c, cases.WALK_SEED + i), limit=c[9]) for i, c in enumerate(cases.WALK_GLU_CASES)],
              "WALK_SUM_CASES": [_call("down", *cases.sum_operands(c, cases.WALK_SEED + i)) for i, c in enumerate(cases.WALK_SUM_CASES)]}
    tables["non-finite on the walk's tails"] = [call for K in cases.WALK_NONFINITE_KS
                                                for call in _nonfinite_calls(*mc.walk_nan_operands(K), mc.walk_nan_blocks(K), mc.walk_bad_ks(K))]
    tiles = []
    for form, N in cases.TILE_CASES:
        rows, w, bias, ids, rw = cases.tile_operands(form, N)
        tiles.append(_call(form, rows, w, bias, ids, rw, alpha=0.0, limit=cases.moemlp_cases.LIMIT))
    tables["TILE_CASES"] = tiles
    outside = []
    for form, N in cases.TILE_ALL_OUTSIDE:
        rows, w, bias, ids, rw = cases.tile_operands("glu" if form == "glu" else "down", N)
        outside.append(_call(form, rows, w, bias, np.full(ids.shape, -1, dtype=np.int32), rw))
    tables["TILE_ALL_OUTSIDE"] = outside
    tables["MANY_CASES"] = [_call(form, *cases.many_operands(c, i, form)) for i, c in enumerate(cases.MANY_CASES) for form in ("plain", "glu", "down")]
    return tables


def _restated(call, mutate=None):
    return cases.grouped_as_kernel(call["x"], call["codes"], call["scales"], call["ids"], call["bias"], call["form"], mutate, call["alpha"], call["limit"], call["rw"])


def test_the_restated_kernel_is_the_float64_reference_and_the_new_tables_catch_what_the_old_ones_let_through():
    """grouped_as_kernel, unmutated, equals the float64 reference on every exact table, old and new.  Then every mutation on every
    table: which tables see it.  Written down (the matrix is printed):
      - the new tables catch every mutation that changes a result;
      - "tail_keeps_w" changes none: the activation of a block past K is zeroed too, so its products are 0 whatever the weight
        registers hold, and the two zeroings of the kernel guard each other.  No table can catch it; it is asserted to be silent;
      - "steps_floor" and "tail_only_wave_idle" were caught before (K = 32 to 96 are one ragged step on wave 0, K = 160 a ragged
        step alone on wave 1); "tail_past_wave_1" and "three_passes" are what the old K set really left open: a ragged step on
        waves 2 to 7, and a fourth pass;
      - "tail_keeps_x_and_scale" shows only through a non-finite activation in the clamped block (Inf x 0), at k = K - 1: the old
        K = 160 edge saw it on wave 1, the new ones see it on waves 6 and 7;
      - the three epilogue mutations and the two above pass every old table."""
    old, new = _old_tables(), _new_tables()
    wants = {}
    for name, table in {**old, **new}.items():
        wants[name] = []
        for call in table:
            want = cases.reference(call["form"], call["x"], call["codes"], call["scales"], call["ids"], call["bias"], call["alpha"], call["limit"], call["rw"])
            assert cases.same_values(_restated(call), want), (name, call["form"], call["codes"].shape)
            wants[name].append(want)
    matrix = {m: {name: any(not cases.same_values(_restated(call, m), want) for call, want in zip(table, wants[name]))
                  for name, table in {**old, **new}.items()} for m in cases.MUTANTS}
    for m in cases.MUTANTS:
        print(f"mutation {m}: caught by " + (", ".join(name for name, hit in matrix[m].items() if hit) or "no table"))
    by_old = {m for m in cases.MUTANTS if any(matrix[m][name] for name in old)}
    by_new = {m for m in cases.MUTANTS if any(matrix[m][name] for name in new)}
    assert by_new == set(cases.MUTANTS) - {"tail_keeps_w"} and "tail_keeps_w" not in by_old
    assert by_old == {"steps_floor", "tail_only_wave_idle", "tail_keeps_x_and_scale"}
    assert not by_old & {"glu_column_forgets_n0", "zeros_on_column_tile_0", "workspace_stride_of_a_tile", "tail_past_wave_1", "three_passes"}
    exact_new = [name for name in new if name != "non-finite on the walk's tails"]
    assert all(any(matrix[m][name] for name in exact_new) for m in by_new - {"tail_keeps_x_and_scale"})
    assert matrix["three_passes"]["WALK_CASES"] and matrix["tail_past_wave_1"]["WALK_GLU_CASES"] and matrix["workspace_stride_of_a_tile"]["WALK_SUM_CASES"]
    assert matrix["glu_column_forgets_n0"]["TILE_CASES"] and matrix["zeros_on_column_tile_0"]["TILE_CASES"] and matrix["zeros_on_column_tile_0"]["TILE_ALL_OUTSIDE"]
