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
from tests.test_moe_host import _normal_or_zero, _walk

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
