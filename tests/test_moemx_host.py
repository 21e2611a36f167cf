"""CPU-side checks of libmbnb_moemx.so: header, binding and exports; argument errors before any device access; the keyword."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moegemm_native as gn, _moemx_native as xn, _mx_native as mxn
from tests import moemx_cases as cases, mx_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_exports_agree():
    lib, header = xn.lib(), open(os.path.join(ROOT, "include", "mbnb_moemx.h")).read()
    assert xn.available() and xn.ABI_VERSION == 1 == lib.mbnb_moemx_abi_version()
    for name, value in (("ABI_VERSION", 1), ("ROW_TILE", cases.R), ("COL_TILE", cases.CT), ("K_STEP", cases.KS), ("MAX_EXPERTS", gn.MAX_EXPERTS),
                        ("MAX_PAIRS", gn.MAX_PAIRS)):
        assert int(re.search(rf"#define MBNB_MOEMX_{name} (\d+)", header).group(1)) == value == getattr(xn, name), name
    assert xn.ROW_TILE == gn.ROW_TILE and (xn.FP4, xn.FP8) == (mxn.ELEM_CODE["fp4"], mxn.ELEM_CODE["fp8"])
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_moemx_\w+)\s*\(", code)))
    out = subprocess.run(["nm", "-D", "--defined-only", xn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert declared == sorted(xn.EXPORTED_SYMBOLS) == sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))
    assert len(re.search(r"mbnb_moemx_experts\(([^)]*)\)", code).group(1).split(",")) == len(xn._SIGNATURES["mbnb_moemx_experts"][1]) == 19


def test_argument_errors_are_a_status_before_any_device_access():
    lib, err = xn.lib(), xn.lib().mbnb_moemx_last_error
    P, BIG = 4096, 1 << 40                                   # an aligned address that is never dereferenced: every call below fails first

    def f(x=P, xs=P, act=xn.FP8, T=4, A=2, slot=0, K=64, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, out=P, od=1, plan=P, pb=BIG):
        return lib.mbnb_moemx_experts(x, xs, act, T, A, slot, K, w, s, E, N, ids, bias, bd, out, od, plan, pb, None)

    assert f(act=2) == xn.ERR_ARG and f(act=-1) == xn.ERR_ARG and b"act_elem" in err()
    assert f(od=3) == xn.ERR_ARG and b"dtype" in err() and f(bias=P, bd=9) == xn.ERR_ARG and b"dtype" in err()
    assert f(K=80) == xn.ERR_SHAPE and b"multiple" in err() and f(K=0) == xn.ERR_SHAPE
    assert f(E=0) == xn.ERR_SHAPE and f(N=0) == xn.ERR_SHAPE and f(T=-1) == xn.ERR_SHAPE and f(A=-1) == xn.ERR_SHAPE
    assert f(E=xn.MAX_EXPERTS, ids=None) == xn.ERR_ARG and b"NULL" in err()
    assert f(E=xn.MAX_EXPERTS + 1) == xn.ERR_SHAPE and b"experts" in err()
    assert f(T=xn.MAX_PAIRS, A=1, ids=None) == xn.ERR_ARG and b"NULL" in err()
    assert f(T=xn.MAX_PAIRS + 1, A=1) == xn.ERR_SHAPE and b"pairs" in err() and f(T=2 ** 40, A=2 ** 40) == xn.ERR_SHAPE
    assert f(E=1, K=32, T=xn.MAX_PAIRS, A=1, N=2 ** 19) == xn.ERR_SHAPE and b"exceed" in err()
    for name in ("x", "xs", "w", "s", "ids", "out"):
        assert f(**{name: None}) == xn.ERR_ARG and b"NULL" in err(), name
    for bad in (dict(x=P + 8), dict(w=P + 2), dict(ids=P + 2), dict(out=P + 1), dict(out=P + 2, od=2), dict(bias=P + 2, bd=2), dict(plan=P + 8)):
        assert f(**bad) == xn.ERR_ARG and b"misaligned" in err(), bad
    need = gn.lib().mbnb_moegemm_plan_bytes(8, 3)
    assert f(plan=None) == xn.ERR_ARG and b"plan" in err()
    assert f(pb=need - 1) == xn.ERR_WORKSPACE and b"plan" in err() and f(pb=0) == xn.ERR_WORKSPACE
    assert f(pb=need, ids=P + 2) == xn.ERR_ARG and b"ids" in err()     # exactly the plan's bytes pass
    for empty in (dict(T=0), dict(A=0)):
        assert f(x=None, xs=None, w=None, s=None, ids=None, out=None, plan=None, pb=0, **empty) == 0


CSRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc")


def _csrc():
    return {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


def _calls(text, name):
    return len(re.findall(r"\b" + name + r"(?:<[^>]*>)?\(", text))


def _between(text, start, end):
    """the text from `start` up to `end`, whitespace normalised"""
    i = text.index(start)
    return " ".join(text[i:text.index(end, i)].split())


def test_the_scaled_mfma_tile_is_defined_once_for_the_linear_and_the_experts():
    """the stage, the LDS-DMA, the fold of a NaN mask, the scaled MFMA and the epilogue value stand in csrc/mx_scaled.h and nowhere
    else; k_gemm_mx and k_mx_experts_scaled include it, call them and define none.  The fragment reads, the zeros past K and the
    loop over the ballots are written out in both kernels (as helpers they changed the instruction streams): their
    texts are held equal here"""
    files, users = _csrc(), ["moemx_kernels.hip", "mx_kernels.hip"]
    shared = files["mx_scaled.h"]
    assert "__builtin_amdgcn_global_load_lds(" in shared and not any("__builtin_amdgcn_global_load_lds(" in files[name] for name in users)
    for text in ("__builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(", "uint32_t fold16(",
                 "(b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xFFFFu", "((a_nan >> row_bit) & 1u)) v = __uint_as_float(0x7FC00000u);",
                 "typedef int v8i", "struct ScaledStage", "A8 ? 0 : 4, BLGP = 4", "void dma16(", "v4f scaled_mfma(", "float scaled_value("):
        assert [name for name, body in files.items() if text in body] == ["mx_scaled.h"] and shared.count(text) == 1, text
    assert [name for name, body in files.items() if '#include "mx_scaled.h"' in body] == users
    assert "asm" not in shared and "namespace mbnb" in shared and '#include "mx_decode.h"' in shared
    assert "float v = acc + b;" in shared
    for name in users:
        src = files[name]
        assert _calls(src, "scaled_mfma") == 1 == _calls(src, "scaled_value") and _calls(src, "dma16") == 2 == _calls(src, "fold16"), name
        assert len(re.findall(r"\bScaledStage<", src)) == 1 and "A_BYTES = S::A_BYTES" in src, name
        for helper in ("dma16", "fold16", "scaled_mfma", "scaled_value"):
            assert not re.search(r"^[^/\n]*(?:__device__|auto) [\w ]*\b" + helper + r"\b\s*(?:\(|=)", src, flags=re.M), (name, helper)
    # what stays written out is the same text in both kernels, but for the names of the tile's first rows and the expert kernel's dead rows
    lin, exp = files["mx_kernels.hip"], files["moemx_kernels.hip"]
    rule = "const bool lo_out = k0 + (A8 ? 16 : 32) * g >= K, hi_out = k0 + 64 + 16 * g >= K, b_out = k0 + 32 * g >= K;"
    assert lin.count(rule) == 1 == exp.count(rule) and sum(body.count("lo_out =") for body in files.values()) == 2
    zeros = _between(exp, rule, "a_nan[i] |=").replace(" || !a_live[i]", "").replace(" || !b_live[i]", "")
    assert _between(lin, rule, "a_nan[i] |=") == zeros and "if (hi_out) af[i][4 + q] = 0;" in zeros
    masks = "a_nan[i] |= fold16(__ballot(sa[i] == kNaNScale)); b_nan[i] |= fold16(__ballot(sb[i] == kNaNScale));"
    for src in (lin, exp):
        assert masks in " ".join(src.split())
    reads = _between(lin, "v8i af[4], bf[4];", "if (t == nk - 1 && K % KS)")
    for mine, theirs in (("wm * 64 + i * 16 + fr", "16 * i + fr"), ("wn * 64 + j * 16 + fr", "64 * wave + 16 * j + fr"), ("TM * 4", "kRowTile * 4")):
        assert mine in reads
        reads = reads.replace(mine, theirs)
    assert reads == _between(exp, "v8i af[4], bf[4];", "use_scales(t, sa_next")


def test_the_plan_layout_and_the_grouped_checks_are_defined_once_for_both_libraries():
    """the plan's word layout, its size, the accessor and the shape checks of a grouped call stand in csrc/mx_plan.h and nowhere
    else; moegemm_kernels.hip and moemx_kernels.hip include it, call them and define none; both refusals of a plan keep their words"""
    files, users = _csrc(), ["moegemm_kernels.hip", "moemx_kernels.hip"]
    shared = files["mx_plan.h"]
    for text in ("max_tiles_of(int64_t", "plan_words(int64_t", "plan_bytes_of(int64_t", "(E < P ? E : P) + P / kPlanRowTile",
                 "E + 2 + 3 * max_tiles_of(P, E) + P", "plan + E + 2", "tiles + 3 * (int64_t)max_tiles", "plan + E + 1", "tiles[3 * t + 2]",
                 "int check_grouped_call(", "int check_plan(", "kPlanMaxPairs);", "(N + col_tile - 1) / col_tile", "the plan %s %lld bytes, %lld needed", "constexpr int kPlanRowTile = 64;"):
        assert [name for name, body in files.items() if text in body] == ["mx_plan.h"] and shared.count(text) == 1, text
    assert [name for name, body in files.items() if '#include "mx_plan.h"' in body] == users
    assert "check_expert_call(what, 0, 0, K, row_dtype, E, N, bias_dtype, has_bias, out_dtype, kPlanMaxExperts, true)" in shared
    for name in users:
        src, lib = files[name], "MOEGEMM" if name.startswith("moegemm") else "MOEMX"
        assert "plan[E" not in src and "plan + E" not in src and "round256" not in src and _calls(src, "check_expert_call") == 0, name
        assert _calls(src, "plan_of") == (2 if lib == "MOEGEMM" else 1) and _calls(src, r"pl\.tile") == 1, name
        assert _calls(src, "check_grouped_call") == (3 if lib == "MOEGEMM" else 1) and _calls(src, "check_plan") == (4 if lib == "MOEGEMM" else 1), name
        for macro, const in (("ROW_TILE", "kPlanRowTile"), ("MAX_PAIRS", "kPlanMaxPairs"), ("MAX_EXPERTS", "kPlanMaxExperts"), ("ERR_WORKSPACE", "kErrPlan")):
            assert f"MBNB_{lib}_{macro} == mbnb::mx::{const}" in src, (name, macro)
    assert files["moegemm_kernels.hip"].count('plan_bytes, P, E, "is NULL or holds")') == 4
    assert files["moemx_kernels.hip"].count('plan_bytes, P, E, "holds")') == 1
    lib, P, BIG = gn.lib(), 4096, 1 << 40
    need = lib.mbnb_moegemm_plan_bytes(8, 3)
    assert need == cases_plan_bytes(8, 3)
    assert lib.mbnb_moegemm_plan(P, 8, 3, None, BIG, None) == gn.ERR_WORKSPACE
    assert lib.mbnb_moegemm_last_error() == b"mbnb_moegemm_plan: the plan is NULL or holds %d bytes, %d needed" % (BIG, need)
    assert xn.lib().mbnb_moemx_experts(P, P, xn.FP8, 4, 2, 0, 64, P, P, 3, 8, P, None, 0, P, 1, P, need - 1, None) == xn.ERR_WORKSPACE
    assert xn.lib().mbnb_moemx_last_error() == b"mbnb_moemx_experts: the plan holds %d bytes, %d needed" % (need - 1, need)


def cases_plan_bytes(P, E, r=cases.R):
    """the plan's bytes, restated: 4 (E + 2 + 3 (min(E, P) + P // R) + P) rounded up to 256"""
    return -(-4 * (E + 2 + 3 * (min(E, P) + P // r) + P) // 256) * 256


def test_the_keyword_and_the_exact_cases():
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    for bad in ("int8", "fp6", None):
        with pytest.raises(ValueError, match="format"):
            bnb.matmul_mxfp4_experts_scaled(torch.zeros(4, 64, dtype=torch.bfloat16), u8(3, 8, 32), u8(3, 8, 2), u8(4, 2).int(), act_format=bad)
    with pytest.raises(ValueError, match="act_format"):
        bnb.ExpertsMXFP4.from_weights(torch.zeros(3, 8, 64), act_format="int8")
    assert bnb.ExpertsMXFP4.act_format == "none"
    # §25's exactness conditions on the exact GPU cases: the codes hold the values, products are multiples of 2^-4, sums (+ bias) below 2^20
    ids = cases.exact_ids()
    assert sorted(np.bincount(ids[(ids >= 0) & (ids < 3)], minlength=3)) == [0, 1, 65] and ((ids < 0) | (ids >= 3)).sum() == 4
    for K in cases.EXACT_K:
        xv, wv = emul.lossless(70, K, 1), emul.lossless(cases.CT + 1, K, 2)
        for elem in ("fp8", "fp4"):
            assert np.array_equal(emul.decode_f64(*emul.quantize(xv, elem), elem), xv)
        assert np.array_equal(emul.decode_f64(*emul.lossless_codes(wv), "fp4"), wv)
        assert (np.abs(xv) @ np.abs(wv).T).max() + 8 < 2 ** 20
        prod16 = xv[:, None, :] * wv[None, :4, :] * 16
        assert np.array_equal(np.round(prod16), prod16)
