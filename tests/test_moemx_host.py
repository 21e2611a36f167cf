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
