"""CPU-side checks of the expert MLP on libmbnb_moemx.so: its exports, its refusals, the keyword and the module attribute."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moegemm_native as gn, _moemx_native as xn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mbnb_moemx_gate_up_glu": 21, "mbnb_moemx_workspace_bytes": 2, "mbnb_moemx_down_sum": 22}
P, BIG, INF = 4096, 1 << 40, float("inf")                    # P: an aligned address that is never dereferenced: every call below fails first


def test_header_binding_and_exports_agree_on_the_new_entry_points():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbnb_moemx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", xn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert xn.ABI_VERSION == 1 == xn.lib().mbnb_moemx_abi_version()
    for name, count in NEW.items():
        assert len(re.search(name + r"\(([^)]*)\)", code).group(1).split(",")) == len(xn._SIGNATURES[name][1]) == count, name
        assert re.search(r"\b" + name + "$", out, flags=re.M) and name in xn.EXPORTED_SYMBOLS, name
    assert xn.workspace_bytes(70, 17) == -(-70 * 17 * 4 // 256) * 256 and xn.workspace_bytes(0, 5) == 0
    for bad in ((-1, 8), (8, 0), (xn.MAX_PAIRS + 1, 8), (xn.MAX_PAIRS, 1 << 30)):
        assert xn.lib().mbnb_moemx_workspace_bytes(*bad) == xn.ERR_SHAPE, bad


def glu(x=P, xs=P, act=xn.FP8, T=4, A=2, K=64, w=P, s=P, E=3, I=32, ids=P, bias=None, bd=0, alpha=1.702, limit=7.0, h=P, hs=P, he=xn.FP8, plan=P, pb=BIG):
    return xn.lib().mbnb_moemx_gate_up_glu(x, xs, act, T, A, K, w, s, E, I, ids, bias, bd, alpha, limit, h, hs, he, plan, pb, None)


def down(h=P, hs=P, act=xn.FP8, T=4, A=2, K=64, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, rw=P, rd=2, out=P, od=1, ws=P, wb=BIG, plan=P, pb=BIG):
    return xn.lib().mbnb_moemx_down_sum(h, hs, act, T, A, K, w, s, E, N, ids, bias, bd, rw, rd, out, od, ws, wb, plan, pb, None)


def test_every_refusal_is_a_status_with_its_text_before_any_device_access():
    err = xn.lib().mbnb_moemx_last_error
    need = gn.lib().mbnb_moegemm_plan_bytes(8, 3)
    for f in (glu, down):                                    # the conventions and the order of mbnb_moemx_experts, through one check_call
        assert f(act=2) == xn.ERR_ARG and b"act_elem" in err() and f(K=80) == xn.ERR_SHAPE and b"multiple" in err()
        assert f(E=xn.MAX_EXPERTS + 1) == xn.ERR_SHAPE and f(T=xn.MAX_PAIRS + 1, A=1) == xn.ERR_SHAPE and b"pairs" in err()
        assert f(ids=None) == xn.ERR_ARG and b"NULL ids" in err() and f(w=P + 2) == xn.ERR_ARG and b"misaligned w_codes" in err()
        assert f(plan=None) == xn.ERR_ARG and f(pb=need - 1) == xn.ERR_WORKSPACE and b"the plan holds" in err()
        assert f(pb=need, ids=P + 2) == xn.ERR_ARG and b"misaligned ids" in err()
        for empty in (dict(T=0), dict(A=0)):                 # a no-op success with unread pointers
            assert f(w=None, s=None, ids=None, plan=None, pb=0, **empty) == 0
    # the gate / up launch's own
    assert glu(I=0) == xn.ERR_SHAPE and glu(I=-32) == xn.ERR_SHAPE and glu(I=1 << 62) == xn.ERR_SHAPE
    for I in (1, 16, 48, 2880 + 16):
        assert glu(I=I) == xn.ERR_SHAPE and b"I = %d is not a multiple of the MX block" % I in err()
    for alpha in (INF, -INF, float("nan")):
        assert glu(alpha=alpha) == xn.ERR_ARG and b"alpha" in err() and b"finite" in err()
    for limit in (0.0, -1.0, -INF, float("nan")):
        assert glu(limit=limit) == xn.ERR_ARG and b"limit" in err() and b"above 0" in err()
    assert glu(limit=INF, ids=None) == xn.ERR_ARG and b"NULL ids" in err()       # +Inf is legal: the next check speaks
    assert glu(he=2) == xn.ERR_ARG and b"unknown h_elem" in err() and glu(act=xn.FP4, he=xn.FP8) == xn.ERR_ARG and b"fp4 with h_elem fp8" in err()
    for name, text in (("x", b"NULL x_codes"), ("h", b"NULL h_codes"), ("hs", b"NULL h_scales")):
        assert glu(**{name: None}) == xn.ERR_ARG and text in err()
    assert glu(h=P + 8) == xn.ERR_ARG and b"misaligned h_codes" in err() and glu(T=0, I=48) == xn.ERR_SHAPE and glu(T=0, alpha=INF) == xn.ERR_ARG
    # down + sum's own
    assert down(rd=3) == xn.ERR_ARG and b"rw" in err() and down(od=3) == xn.ERR_ARG
    need = xn.workspace_bytes(8, 8)
    for bad in (dict(ws=None), dict(wb=need - 1), dict(wb=0), dict(wb=-5)):
        assert down(**bad) == xn.ERR_WORKSPACE and b"workspace" in err() and b"%d needed" % need in err(), bad
    assert down(wb=need, ids=P + 2) == xn.ERR_ARG and b"misaligned ids" in err()  # exactly the workspace's bytes pass
    assert down(ws=P + 8) == xn.ERR_ARG and b"misaligned workspace" in err() and down(rw=P + 2) == xn.ERR_ARG and b"misaligned rw" in err()
    assert down(rw=None) == xn.ERR_ARG and b"NULL rw" in err() and down(out=None) == xn.ERR_ARG and b"NULL out" in err()
    assert down(T=0, ws=None, wb=0, rw=None, out=None, h=None, hs=None) == 0


def test_the_keyword_the_attribute_and_the_names():
    for name in ("matmul_mxfp4_experts_scaled_glu", "matmul_mxfp4_experts_scaled_sum", "moe_mlp_mxfp4_scaled"):
        assert name in bnb.__all__ and inspect.signature(getattr(bnb, name)).parameters["act_format"].default == "fp8", name
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    x, ids, rw = torch.zeros(4, 64, dtype=torch.bfloat16), u8(4, 2).int(), torch.zeros(4, 2)
    for bad in ("none", "int8", None):
        for call in (lambda: bnb.matmul_mxfp4_experts_scaled_glu(x, u8(3, 64, 32), u8(3, 64, 2), ids, act_format=bad),
                     lambda: bnb.matmul_mxfp4_experts_scaled_sum((u8(4, 2, 32), u8(4, 2, 1)), u8(3, 8, 16), u8(3, 8, 1), ids, rw, act_format=bad),
                     lambda: bnb.moe_mlp_mxfp4_scaled(x, u8(3, 64, 32), u8(3, 64, 2), None, u8(3, 64, 16), u8(3, 64, 1), None, ids, rw, act_format=bad)):
            with pytest.raises(ValueError, match="format"):
                call()
    with pytest.raises(ValueError, match="multiple of the MX block"):
        bnb.matmul_mxfp4_experts_scaled_glu(x, u8(3, 96, 32), u8(3, 96, 2), ids)     # I = 48
    with pytest.raises(ValueError, match="codes, scales"):
        bnb.matmul_mxfp4_experts_scaled_sum(x, u8(3, 8, 16), u8(3, 8, 1), ids, rw)
    assert bnb.MoEMLPMXFP4.act_format == "none" and "act_format" not in inspect.signature(bnb.MoEMLPMXFP4.__init__).parameters
    layer = bnb.MoEMLPMXFP4(3, 64, 32)
    layer.act_format = "int8"
    with pytest.raises(ValueError, match="act_format"):
        layer(x, ids, rw)
    assert bnb.MoEBlockMXFP4(3, 64, 32, top_k=2).experts.act_format == "none"
