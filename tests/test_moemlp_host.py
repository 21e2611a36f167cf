"""CPU-side checks of the MXFP4 mixture-of-experts MLP (libmbnb_moemlp.so, functional.matmul_mxfp4_experts_glu / _sum / moe_mlp_mxfp4,
nn.MoEMLPMXFP4), without a GPU: the C ABI (the header, the binding and the library agree; the library exports exactly
its header and needs no other libmbnb_*; every argument error is a status before any device access), the Python surface, the numpy
restatements of tests/moemlp_cases.py and its case tables."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _moemlp_native as mlpn, _mx_native as mxn
from tests import moe_cases, moemlp_cases as cases, optim_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_moemlp.h")
CSRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc")
SOURCE = os.path.join(CSRC, "moemlp_kernels.hip")
NAMES = sorted(["mbnb_moemlp_abi_version", "mbnb_moemlp_last_error", "mbnb_moemlp_last_launch", "mbnb_moemlp_gate_up_glu",
                "mbnb_moemlp_workspace_bytes", "mbnb_moemlp_down_sum"])
F32 = np.float32
INF = float("inf")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_header_binding_and_library_agree():
    lib = mlpn.lib()
    assert mlpn.available()
    header = open(HEADER).read()
    assert mlpn.ABI_VERSION == 1 and lib.mbnb_moemlp_abi_version() == 1
    assert int(re.search(r"#define MBNB_MOEMLP_ABI_VERSION (\d+)", header).group(1)) == 1
    assert int(re.search(r"#define MBNB_MOEMLP_MAX_PAIRS (\d+)", header).group(1)) == mlpn.MAX_PAIRS == 1024
    assert int(re.search(r"#define MBNB_MOEMLP_MAX_EXPERTS (\d+)", header).group(1)) == mlpn.MAX_EXPERTS == 1024
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_moemlp_\w+)\s*\(", code)))
    assert declared == sorted(mlpn.EXPORTED_SYMBOLS) == NAMES
    for name, n in (("gate_up_glu", 17), ("workspace_bytes", 3), ("down_sum", 19)):
        n_args = len(re.search(r"mbnb_moemlp_" + name + r"\(([^)]*)\)", code).group(1).split(","))
        assert n_args == len(mlpn._SIGNATURES["mbnb_moemlp_" + name][1]) == n, name
    assert (mlpn.ERR_ARG, mlpn.ERR_SHAPE, mlpn.ERR_WORKSPACE) == (moen.ERR_ARG, moen.ERR_SHAPE, -3)
    assert re.search(r"MBNB_MOEMLP_ERR_ARG = -1, MBNB_MOEMLP_ERR_SHAPE = -2, MBNB_MOEMLP_ERR_WORKSPACE = -3", header)
    assert lib.mbnb_moemlp_last_launch() == b"" or lib.mbnb_moemlp_last_launch().startswith(b"mx_")
    # the ABIs of the libraries this one stands beside did not move
    moe_header = open(os.path.join(ROOT, "include", "mbnb_moe.h")).read()
    assert int(re.search(r"#define MBNB_MOE_ABI_VERSION (\d+)", moe_header).group(1)) == 1 == moen.ABI_VERSION == moen.lib().mbnb_moe_abi_version()
    assert len(moen.EXPORTED_SYMBOLS) == 4 and "moemlp" not in moe_header.lower()
    mx_header = open(os.path.join(ROOT, "include", "mbnb_mx.h")).read()
    assert int(re.search(r"#define MBNB_MX_ABI_VERSION (\d+)", mx_header).group(1)) == 2 == mxn.ABI_VERSION == mxn.lib().mbnb_mx_abi_version()


def test_the_library_exports_exactly_its_header_and_needs_no_other_library_of_ours():
    assert _exported(mlpn.LIB_PATH) == NAMES
    assert not [n for n in _exported(moen.LIB_PATH) + _exported(mxn.LIB_PATH) if n.startswith("mbnb_moemlp")]
    needed = subprocess.run(["readelf", "-d", mlpn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed
    assert not hasattr(mlpn, "_REQUIRES")


def test_the_makefile_the_build_and_the_source():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*moemlp$", makefile, flags=re.M) and re.search(r"^moemlp_SRCS\s*:=\s*moemlp_kernels\.hip$", makefile, flags=re.M)
    assert "moemlp" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1) and "libmbnb_moemlp.so" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    tup = [n.strip() for n in re.search(r"for binding in \(([^)]*)\)", entry).group(1).split(",")]
    assert tup.index("_moemlp_native") + 1 == tup.index("_group_native") and tup[-1] == "_mlora_native" and len(tup) == 12
    src = open(SOURCE).read()
    for path in (SOURCE, HEADER, mlpn.__file__):
        text = open(path).read()
        assert "set_kernel_name" not in text and "set_kernel_variant" not in text, path
        assert "atomic" not in text.lower() and "asm" not in text, path
    assert '#include "host.h"' in src and "common.h" not in src and '#include "mx_decode.h"' in src
    assert "mbnb_moemlp_last_launch" in src and "last_launch()" in src and "k_mx_experts_rt" in src and "k_routed_sum" in src
    shared = open(os.path.join(CSRC, "mx_decode.h")).read()
    for name in ("decode8_16", "mfma16", "scale_value", "load_bias", "store_out"):       # defined once, in the header the three files share
        assert re.search(r"__device__ __forceinline__ [\w ]+ " + name + r"\(", shared), name
        assert not re.search(r"__device__ __forceinline__ [\w ]+ " + name + r"\(", src), name
    # the decode tile, the pair list and the checks of an expert call are the header's too: this file only calls them
    for name in ("tile_walk", "tile_reduce", "list_pairs", "lane_rank", "check_expert_call", "check_expert_pointers"):
        definition = re.compile(r"^(?:__device__ __forceinline__|static) [\w ]+ " + name + r"\(", flags=re.M)
        assert len(definition.findall(shared)) == 1 and not definition.search(src), name
    for inner in ("__builtin_amdgcn_permlane32_swap", "mfma16(", "decode8_16<"):
        assert inner in shared and inner not in src, inner
    calls = lambda name: len(re.findall(r"\b" + name + r"(?:<\w+>)?\(", src))            # whatever the arguments are called
    assert calls("tile_walk") == 1 == calls("tile_reduce") == calls("list_pairs")
    assert src.count("__ballot(") == 2 == shared.count("__ballot(")      # here the presence walk; the ballots over the ids are list_pairs'
    # both entry points go through the shared shape check and the shared NULL and alignment checks
    assert calls("check_expert_call") == 2 and calls("check_expert_pointers") + calls("check_expert_nulls") == 2 == 1 + calls("check_expert_alignment")
    assert "MBNB_MOEMLP_MAX_PAIRS == mbnb::mx::kMaxPairs" in src and "MBNB_MOEMLP_ERR_ARG == mbnb::mx::kErrArg" in src
    assert "MBNB_MOE_MAX_PAIRS == mbnb::mx::kMaxPairs" in open(os.path.join(CSRC, "moe_kernels.hip")).read()


def test_argument_errors_are_a_status_before_any_device_access():
    lib = mlpn.lib()
    err = lambda: lib.mbnb_moemlp_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first

    def glu(x=P, T=4, A=2, K=64, xd=1, w=P, s=P, E=3, I=8, ids=P, bias=None, bd=0, alpha=1.702, limit=7.0, out=P, od=1):
        return lib.mbnb_moemlp_gate_up_glu(x, T, A, K, xd, w, s, E, I, ids, bias, bd, alpha, limit, out, od, None)

    def down(h=P, T=4, A=2, K=64, hd=1, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, rw=P, rd=2, out=P, od=1, ws=P, wb=1 << 20):
        return lib.mbnb_moemlp_down_sum(h, T, A, K, hd, w, s, E, N, ids, bias, bd, rw, rd, out, od, ws, wb, None)

    for f, n, rows in ((glu, "I", "xd"), (down, "N", "hd")):
        assert f(**{rows: 7}) == mlpn.ERR_ARG and b"dtype" in err()
        assert f(**{rows: -1}) == mlpn.ERR_ARG and b"dtype" in err()
        assert f(od=3) == mlpn.ERR_ARG and b"dtype" in err()
        assert f(bias=P, bd=9) == mlpn.ERR_ARG and b"dtype" in err()
        assert f(**{rows: 2}) == mlpn.ERR_ARG and b"16-bit activations" in err()
        assert f(K=80) == mlpn.ERR_SHAPE and b"multiple" in err()
        assert f(K=0) == mlpn.ERR_SHAPE and f(K=-32) == mlpn.ERR_SHAPE
        assert f(E=0) == mlpn.ERR_SHAPE and f(E=-1) == mlpn.ERR_SHAPE
        assert f(**{n: 0}) == mlpn.ERR_SHAPE and f(**{n: -3}) == mlpn.ERR_SHAPE
        assert f(T=-1) == mlpn.ERR_SHAPE and f(A=-1) == mlpn.ERR_SHAPE
        # MAX_EXPERTS and MAX_PAIRS pass the shape checks (the next refusal is the NULL ids); one more does not
        assert f(E=mlpn.MAX_EXPERTS, ids=None) == mlpn.ERR_ARG and b"NULL" in err()
        assert f(E=mlpn.MAX_EXPERTS + 1) == mlpn.ERR_SHAPE and b"experts" in err()
        assert f(T=mlpn.MAX_PAIRS // 4, A=4, ids=None) == mlpn.ERR_ARG and b"NULL" in err()
        assert f(T=mlpn.MAX_PAIRS, A=1, ids=None) == mlpn.ERR_ARG and b"NULL" in err()
        assert f(T=mlpn.MAX_PAIRS + 1, A=1) == mlpn.ERR_SHAPE and b"pairs" in err()
        assert f(T=1, A=mlpn.MAX_PAIRS + 1) == mlpn.ERR_SHAPE and b"pairs" in err()
        assert f(T=2 ** 40, A=2 ** 40) == mlpn.ERR_SHAPE and b"pairs" in err()
        # sizes within one launch
        assert f(E=2 ** 10, K=2 ** 10, **{n: 2 ** 20}) == mlpn.ERR_SHAPE and b"exceed" in err()
        assert f(E=4, K=2 ** 10, **{n: 2 ** 30}) == mlpn.ERR_SHAPE and b"exceed" in err()
        assert f(E=1, K=32, T=1024, A=1, **{n: 2 ** 29}) == mlpn.ERR_SHAPE and b"exceed" in err()
        assert f(ids=P + 2) == mlpn.ERR_ARG and b"misaligned" in err() and b"ids" in err()
        assert f(w=P + 2) == mlpn.ERR_ARG and b"misaligned" in err()
        assert f(out=P + 1) == mlpn.ERR_ARG and b"misaligned" in err()
        assert f(out=P + 2, od=2) == mlpn.ERR_ARG and b"misaligned" in err()
        assert f(bias=P + 2, bd=2) == mlpn.ERR_ARG and b"misaligned" in err()
        assert f(bias=P + 1, bd=1) == mlpn.ERR_ARG and b"misaligned" in err()
    for name in ("x", "w", "s", "ids", "out"):
        assert glu(**{name: None}) == mlpn.ERR_ARG and b"NULL" in err(), name
    for name in ("h", "w", "s", "ids", "rw", "out"):
        assert down(**{name: None}) == mlpn.ERR_ARG and b"NULL" in err(), name
    assert glu(x=P + 8) == mlpn.ERR_ARG and b"misaligned" in err()
    assert down(h=P + 8) == mlpn.ERR_ARG and b"misaligned" in err()
    assert glu(I=2 ** 40) == mlpn.ERR_SHAPE
    # alpha and limit
    for bad in (INF, -INF, float("nan")):
        assert glu(alpha=bad) == mlpn.ERR_ARG and b"alpha" in err(), bad
    for bad in (0.0, -0.0, -7.0, -INF, float("nan")):
        assert glu(limit=bad) == mlpn.ERR_ARG and b"limit" in err(), bad
    assert glu(limit=INF, alpha=0.0, ids=None) == mlpn.ERR_ARG and b"NULL" in err()           # +Inf and 0 pass
    assert glu(limit=1e-30, alpha=-3.0, ids=None) == mlpn.ERR_ARG and b"NULL" in err()
    # the routing weights and the workspace
    assert down(rd=3) == mlpn.ERR_ARG and b"dtype" in err() and down(rd=-1) == mlpn.ERR_ARG
    assert down(rw=P + 2, rd=2) == mlpn.ERR_ARG and b"misaligned" in err()
    assert down(rw=P + 1, rd=0) == mlpn.ERR_ARG and b"misaligned" in err()
    need = lib.mbnb_moemlp_workspace_bytes(4, 2, 8)
    assert need == 256
    assert down(wb=need - 1) == mlpn.ERR_WORKSPACE and b"workspace" in err()
    assert down(wb=0) == mlpn.ERR_WORKSPACE and down(wb=-1) == mlpn.ERR_WORKSPACE
    assert down(ws=None) == mlpn.ERR_WORKSPACE and b"workspace" in err()
    assert down(ws=P + 8) == mlpn.ERR_ARG and b"misaligned" in err() and b"workspace" in err()
    assert down(wb=need, ids=P + 2) == mlpn.ERR_ARG and b"ids" in err()                       # exactly workspace_bytes passes
    # empty work: a no-op success, pointers unread
    assert glu(T=0, x=None, w=None, s=None, ids=None, out=None) == 0
    assert glu(A=0, x=None, w=None, s=None, ids=None, out=None) == 0
    assert down(T=0, h=None, w=None, s=None, ids=None, rw=None, out=None, ws=None, wb=0) == 0
    assert down(A=0, h=None, w=None, s=None, ids=None, rw=None, out=None, ws=None, wb=0) == 0
    with pytest.raises(RuntimeError, match="status -3"):
        mlpn.check(-3, "unit")


def test_workspace_bytes():
    f = mlpn.lib().mbnb_moemlp_workspace_bytes
    assert [f(1, 1, 1), f(1, 1, 64), f(1, 1, 65), f(4, 4, 2880), f(256, 4, 2880), f(0, 4, 8), f(4, 0, 8)] == \
        [256, 256, 512, 4 * 4 * 2880 * 4, 1024 * 2880 * 4, 0, 0]
    assert mlpn.workspace_bytes(5, 3, 17) == 1024 == -(-5 * 3 * 17 * 4 // 256) * 256
    assert f(1024, 1, 8) == 1024 * 32 and f(1025, 1, 8) == mlpn.ERR_SHAPE and f(1, 1025, 8) == mlpn.ERR_SHAPE
    assert f(-1, 1, 8) == mlpn.ERR_SHAPE and f(1, -1, 8) == mlpn.ERR_SHAPE and f(1, 1, 0) == mlpn.ERR_SHAPE and f(1, 1, -8) == mlpn.ERR_SHAPE
    assert f(1024, 1, 2 ** 29) == mlpn.ERR_SHAPE and f(2 ** 40, 2 ** 40, 1) == mlpn.ERR_SHAPE
    with pytest.raises(RuntimeError, match="status -2"):
        mlpn.workspace_bytes(1025, 1, 8)


# ----------------------------------------------------------------------------- the Python surface
def test_signatures_and_exports():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.matmul_mxfp4_experts_glu) == [("input", E), ("weight", E), ("weight_scales", E), ("expert_ids", E), ("bias", None),
                                                    ("alpha", 1.702), ("limit", 7.0), ("dtype", None)]
    assert params(bnb.matmul_mxfp4_experts_sum) == [("input", E), ("weight", E), ("weight_scales", E), ("expert_ids", E), ("routing_weights", E),
                                                    ("bias", None), ("dtype", None)]
    assert params(bnb.moe_mlp_mxfp4) == [("input", E), ("gate_up_weight", E), ("gate_up_scales", E), ("gate_up_bias", E), ("down_weight", E),
                                         ("down_scales", E), ("down_bias", E), ("expert_ids", E), ("routing_weights", E), ("alpha", 1.702),
                                         ("limit", 7.0), ("dtype", None)]
    assert params(bnb.MoEMLPMXFP4.__init__) == [("self", E), ("num_experts", E), ("hidden_size", E), ("intermediate_size", E), ("bias", True),
                                                ("alpha", 1.702), ("limit", 7.0), ("device", None), ("compute_dtype", torch.bfloat16)]
    assert params(bnb.MoEMLPMXFP4.forward) == [("self", E), ("x", E), ("expert_ids", E), ("routing_weights", E)]
    assert params(bnb.MoEMLPMXFP4.from_weights)[:6] == [("gate", E), ("up", E), ("down", E), ("gate_bias", None), ("up_bias", None), ("down_bias", None)]
    for name in ("matmul_mxfp4_experts_glu", "matmul_mxfp4_experts_sum", "moe_mlp_mxfp4", "MoEMLPMXFP4"):
        assert name in bnb.__all__ and hasattr(bnb, name), name
    assert "MoEMLPMXFP4" in bnb.nn.__all__ and bnb.nn.MoEMLPMXFP4 is bnb.MoEMLPMXFP4
    assert bnb.moe_mlp_mxfp4 is bnb.functional.moe_mlp_mxfp4 and bnb.matmul_mxfp4_experts_glu is bnb.functional.matmul_mxfp4_experts_glu
    assert len(bnb.__all__) == len(set(bnb.__all__)) and len(bnb.nn.__all__) == len(set(bnb.nn.__all__))


def _cpu_operands(E=3, N=8, K=64, T=4, A=2, dtype=torch.bfloat16):
    return (torch.zeros(T, K, dtype=dtype), torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 32, dtype=torch.uint8),
            torch.zeros(T, A, dtype=torch.int32), torch.zeros(T, A))


def test_what_the_two_functions_refuse():
    x, w, s, ids, rw = _cpu_operands()
    h = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    glu = bnb.matmul_mxfp4_experts_glu
    ssum = lambda *a, **k: bnb.matmul_mxfp4_experts_sum(*a, **k)
    for f, inp, tail in ((glu, x, ()), (ssum, h, (rw,))):
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
        glu(h, w, s, ids)                                    # a row per slot is the down projection's form
    with pytest.raises(ValueError, match="does not match expert_ids"):
        ssum(x, w, s, ids, rw)                               # and a shared row the gate / up projection's
    with pytest.raises(ValueError, match="come in pairs"):
        glu(x, w[:, :7], s[:, :7], ids)
    for bad in (dict(alpha=INF), dict(alpha=float("nan")), dict(limit=0.0), dict(limit=-1.0), dict(limit=float("nan"))):
        with pytest.raises(ValueError, match="alpha .* finite and limit"):
            glu(x, w, s, ids, **bad)
    with pytest.raises(ValueError, match="cuda"):
        glu(x, w, s, ids, limit=INF, alpha=0.0)
    with pytest.raises(ValueError, match="routing_weights"):
        ssum(h, w, s, ids, rw[:, :1])
    with pytest.raises(ValueError, match="routing_weights"):
        ssum(h, w, s, ids, rw.long())
    with pytest.raises(NotImplementedError, match="inference-only"):
        ssum(h, w, s, ids, rw.clone().requires_grad_())
    with pytest.raises(ValueError, match="cuda"):
        bnb.moe_mlp_mxfp4(x, torch.zeros(3, 16, 32, dtype=torch.uint8), torch.zeros(3, 16, 2, dtype=torch.uint8), None,
                          torch.zeros(3, 64, 4, dtype=torch.uint8), torch.zeros(3, 64, 1, dtype=torch.uint8), None, ids, rw)


def test_the_module_state_dict_round_trip_and_repr():
    layer = bnb.MoEMLPMXFP4(3, 64, 32)
    shapes = {"gate_up_proj_blocks": (3, 64, 2, 16), "gate_up_proj_scales": (3, 64, 2), "gate_up_proj_bias": (3, 64),
              "down_proj_blocks": (3, 64, 1, 16), "down_proj_scales": (3, 64, 1), "down_proj_bias": (3, 64)}
    sd = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes and list(sd) == list(shapes)
    assert all(sd[k].dtype == (torch.bfloat16 if k.endswith("bias") else torch.uint8) for k in sd)
    assert bool((layer.gate_up_proj_scales == 127).all()) and not list(layer.parameters())
    for part in ("num_experts=3", "hidden_size=64", "intermediate_size=32", "bias=True", "alpha=1.702", "limit=7.0", "mxfp4"):
        assert part in repr(layer), part
    g = torch.Generator().manual_seed(1)
    new = {k: (torch.randn(shapes[k], generator=g) if k.endswith("bias") else torch.randint(0, 255, shapes[k], generator=g, dtype=torch.uint8)) for k in shapes}
    other = bnb.MoEMLPMXFP4(3, 64, 32, compute_dtype=torch.float16)
    other.load_state_dict({k: v.clone() for k, v in new.items()})
    for k in shapes:
        assert torch.equal(getattr(other, k), new[k].to(getattr(other, k).dtype)), k
    assert other.down_proj_bias.dtype == torch.float16
    bare = bnb.MoEMLPMXFP4(2, 32, 96, bias=False, alpha=1.0, limit=INF)
    assert bare.gate_up_proj_bias is None and bare.down_proj_bias is None and len(bare.state_dict()) == 4 and "bias=False" in repr(bare) and "limit=inf" in repr(bare)
    for bad in ((0, 64, 32), (3, 48, 32), (3, 64, 48), (3, 0, 32), (3, 64, 0)):
        with pytest.raises(ValueError):
            bnb.MoEMLPMXFP4(*bad)
    with pytest.raises(ValueError, match="cuda"):
        layer(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"\[E, I, H\]"):
        bnb.MoEMLPMXFP4.from_weights(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(64, 8))
    with pytest.raises(ValueError, match="down"):
        bnb.MoEMLPMXFP4.from_weights(torch.zeros(3, 32, 64), torch.zeros(3, 32, 64), torch.zeros(3, 32, 64))
    with pytest.raises(ValueError, match="none of them"):
        bnb.MoEMLPMXFP4.from_weights(torch.zeros(3, 32, 64), torch.zeros(3, 32, 64), torch.zeros(3, 64, 32), torch.zeros(3, 32))


def test_from_weights_interleaves_gate_and_up(monkeypatch):
    """Row 2j of the stored weight is gate j and row 2j + 1 is up j (and so for the bias): shown with a stand-in for the HIP quantiser
    that records the rows it is given"""
    from mps_bitsandbytes_amd import functional as F
    seen = []

    def fake_quantize(t, elem):
        seen.append(t.clone())
        return torch.zeros(t.shape[0], t.shape[1] // 2, dtype=torch.uint8), torch.full((t.shape[0], t.shape[1] // 32), 127, dtype=torch.uint8)

    monkeypatch.setattr(F, "quantize_mx", fake_quantize)
    E, I, H = 2, 32, 64
    gate = torch.arange(E * I * H, dtype=torch.float32).reshape(E, I, H)
    up, down = -gate, torch.ones(E, H, I)
    gb, ub, db = torch.arange(E * I, dtype=torch.float32).reshape(E, I), -torch.arange(E * I, dtype=torch.float32).reshape(E, I) - 1, torch.ones(E, H)
    layer = bnb.MoEMLPMXFP4.from_weights(gate, up, down, gb, ub, db, device="cpu")
    rows = seen[0].reshape(E, 2 * I, H)
    assert torch.equal(rows[:, 0::2], gate) and torch.equal(rows[:, 1::2], up) and tuple(seen[1].shape) == (E * H, I)
    assert torch.equal(layer.gate_up_proj_bias[:, 0::2].float(), gb) and torch.equal(layer.gate_up_proj_bias[:, 1::2].float(), ub)
    assert torch.equal(layer.down_proj_bias.float(), db) and layer.compute_dtype == torch.bfloat16


# ----------------------------------------------------------------------------- the chains
def _sweep():
    g = np.concatenate([np.linspace(-60.0, 7.0, 200001), np.linspace(-53.0, -51.0, 20001), np.linspace(6.9, 7.1, 2001)]).astype(F32)
    us = np.array([-7.0, -1.5, -1.0, 0.0, 0.37, 3.0, 7.0], dtype=F32)
    return np.repeat(g[None, :], us.size, axis=0), np.repeat(us[:, None], g.size, axis=1)


def test_the_numpy_restatement_stays_inside_the_derived_bound():
    g, u = _sweep()
    r = cases.glu_f64(g, u, cases.ALPHA, cases.LIMIT)
    y = cases.glu_f32(g, u, cases.ALPHA, cases.LIMIT).astype(np.float64)
    ratio = np.abs(y - r) / cases.glu_tol(r)
    assert ratio.max() < 0.5, ratio.max()
    for dtype in cases.DTYPES:
        ok, _, _ = cases.within_glu_bound(cases.round_direct(y, dtype), r, dtype)
        assert ok.all(), dtype
    # the planted pre-activations of the GPU test, and what they cover
    bias = cases.planted_bias()
    pg, pu = cases.split(bias)
    lim = F32(cases.LIMIT)
    assert {float(lim), float(np.nextafter(lim, F32(0))), float(np.nextafter(lim, F32(9)))} <= set(pg.reshape(-1).tolist())
    assert {float(lim), float(-lim)} <= set(pu.reshape(-1).tolist())
    edge = -88.72284 / cases.ALPHA
    assert (np.abs(pg - edge) < 2e-3).sum() >= 3 and abs(edge + 52.13) < 0.01 and pg.min() <= -60.0 and np.isfinite(bias).all()
    r = cases.glu_f64(pg, pu, cases.ALPHA, cases.LIMIT)
    assert (np.abs(cases.glu_f32(pg, pu, cases.ALPHA, cases.LIMIT) - r) <= cases.glu_tol(r)).all()
    ids = cases.planted_ids()
    assert set(ids.reshape(-1).tolist()) == set(range(cases.PLANT_SHAPE[0]))


def test_the_alpha_zero_restatement_is_the_float64_chain_rounded_per_operation():
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.normal(0, 6, 20000), [7.0, -7.0, 0.0, 1e-40, 3e38, -3e38, INF, -INF, np.nan]]).astype(F32)
    u = np.concatenate([rng.normal(0, 6, 20000), [7.0, -7.0, -1.0, 1e-40, 3e38, -3e38, -INF, INF, 1.0]]).astype(F32)
    for limit in (cases.LIMIT, INF):
        a, b = cases.glu_f32(g, u, 0.0, limit), cases.glu_f64_rounded_per_operation(g, u, limit)
        assert (np.isnan(a) == np.isnan(b)).all() and (a[~np.isnan(a)].view(np.uint32) == b[~np.isnan(b)].view(np.uint32)).all()
    assert np.isnan(cases.glu_f32(F32(-INF), F32(1), 0.0, 7.0)) and cases.glu_f32(F32(INF), F32(1), 0.0, 7.0) == 7.0      # 0 * Inf; the clamp
    assert cases.glu_f32(F32(100), F32(100), 0.0, 7.0) == 28.0 and cases.glu_f32(F32(2), F32(-100), 0.0, 7.0) == -6.0


def test_round_direct_and_the_routed_sum():
    v = np.array([1.00390625, 1.01171875, 65520.0, 3.4e38, 1e-45, -2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.9])
    assert cases.round_direct(v, torch.bfloat16).tolist() == [1.0, 1.015625, 65536.0, INF, 0.0, -2.0 ** -25, 1.0, 1.0, 65536.0]
    assert cases.round_direct(v, torch.float16).tolist() == [1.00390625, 1.01171875, INF, INF, 0.0, -0.0, 1.0, 1 + 2.0 ** -9, 65504.0]
    x = np.random.default_rng(6).normal(0, 100, 5000)
    for dtype in (torch.bfloat16, torch.float16):
        assert (cases.round_direct(x, dtype) == torch.from_numpy(x).to(dtype).double().numpy()).sum() > 4990      # torch rounds twice: rare ties
    ids = np.array([[0, 5, 1], [-1, 9, 2 ** 31 - 1], [2, -1, 2]], dtype=np.int32)
    rw = np.array([[0.5, np.nan, 0.25], [np.nan, np.nan, np.nan], [1.0, np.nan, 2.0 ** -24]], dtype=F32)
    y = np.arange(18, dtype=F32).reshape(9, 2) + F32(1)
    out = cases.routed_sum_f32(y, rw, ids, 5)
    assert out[1].view(np.uint32).tolist() == [0, 0]
    assert out[0].tolist() == [0.5 * 1 + 0.25 * 5, 0.5 * 2 + 0.25 * 6]
    assert out[2, 0] == optim_emul.fma(F32(2.0 ** -24), F32(17), F32(13)) == F32(13.000001)


# ----------------------------------------------------------------------------- the tables
def test_the_case_tables_cover_every_listed_size():
    G, S = cases.GLU_CASES, cases.SUM_CASES
    assert {c[0] for c in G} == {1, 2, 5, 9, 1024} == {c[0] for c in S}
    assert {c[1] for c in G} == {1, 7, 8, 9, 17} and {c[1] for c in S} == {1, 5, 15, 16, 17, 33}
    assert {c[2] for c in G} == {32, 64, 160, 1056, 2080} == {c[2] for c in S}
    assert {c[4] for c in S} >= {1, 2, 4, 8}
    for table in (G, S):
        assert {c[3] * c[4] for c in table} >= {1, cases.SCAN - 1, cases.SCAN, cases.SCAN + 1, cases.MAX_PAIRS}
        assert all(sum(c[5]) == c[3] * c[4] and len(c[5]) == c[0] for c in table)
        assert any(set(c[5]) >= set(cases.EDGE_COUNTS) for c in table) and cases.EDGE_COUNTS == (0, 1, 15, 16, 17, 33)
        distinct = [(sum(1 for n in c[5] if n), c[0], c[3] * c[4]) for c in table]
        assert any(d == 1 and e > 1 for d, e, p in distinct)                                  # one distinct expert
        assert any(d == e < p for d, e, p in distinct) and any(d == p < e for d, e, p in distinct)
        assert any(c[5][-1] and not any(c[5][:-1]) for c in table) and any(c[5][0] and not any(c[5][1:]) for c in table if c[0] > 1)
        big = [c for c in table if c[0] == cases.MAX_EXPERTS]
        assert [c[1:3] for c in big] == [(1, 32)] and big[0][5][1023] and big[0][5][0] and big[0][5][63] and big[0][5][64]
        assert {(c[6], c[7]) for c in table} == {(xd, od) for xd in cases.X16 for od in cases.DTYPES}
        assert {c[8] for c in table} == {True, False}
    assert {c[9] for c in G} == {cases.LIMIT, INF} and {c[9] for c in S} == set(cases.DTYPES)
    assert any(c[3] == 1 and c[4] > 1 and max(c[5]) == c[4] for c in S)                      # all slots of a token on one expert
    # the pre-activations of the exact cases lie on both sides of the limit, and are exact in f32 in any order
    for index, case in enumerate(G):
        x, w, bias, ids = cases.glu_operands(case, index)
        assert (cases.to_dtype(x, case[6]).double().numpy() == x).all() and ids.shape == (case[3], case[4])
        flat = ids.reshape(-1)
        pre = np.einsum("pk,pnk->pn", np.repeat(x, case[4], axis=0), w[flat]) + (0 if bias is None else bias[flat])
        total = np.einsum("pk,pnk->pn", np.abs(np.repeat(x, case[4], axis=0)), np.abs(w[flat])) + 8
        assert (pre % 2.0 ** -7 == 0).all() and total.max() / 2.0 ** -7 < 2.0 ** 24
        assert (pre < -cases.LIMIT).any() and (np.abs(pre) < cases.LIMIT).any() and ((pre > cases.LIMIT).any() or pre.size == 2)
    for index, case in enumerate(S):
        h, w, bias, ids, rw = cases.sum_operands(case, index)
        assert h.shape == (case[3], case[4], case[2]) and rw.shape == ids.shape == (case[3], case[4])
        for dtype in cases.DTYPES:
            assert (cases.to_dtype(rw, dtype).double().numpy() == rw).all()
    planted = [set(cases.sum_operands(c, i)[4].reshape(-1).tolist()) >= set(cases.RW_SPECIALS) for i, c in enumerate(S)]
    assert sum(planted) >= 8 and {c[9] for c, p in zip(S, planted) if p} == set(cases.DTYPES)
    assert cases.RANDOM_GLU_SHAPES == ((5, 3, 4, 34, 1056), (5, 3, 4, 18, 1056)) and cases.RANDOM_SUM_SHAPE == (16, 4, 9, 17, 2080)
    E, I, K, T, A = cases.EDGE_SHAPE
    assert cases.NAN_BLOCKS == (0, K // 64, K // 32 - 1) and cases.EDGE_IDS.shape == (T, A) and cases.EDGE_IDS.max() == E - 1
    routed = (cases.EDGE_IDS == cases.NAN_EXPERT).any(axis=1)
    assert routed.any() and not routed.all() and (cases.EDGE_IDS[3] == cases.NAN_EXPERT).all() and cases.NAN_OUTPUT < I
    assert len(set(cases.OUT_OF_RANGE_PLACES)) == 4 == len(cases.OUT_OF_RANGE) and all(t != 1 for t, _ in cases.OUT_OF_RANGE_PLACES)
    for off in cases.OFFSETS:
        assert off["x"] % 16 == 0 and off["w_codes"] % 16 == 0 and off["ws"] % 16 == 0
    assert {o["ws"] for o in cases.OFFSETS} == {0, 16, 32, 48} and {o["rw"] % 4 for o in cases.OFFSETS} == {0, 1, 2, 3}
    T, A, E, I, H = cases.CUT_SHAPE
    assert T * A > cases.MAX_PAIRS and (cases.MAX_PAIRS // A) * 2 > T > cases.MAX_PAIRS // A
    assert cases.glu_text(torch.bfloat16, 32, 4) == "mx_glu bf16 E32 P4 R4" and cases.down_text(torch.float16, 9, 64, 4) == "mx_down_sum f16 E9 P64 R9 A4"


def _assert_walk_operands_exact(rows, x_dtype, w, bias, ids, unit):
    """The conditions of tests/test_moe_host.py's exact cases on rows scaled by 2^-3: rows exact in their 16-bit type, weights that
    quantise to their own codes, every block's partial sum and every output a multiple of the unit, the sum of the magnitudes below
    2^24 units: exact in f32 in any order"""
    E, N, K = w.shape
    assert (cases.to_dtype(rows, x_dtype).double().numpy() == rows).all()
    codes, scales = cases.quantize_experts(w)
    assert (moe_cases.decode_experts(codes, scales) == w).all()
    w2 = w.reshape(E * N, K)
    total = np.abs(rows) @ np.abs(w2).T + (0 if bias is None else np.abs(bias).reshape(-1)[None, :])
    assert total.max() / unit < 2.0 ** 24, total.max()
    blocks = np.einsum("mbk,nbk->mnb", rows.reshape(rows.shape[0], -1, 32), w2.reshape(E * N, -1, 32))
    assert (blocks % unit == 0).all() and (blocks.sum(axis=2) == rows @ w2.T).all()
    pre = moe_cases.reference_f64(rows.reshape(ids.shape[0], -1, K) if rows.shape[0] == ids.size else rows, w, bias, ids)
    assert (pre % unit == 0).all() and (pre.astype(F32) == pre).all()
    return pre


@pytest.mark.parametrize("index", range(len(cases.WALK_KS)))
def test_every_walk_case_of_both_epilogues_is_exact_in_f32_in_any_order(index):
    K = cases.WALK_KS[index]
    assert 3104 * 144 * 0.125 / 2.0 ** -7 < 2.0 ** 24         # the worst case of lossless rows at the longest K
    case = cases.WALK_GLU_CASES[index]
    assert case[:6] == (3, cases.TILE // 2 + 1, K, 11, 3, (17, 0, 16))
    x, w, bias, ids = cases.glu_operands(case, cases.WALK_SEED + index)
    assert np.bincount(ids.reshape(-1), minlength=3).tolist() == [17, 0, 16] and w.shape == (3, 18, K)
    pre = _assert_walk_operands_exact(x, case[6], w, bias, ids, 2.0 ** -7)
    assert (pre < -cases.LIMIT).any() and (np.abs(pre) < cases.LIMIT).any() and (pre > cases.LIMIT).any()
    case = cases.WALK_SUM_CASES[index]
    assert case[:6] == (3, cases.TILE + 1, K, 11, 3, (17, 0, 16))
    h, w, bias, ids, rw = cases.sum_operands(case, cases.WALK_SEED + index)
    assert h.shape == (11, 3, K) and set(rw.reshape(-1).tolist()) >= set(cases.RW_SPECIALS)
    for dtype in cases.DTYPES:
        assert (cases.to_dtype(rw, dtype).double().numpy() == rw).all()
    _assert_walk_operands_exact(h.reshape(-1, K), case[6], w, bias, ids, 2.0 ** -7)


def test_the_walk_cases_alternate_every_form():
    G, S = cases.WALK_GLU_CASES, cases.WALK_SUM_CASES
    assert cases.WALK_KS is moe_cases.WALK_KS and [c[2] for c in G] == list(cases.WALK_KS) == [c[2] for c in S]
    for table in (G, S):
        assert {c[6] for c in table} == set(cases.X16) and {c[7] for c in table} == set(cases.DTYPES) and {c[8] for c in table} == {True, False}
        assert all(table[i][6] != table[i + 1][6] and table[i][7] != table[i + 1][7] for i in range(len(table) - 1))
    assert {c[9] for c in G} == {cases.LIMIT, INF} and {c[9] for c in S} == set(cases.DTYPES)
    assert not set(cases.WALK_KS) & ({c[2] for c in cases.GLU_CASES} | {c[2] for c in cases.SUM_CASES})
