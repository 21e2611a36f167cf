"""CPU-side checks of the mixture-of-experts router and block (libmbnb_router.so, functional.moe_router_topk / moe_block_mxfp4,
nn.MoERouterTopK / MoEBlockMXFP4), without a GPU: the C ABI (the header, the binding and the library agree; the library
exports exactly its header and needs no other libmbnb_*; every argument error is a status before any device access), the Python
surface, the numpy restatement of tests/router_cases.py and its case tables."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moemlp_native as mlpn, _router_native as rn
from tests import router_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_router.h")
CSRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc")
SOURCE = os.path.join(CSRC, "router_kernels.hip")
NAMES = sorted(["mbnb_router_abi_version", "mbnb_router_last_error", "mbnb_router_last_launch", "mbnb_router_topk_softmax"])
F32 = np.float32
INF = float("inf")
NAN = float("nan")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_header_binding_and_library_agree():
    lib = rn.lib()
    assert rn.available()
    header = open(HEADER).read()
    assert rn.ABI_VERSION == 1 and lib.mbnb_router_abi_version() == 1
    assert int(re.search(r"#define MBNB_ROUTER_ABI_VERSION (\d+)", header).group(1)) == 1
    assert int(re.search(r"#define MBNB_ROUTER_MAX_EXPERTS (\d+)", header).group(1)) == rn.MAX_EXPERTS == 1024 == mlpn.MAX_EXPERTS
    assert int(re.search(r"#define MBNB_ROUTER_MAX_TOPK (\d+)", header).group(1)) == rn.MAX_TOPK == 32
    assert int(re.search(r"#define MBNB_ROUTER_MAX_K (\d+)", header).group(1)) == rn.MAX_K and rn.MAX_K % 8 == 0 and rn.MAX_K >= 2880
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_router_\w+)\s*\(", code)))
    assert declared == sorted(rn.EXPORTED_SYMBOLS) == NAMES
    n_args = len(re.search(r"mbnb_router_topk_softmax\(([^)]*)\)", code).group(1).split(","))
    assert n_args == len(rn._SIGNATURES["mbnb_router_topk_softmax"][1]) == 14
    assert (rn.ERR_ARG, rn.ERR_SHAPE) == (mlpn.ERR_ARG, mlpn.ERR_SHAPE)
    assert re.search(r"MBNB_ROUTER_ERR_ARG = -1, MBNB_ROUTER_ERR_SHAPE = -2", header)
    assert re.search(r"MBNB_ROUTER_F16 = 0, MBNB_ROUTER_BF16 = 1, MBNB_ROUTER_F32 = 2", header)
    assert (rn.F16, rn.BF16, rn.F32) == (0, 1, 2)
    assert lib.mbnb_router_last_launch() == b"" or lib.mbnb_router_last_launch().startswith(b"router ")


def test_the_library_exports_exactly_its_header_and_needs_no_other_library_of_ours():
    assert _exported(rn.LIB_PATH) == NAMES
    assert not [n for n in _exported(mlpn.LIB_PATH) if n.startswith("mbnb_router")]
    needed = subprocess.run(["readelf", "-d", rn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed
    assert not hasattr(rn, "_REQUIRES")


def test_the_makefile_the_build_and_the_source():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*router$", makefile, flags=re.M) and re.search(r"^router_SRCS\s*:=\s*router_kernels\.hip$", makefile, flags=re.M)
    assert "router" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1) and "libmbnb_router.so" in makefile
    assert "-ffp-contract=off" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    tup = [n.strip() for n in re.search(r"for binding in \(([^)]*)\)", entry).group(1).split(",")]
    assert tup == ["_native", "_optim_native", "_train_native", "_sparse_native", "_paged_native", "_mx_native", "_moe_native", "_moemlp_native",
                   "_group_native", "_lora_native", "_batch_native", "_mlora_native"]
    after = entry[entry.index("for binding in ("):]
    assert re.search(r"^\s+_router_native\.lib\(\)", after, flags=re.M) and "thirteen" in entry and "libmbnb_router.so" in entry
    src = open(SOURCE).read()
    for path in (SOURCE, HEADER, rn.__file__):
        text = open(path).read()
        assert "set_kernel_name" not in text and "set_kernel_variant" not in text, path
        assert "atomic" not in text.lower() and "asm" not in text, path
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes == ["../../include/mbnb_router.h", "host.h"]
    assert "mbnb_router_last_launch" in src and "last_launch()" in src and "k_router" in src and src.count("hipLaunchKernelGGL") == 1
    assert "_loader" in open(rn.__file__).read() and "CDLL" not in open(rn.__file__).read()


def test_argument_errors_are_a_status_before_any_device_access():
    lib = rn.lib()
    err = lambda: lib.mbnb_router_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first

    def f(x=P, T=4, K=64, xd=1, w=P, E=8, bias=None, bd=0, A=2, ids=P, rw=P, rd=2, logits=None):
        return lib.mbnb_router_topk_softmax(x, T, K, xd, w, E, bias, bd, A, ids, rw, rd, logits, None)

    assert f(xd=7) == rn.ERR_ARG and b"dtype" in err()
    assert f(xd=-1) == rn.ERR_ARG and b"dtype" in err()
    assert f(xd=2) == rn.ERR_ARG and b"16-bit" in err()      # f32 activations
    assert f(rd=3) == rn.ERR_ARG and b"dtype" in err() and f(rd=-1) == rn.ERR_ARG
    assert f(bias=P, bd=9) == rn.ERR_ARG and b"dtype" in err()
    for K in (0, -8, 4, 12, 63, 2881):
        assert f(K=K) == rn.ERR_SHAPE and b"multiple of 8" in err(), K
    assert f(K=rn.MAX_K + 8) == rn.ERR_SHAPE and b"at most" in err()
    assert f(K=rn.MAX_K, ids=None) == rn.ERR_ARG and b"NULL" in err()                         # the limit itself passes the shape checks
    assert f(E=0) == rn.ERR_SHAPE and f(E=-1) == rn.ERR_SHAPE
    assert f(E=rn.MAX_EXPERTS + 1) == rn.ERR_SHAPE and b"experts" in err()
    assert f(E=rn.MAX_EXPERTS, A=32, ids=None) == rn.ERR_ARG and b"NULL" in err()
    for A, E in ((0, 8), (-1, 8), (9, 8), (33, 64), (33, 1024), (2, 1)):
        assert f(A=A, E=E) == rn.ERR_SHAPE and b"top_k" in err(), (A, E)
    assert f(A=8, E=8, ids=None) == rn.ERR_ARG and f(A=32, E=32, ids=None) == rn.ERR_ARG and f(A=1, E=1, ids=None) == rn.ERR_ARG
    assert f(T=-1) == rn.ERR_SHAPE and b"T =" in err()
    assert f(T=2 ** 31) == rn.ERR_SHAPE and f(T=2 ** 40) == rn.ERR_SHAPE and b"one launch" in err()
    assert f(T=2 ** 31 - 1, ids=None) == rn.ERR_ARG and b"NULL" in err()
    for name in ("x", "w", "ids", "rw"):
        assert f(**{name: None}) == rn.ERR_ARG and b"NULL" in err(), name
    assert f(x=P + 8) == rn.ERR_ARG and b"misaligned" in err() and b"16 bytes" in err()
    assert f(w=P + 2) == rn.ERR_ARG and b"misaligned" in err() and b"16 bytes" in err()
    assert f(ids=P + 2) == rn.ERR_ARG and b"misaligned" in err() and b"ids" in err()
    assert f(logits=P + 2) == rn.ERR_ARG and b"misaligned" in err() and b"logits_out" in err()
    assert f(rw=P + 2, rd=2) == rn.ERR_ARG and b"misaligned" in err()
    assert f(rw=P + 1, rd=0) == rn.ERR_ARG and b"misaligned" in err()
    assert f(bias=P + 2, bd=2) == rn.ERR_ARG and b"misaligned" in err()
    assert f(bias=P + 1, bd=1) == rn.ERR_ARG and b"misaligned" in err()
    # empty work: a no-op success, pointers unread; the other refusals still come first
    assert f(T=0, x=None, w=None, ids=None, rw=None) == 0
    assert f(T=0, x=None, w=None, ids=None, rw=None, bias=None, logits=None, A=8, E=8, K=rn.MAX_K) == 0
    assert f(T=0, K=12) == rn.ERR_SHAPE and f(T=0, A=9) == rn.ERR_SHAPE and f(T=0, xd=2) == rn.ERR_ARG
    with pytest.raises(RuntimeError, match="status -2"):
        rn.check(-2, "unit")


# ----------------------------------------------------------------------------- the Python surface
def test_signatures_and_exports():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.moe_router_topk) == [("input", E), ("weight", E), ("bias", None), ("top_k", 4), ("weights_dtype", torch.float32),
                                           ("return_logits", False)]
    assert params(bnb.moe_block_mxfp4)[:9] == [("input", E), ("router_weight", E), ("router_bias", E), ("gate_up_weight", E), ("gate_up_scales", E),
                                               ("gate_up_bias", E), ("down_weight", E), ("down_scales", E), ("down_bias", E)]
    assert params(bnb.moe_block_mxfp4)[9:] == [("top_k", 4), ("alpha", 1.702), ("limit", 7.0), ("return_routing", False)]
    assert params(bnb.MoERouterTopK.__init__) == [("self", E), ("hidden_size", E), ("num_experts", E), ("top_k", 4), ("bias", True), ("device", None),
                                                  ("dtype", torch.bfloat16)]
    assert params(bnb.MoERouterTopK.forward) == [("self", E), ("x", E)]
    assert params(bnb.MoERouterTopK.from_linear)[:2] == [("linear", E), ("top_k", 4)]
    assert params(bnb.MoEBlockMXFP4.__init__) == [("self", E), ("num_experts", E), ("hidden_size", E), ("intermediate_size", E), ("top_k", 4),
                                                  ("bias", True), ("alpha", 1.702), ("limit", 7.0), ("device", None), ("compute_dtype", torch.bfloat16)]
    assert params(bnb.MoEBlockMXFP4.forward) == [("self", E), ("x", E), ("return_routing", False)]
    for name in ("moe_router_topk", "moe_block_mxfp4", "MoERouterTopK", "MoEBlockMXFP4"):
        assert name in bnb.__all__ and hasattr(bnb, name), name
    assert "MoERouterTopK" in bnb.nn.__all__ and "MoEBlockMXFP4" in bnb.nn.__all__
    assert bnb.nn.MoERouterTopK is bnb.MoERouterTopK and bnb.nn.MoEBlockMXFP4 is bnb.MoEBlockMXFP4
    assert bnb.moe_router_topk is bnb.functional.moe_router_topk and bnb.moe_block_mxfp4 is bnb.functional.moe_block_mxfp4
    assert len(bnb.__all__) == len(set(bnb.__all__)) and len(bnb.nn.__all__) == len(set(bnb.nn.__all__))


def test_what_the_function_refuses():
    f = bnb.moe_router_topk
    x, w, b = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="cuda"):            # well-formed operands: the refusal left is the CPU tensor
        f(x, w, b)
    with pytest.raises(ValueError, match="cuda"):
        f(x.reshape(2, 2, 64).half(), w.half(), None, top_k=8, weights_dtype=torch.float16, return_logits=True)
    with pytest.raises(ValueError, match="cuda"):
        f(x, w, b.float())
    with pytest.raises(ValueError, match=r"\[E, K\]"):
        f(x, w[0], b)
    with pytest.raises(ValueError, match="multiple of 8"):
        f(x[:, :60], w[:, :60], b)
    with pytest.raises(ValueError, match="multiple of 8"):
        f(torch.zeros(1, rn.MAX_K + 8, dtype=torch.bfloat16), torch.zeros(2, rn.MAX_K + 8, dtype=torch.bfloat16), None, top_k=1)
    with pytest.raises(ValueError, match="1025 experts"):
        f(x, torch.zeros(1025, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="does not match weight"):
        f(x[:, :56], w, b)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        f(x.float(), w.float(), b)
    with pytest.raises(ValueError, match="input's dtype"):
        f(x, w.half(), b)
    with pytest.raises(ValueError, match="bias"):
        f(x, w, b[:7])
    with pytest.raises(ValueError, match="bias"):
        f(x, w, b.reshape(1, 8))
    with pytest.raises(ValueError, match="bias"):
        f(x, w, b.long())
    for bad in (0, -1, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="top_k"):
            f(x, w, b, top_k=bad)
    with pytest.raises(ValueError, match="top_k"):
        f(x, torch.zeros(64, 64, dtype=torch.bfloat16), None, top_k=33)
    for bad in (torch.float64, torch.int32):
        with pytest.raises(ValueError, match="weights_dtype"):
            f(x, w, b, weights_dtype=bad)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x.clone().requires_grad_(), w, b)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x, w.clone().requires_grad_(), b)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x, w, b.clone().requires_grad_())
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        f(x.clone().requires_grad_(), w, b)
    with pytest.raises(ValueError, match="cuda"):
        bnb.moe_block_mxfp4(x, w, b, torch.zeros(8, 128, 32, dtype=torch.uint8), torch.zeros(8, 128, 2, dtype=torch.uint8), None,
                            torch.zeros(8, 64, 32, dtype=torch.uint8), torch.zeros(8, 64, 2, dtype=torch.uint8), None)


def test_the_modules_state_dict_round_trip_and_repr():
    router = bnb.MoERouterTopK(64, 8)
    sd = router.state_dict()
    assert list(sd) == ["weight", "bias"] and tuple(sd["weight"].shape) == (8, 64) and tuple(sd["bias"].shape) == (8,)
    assert sd["weight"].dtype == sd["bias"].dtype == torch.bfloat16 and not list(router.parameters())
    for part in ("hidden_size=64", "num_experts=8", "top_k=4", "bias=True", "bfloat16"):
        assert part in repr(router), part
    bare = bnb.MoERouterTopK(64, 8, top_k=8, bias=False, dtype=torch.float16)
    assert bare.bias is None and list(bare.state_dict()) == ["weight"] and "bias=False" in repr(bare) and "top_k=8" in repr(bare)
    for bad in ((60, 8), (0, 8), (64, 0)):
        with pytest.raises(ValueError):
            bnb.MoERouterTopK(*bad)
    for bad in (0, 9, 33):
        with pytest.raises(ValueError, match="top_k"):
            bnb.MoERouterTopK(64, 8 if bad != 33 else 64, top_k=bad)
    with pytest.raises(ValueError, match="dtype"):
        bnb.MoERouterTopK(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        router(torch.zeros(4, 64, dtype=torch.bfloat16))
    linear = torch.nn.Linear(64, 8)
    got = bnb.MoERouterTopK.from_linear(linear, 2)
    assert got.top_k == 2 and got.weight.dtype == torch.bfloat16 and torch.equal(got.weight, linear.weight.detach().to(torch.bfloat16))
    assert torch.equal(got.bias, linear.bias.detach().to(torch.bfloat16)) and got.weight.device.type == "cpu"
    got = bnb.MoERouterTopK.from_linear(torch.nn.Linear(64, 8, bias=False).half())
    assert got.bias is None and got.weight.dtype == torch.float16 and got.top_k == 4

    block = bnb.MoEBlockMXFP4(8, 64, 32)
    keys = ["router.weight", "router.bias"] + ["experts." + k for k in bnb.MoEMLPMXFP4(8, 64, 32).state_dict()]
    assert list(block.state_dict()) == keys and len(keys) == 8 and not list(block.parameters())
    assert isinstance(block.router, bnb.MoERouterTopK) and isinstance(block.experts, bnb.MoEMLPMXFP4)
    assert block.router.top_k == 4 and block.experts.alpha == 1.702 and block.experts.limit == 7.0
    for part in ("MoERouterTopK", "MoEMLPMXFP4", "top_k=4", "num_experts=8", "intermediate_size=32"):
        assert part in repr(block), part
    g = torch.Generator().manual_seed(2)
    new = {k: (torch.randint(0, 255, tuple(v.shape), generator=g, dtype=torch.uint8) if v.dtype == torch.uint8 else torch.randn(tuple(v.shape), generator=g))
           for k, v in block.state_dict().items()}
    other = bnb.MoEBlockMXFP4(8, 64, 32, top_k=2, compute_dtype=torch.float16)
    result = other.load_state_dict({"" + k: v.clone() for k, v in new.items()}, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for k, v in other.state_dict().items():
        assert torch.equal(v, new[k].to(v.dtype)), k
    assert other.router.weight.dtype == torch.float16 and other.experts.down_proj_bias.dtype == torch.float16
    again = bnb.MoEBlockMXFP4(8, 64, 32)
    again.load_state_dict(block.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        again.load_state_dict({k: v for k, v in new.items() if k != "router.bias"}, strict=True)
    bare = bnb.MoEBlockMXFP4(8, 64, 32, bias=False)
    assert "router.bias" not in bare.state_dict() and len(bare.state_dict()) == 5


def test_the_blocks_forward_is_the_composition_of_the_two_functional_calls(monkeypatch):
    from mps_bitsandbytes_amd import functional as F
    calls = []

    def fake_router(input, weight, bias=None, top_k=4, weights_dtype=torch.float32, return_logits=False):
        calls.append(("router", input, weight, bias, top_k))
        T = input.reshape(-1, input.shape[-1]).shape[0]
        return torch.full((T, top_k), 3, dtype=torch.int32), torch.full((T, top_k), 0.25)

    def fake_mlp(input, gu, gus, gub, dw, ds, db, expert_ids, routing_weights, alpha=1.702, limit=7.0, dtype=None):
        calls.append(("mlp", input, gu, gus, gub, dw, ds, db, expert_ids, routing_weights, alpha, limit))
        return input + 1

    monkeypatch.setattr(F, "moe_router_topk", fake_router)
    monkeypatch.setattr(F, "moe_mlp_mxfp4", fake_mlp)
    block = bnb.MoEBlockMXFP4(8, 64, 32, top_k=2, alpha=1.5, limit=6.0)
    x = torch.randn(2, 3, 64).to(torch.bfloat16)
    out, (ids, rw) = block(x, return_routing=True)
    assert [c[0] for c in calls] == ["router", "mlp"]
    r, m = calls
    assert tuple(r[1].shape) == (6, 64) and r[2] is block.router.weight and r[3] is block.router.bias and r[4] == 2
    assert m[1] is r[1] and m[2] is block.experts.gate_up_proj_blocks and m[7] is block.experts.down_proj_bias
    assert m[8] is ids and m[9] is rw and m[10:] == (1.5, 6.0)
    assert tuple(out.shape) == (2, 3, 64) and torch.equal(out, x + 1) and tuple(ids.shape) == (6, 2)
    calls.clear()
    out2 = block(x[0])
    assert torch.equal(out2, x[0] + 1) and calls[0][1] is not None and tuple(calls[1][1].shape) == (3, 64)
    # the function is the same composition
    calls.clear()
    e = block.experts
    out3, (ids3, rw3) = F.moe_block_mxfp4(x, block.router.weight, block.router.bias, e.gate_up_proj_blocks, e.gate_up_proj_scales, e.gate_up_proj_bias,
                                          e.down_proj_blocks, e.down_proj_scales, e.down_proj_bias, top_k=2, alpha=1.5, limit=6.0, return_routing=True)
    assert [c[0] for c in calls] == ["router", "mlp"] and calls[1][8] is ids3 and calls[1][9] is rw3 and calls[1][10:] == (1.5, 6.0)
    assert torch.equal(out3, out) and calls[0][4] == 2


# ----------------------------------------------------------------------------- the restatement
def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_the_tie_rule_the_nan_rank_and_the_zeros():
    l = np.array([[1.0, 3.0, 3.0, -INF, 3.0, INF, 2.0, 3.0]], dtype=F32)
    assert cases.select(l, 8).tolist() == [[5, 1, 2, 4, 7, 6, 0, 3]]
    assert cases.select(l, 3).tolist() == [[5, 1, 2]]
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(F32)[0]
    l = np.array([[INF, NAN, 0.0, neg_nan, -INF]], dtype=F32)
    assert cases.select(l, 5).tolist() == [[1, 3, 0, 2, 4]]      # NaNs of either sign first, in index order, then +Inf
    l = np.array([[-1.0, -0.0, 0.0, -0.0, 1e-45, -1e-45]], dtype=F32)
    assert cases.select(l, 6).tolist() == [[4, 1, 2, 3, 5, 0]]   # -0 == +0: index order among them; the denormals on either side
    keys = cases.rank_key(np.array([-INF, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, INF, NAN], dtype=F32)).astype(np.int64)
    assert (np.diff(keys) >= 0).all() and (np.diff(keys) == 0).sum() == 1 and keys[4] == keys[5] and keys[-1] == 0xFFFFFFFF and keys.min() > 0
    ids, rw = cases.emulate(np.array([[1.0, NAN, 2.0, 0.5]], dtype=F32), 3)
    assert ids.tolist() == [[1, 2, 0]] and np.isnan(rw).all()    # a NaN logit is first and makes every weight of the token NaN
    ids, rw = cases.emulate(np.array([[INF, 1.0, INF, 0.5]], dtype=F32), 2)
    assert ids.tolist() == [[0, 2]] and np.isnan(rw).all()       # Inf - Inf
    ids, rw = cases.emulate(np.array([[-INF, 1.0], [1.0, -INF]], dtype=F32), 2)
    assert ids.tolist() == [[1, 0], [0, 1]] and _bits(rw).tolist() == [[0x3F800000, 0], [0x3F800000, 0]]      # a selected -Inf: +0
    ids64, rw64 = cases.emulate64(np.array([[-INF, 1.0], [2.0, NAN]], dtype=F32), 2)
    assert ids64.tolist() == [[1, 0], [1, 0]] and rw64[0].tolist() == [1.0, 0.0] and np.isnan(rw64[1]).all()


def test_the_exact_cases_of_the_chain():
    for A in (1, 2, 3, 4, 7, 8, 32):
        for c in (0.0, -3.25, 1e30, -1e-40):
            ids, rw = cases.emulate(np.full((2, 40), c, dtype=F32), A)
            assert ids.tolist() == [list(range(A))] * 2
            assert (_bits(rw) == _bits(F32(1) / F32(A))).all(), (A, c)
    for gap in (110.0, 111.5, 1000.0, 1e30):
        l = np.array([[5.0 - 2 * gap, 5.0, 5.0 - gap, 5.0 - 3 * gap]], dtype=F32)
        ids, rw = cases.emulate(l, 4)
        assert ids.tolist() == [[1, 2, 0, 3]] and _bits(rw).tolist() == [[0x3F800000, 0, 0, 0]], gap
    c = F32(7.5)
    ids, rw = cases.emulate(np.array([[c - 110, c, c - 110, c]], dtype=F32), 4)
    assert ids.tolist() == [[1, 3, 0, 2]] and rw.tolist() == [[0.5, 0.5, 0.0, 0.0]]
    # the planted rows of the GPU test: what each must give, and which are exact
    for name in cases.PLANTED:
        b, A, exact = cases.planted(name)
        ids, rw = cases.emulate(b[None, :], A)
        _, rw64 = cases.emulate64(b[None, :], A)
        assert cases.within_weight_bound(rw, rw64, A).all(), name
        v = b[ids[0]]
        assert (np.diff(v) <= 0).all() and all(ids[0, i] < ids[0, i + 1] for i in range(A - 1) if v[i] == v[i + 1]), name
        if exact:
            d = v - v[0]
            assert ((d == 0) | (d <= -110)).all(), name
    assert cases.emulate(cases.planted("all-equal")[0][None], 4)[0].tolist() == [[0, 1, 2, 3]]
    assert cases.emulate(cases.planted("pairs-64")[0][None], 4)[0].tolist() == [[6, 70, 5, 69]]
    assert cases.emulate(cases.planted("pairs-4-and-16")[0][None], 4)[0].tolist() == [[33, 37, 100, 116]]
    assert cases.emulate(cases.planted("zeros")[0][None], 8)[0].tolist() == [[3, 27, 64, 90, 91, 0, 1, 2]]
    assert cases.emulate(cases.planted("boundary")[0][None], 4)[0].tolist() == [[77, 8, 9, 10]]
    assert cases.emulate(cases.planted("half-half")[0][None], 4)[0].tolist() == [[40, 101, 2, 41]]
    z = cases.planted("zeros")[0]
    assert np.signbit(z[[27, 90, 91]]).all() and not np.signbit(z[[3, 64]]).any()


def test_the_f32_chain_stays_inside_the_bound_of_the_float64_chain():
    v = cases.gap_sweep()
    assert v.shape[1] == cases.SWEEP_A and (np.diff(v, axis=1) <= 0).all()
    gaps = (v[:, 1:].astype(np.float64) - v[:, :1])
    assert gaps.min() < -99 and gaps.max() > -0.01 and ((gaps < -87.4) & (gaps > -100)).sum() > 1000
    ids, rw = cases.emulate(v, cases.SWEEP_A)
    ids64, rw64 = cases.emulate64(v, cases.SWEEP_A)
    assert np.array_equal(ids, ids64) and (ids == np.arange(cases.SWEEP_A)).all()
    with np.errstate(all="ignore"):
        ratio = np.abs(rw.astype(np.float64) - rw64) / cases.weight_tol(rw64, cases.SWEEP_A)
    assert cases.within_weight_bound(rw, rw64, cases.SWEEP_A).all(), float(ratio.max())
    assert abs(rw64.sum(axis=1) - 1).max() < 1e-12
    assert cases.weight_tol(np.array([1.0, 0.0]), 4).tolist() == [16 * 2.0 ** -24 + 2.0 ** -149, 2.0 ** -149]


def test_the_lossless_operands_and_the_logit_bound():
    for index, case in enumerate(cases.LOGIT_CASES):
        E, K, T, A, dtype, bias_dtype = case
        x, W, bias = cases.logit_operands(case, index)
        assert x.shape == (T, K) and W.shape == (E, K) and (bias is None) == (bias_dtype is None)
        for a in (x, W):
            assert (cases.to_dtype(a, dtype).double().numpy() == a).all()
        if bias is not None:
            assert (cases.to_dtype(bias, bias_dtype).double().numpy() == bias).all()
        # every product a multiple of 2^-4, and the sum of the magnitudes (the bias included) below 2^-4 * 2^24: exact in any order
        mag = np.abs(x) @ np.abs(W).T + (0 if bias is None else np.abs(bias))
        assert ((x[:, None, :] * W[None, :, :]) % 2.0 ** -4 == 0).all() and mag.max() / 2.0 ** -4 < 2.0 ** 24
        l = cases.logits_f64(x, W, bias)
        assert (l.astype(F32).astype(np.float64) == l).all()
        if E >= 63:
            assert any(len(set(row.tolist())) < E for row in l)                            # small integers: ties are the rule
    x, W, b = np.ones((1, 8)), np.full((2, 8), 0.5), np.array([1.0, -2.0])
    assert cases.logits_f64(x, W, b).tolist() == [[5.0, 2.0]] and cases.logit_tol(x, W, b).tolist() == [[10 * 2.0 ** -24 * 5, 10 * 2.0 ** -24 * 6]]


def test_the_gap_fixture_leaves_no_token_out():
    T, K, E, A = cases.GAP_SHAPE
    assert (K, E, T) == (64, 128, 64) and len(cases.GAP_SEEDS) >= 2
    for seed in cases.GAP_SEEDS:
        x, W, bias = cases.gap_operands(seed)
        ids, ok = cases.gap_margins(x, W, bias, A)
        assert ids.shape == (T, A) and ok.shape == (T,) and ok.all(), (seed, np.nonzero(~ok)[0])
        l = cases.logits_f64(x.double().numpy(), W.double().numpy(), bias.double().numpy())
        assert np.array_equal(ids, cases.select(l.astype(F32), A))
        assert len({tuple(r) for r in ids.tolist()}) > T // 2                              # the tokens route differently


def test_the_case_tables_cover_every_listed_size():
    L = cases.LOGIT_CASES
    assert {c[0] for c in L} >= {1, 2, 63, 64, 65, 128, 1000, 1024}
    assert {c[1] for c in L} == {8, 16, 504, 512, 520, 2880}
    assert {c[2] for c in L} == {1, 2, 3, 17}
    assert {c[3] for c in L} >= {1, 2, 4, 8, 32} and any(c[3] == c[0] and 2 < c[0] <= 32 for c in L) and all(c[3] <= min(c[0], 32) for c in L)
    assert {c[4] for c in L} == set(cases.X16) and {c[5] for c in L} == set(cases.DTYPES) | {None}
    assert {c[4] for c in L if c[5] is None} == set(cases.X16)
    assert cases.RANDOM_SHAPES == ((17, 2880, 32, 4), (17, 2880, 128, 4))
    assert set(cases.PLANTED) == {"all-equal", "pairs-64", "pairs-4-and-16", "zeros", "boundary", "half-half"}
    T, K, E, A = cases.BAD_SHAPE
    assert cases.BAD_K == (0, K // 2, K - 1) and 0 < cases.BAD_TOKEN < T - 1 and cases.BAD_EXPERT < E and K > 512
    assert cases.BLOCK_SHAPES == ((8, 64, 64, 2, 1), (8, 64, 64, 2, 5), (8, 64, 64, 4, 1), (8, 64, 64, 4, 5))
    for off in cases.OFFSETS:
        assert off["x"] % 16 == 0 and off["w"] % 16 == 0
    assert {o["rw"] % 4 for o in cases.OFFSETS} == {0, 1, 3} and {o["ids"] for o in cases.OFFSETS} == {0, 1, 2, 3}
    assert cases.launch_text(torch.bfloat16, 128, 2880, 4, 3) == "router bf16 E128 K2880 A4 T3"
