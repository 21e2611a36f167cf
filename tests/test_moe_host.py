"""CPU-side checks of the MXFP4 expert linears (libmbnb_moe.so, functional.matmul_mxfp4_experts, nn.ExpertsMXFP4),
without a GPU: the C ABI (the header, the binding and the library agree; the library exports exactly its header and needs no other
libmbnb_*; every argument error is a status before any device access), the Python surface, and the case tables of
tests/moe_cases.py: every exact case is exact in f32 in ANY summation order and stays inside the normal f32 range."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _moe_native as moen, _mx_native as mxn
from tests import moe_cases as cases, mx_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_moe.h")
CSRC = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc")
SOURCE = os.path.join(CSRC, "moe_kernels.hip")
NAMES = sorted(["mbnb_moe_abi_version", "mbnb_moe_last_error", "mbnb_moe_last_launch", "mbnb_moe_mxfp4_experts"])
NORMAL_MIN, NORMAL_MAX = 2.0 ** -126, 2.0 ** 128


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the C ABI, without a device
def test_header_binding_and_library_agree():
    lib = moen.lib()
    assert moen.available()
    header = open(HEADER).read()
    assert moen.ABI_VERSION == 1 and lib.mbnb_moe_abi_version() == 1
    assert int(re.search(r"#define MBNB_MOE_ABI_VERSION (\d+)", header).group(1)) == 1
    assert int(re.search(r"#define MBNB_MOE_MAX_PAIRS (\d+)", header).group(1)) == moen.MAX_PAIRS == 1024
    declared = sorted(set(re.findall(r"\b(mbnb_moe_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(moen.EXPORTED_SYMBOLS) == NAMES
    n_args = len(re.search(r"int mbnb_moe_mxfp4_experts\(([^)]*)\)", header).group(1).split(","))
    assert n_args == len(moen._SIGNATURES["mbnb_moe_mxfp4_experts"][1]) == 16
    assert (moen.ERR_ARG, moen.ERR_SHAPE) == (mxn.ERR_ARG, mxn.ERR_SHAPE) == (-1, -2)
    assert re.search(r"MBNB_MOE_ERR_ARG = -1, MBNB_MOE_ERR_SHAPE = -2", header)
    assert lib.mbnb_moe_last_launch() == b"" or lib.mbnb_moe_last_launch().startswith(b"mx_experts ")
    # the MX library's ABI did not move
    mx_header = open(os.path.join(ROOT, "include", "mbnb_mx.h")).read()
    assert int(re.search(r"#define MBNB_MX_ABI_VERSION (\d+)", mx_header).group(1)) == 2 == mxn.ABI_VERSION == mxn.lib().mbnb_mx_abi_version()
    assert "moe" not in mx_header.lower()


def test_the_library_exports_exactly_its_header_and_needs_no_other_library_of_ours():
    assert _exported(moen.LIB_PATH) == NAMES
    assert not [n for n in _exported(mxn.LIB_PATH) if n.startswith("mbnb_moe")]
    needed = subprocess.run(["readelf", "-d", moen.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed
    assert not hasattr(moen, "_REQUIRES")


def test_the_makefile_the_build_and_the_sources():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*moe$", makefile, flags=re.M) and re.search(r"^moe_SRCS\s*:=\s*moe_kernels\.hip$", makefile, flags=re.M)
    assert "moe" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    tup = re.search(r"for binding in \(([^)]*)\)", entry).group(1)
    assert "_moe_native" in tup and tup.strip().endswith("_mlora_native")
    src = open(SOURCE).read()
    for path in (SOURCE, os.path.join(CSRC, "mx_decode.h"), HEADER, moen.__file__):
        text = open(path).read()
        assert "set_kernel_name" not in text and "set_kernel_variant" not in text, path
        assert "atomic" not in text.lower(), path
    assert '#include "host.h"' in src and '#include "common.h"' not in src and '#include "mx_decode.h"' in src
    assert "mbnb_moe_last_launch" in src and "last_launch()" in src and "k_mx_experts" in src
    # the helpers the two kernel files share are defined once, in the header both include
    mx_src = open(os.path.join(CSRC, "mx_kernels.hip")).read()
    shared = open(os.path.join(CSRC, "mx_decode.h")).read()
    assert '#include "mx_decode.h"' in mx_src
    for name in ("decode8_16", "mfma16", "scale_value", "load_bias", "store_out"):
        definition = re.compile(r"__device__ __forceinline__ [\w ]+ " + name + r"\(")
        assert definition.search(shared), name
        assert not definition.search(mx_src) and not definition.search(src), name
    assert "struct E2M1Bytes" in shared and "struct E2M1Bytes" not in mx_src and "struct E2M1Bytes" not in src
    # the decode tile, the pair list and the checks of an expert call are ONE text: defined in the header, called by the kernel files
    mlp_src = open(os.path.join(CSRC, "moemlp_kernels.hip")).read()
    kernels = {"mx_kernels.hip": mx_src, "moe_kernels.hip": src, "moemlp_kernels.hip": mlp_src}
    for name in ("tile_walk", "tile_reduce", "list_pairs", "lane_rank", "check_expert_call", "check_expert_pointers"):
        definition = re.compile(r"^(?:__device__ __forceinline__|static) [\w ]+ " + name + r"\(", flags=re.M)
        assert len(definition.findall(shared)) == 1, name
        assert not any(definition.search(text) for text in kernels.values()), name
    for name, text in kernels.items():
        for inner in ("__builtin_amdgcn_permlane32_swap", "mfma16(", "decode8_16<"):
            assert inner in shared and inner not in text, (name, inner)
    calls = lambda text, name: len(re.findall(r"\b" + name + r"(?:<\w+>)?\(", text))     # whatever the arguments are called
    for name in ("tile_walk", "tile_reduce"):
        assert all(calls(text, name) == 1 for text in kernels.values()), name
    assert calls(src, "list_pairs") == 1 == calls(mlp_src, "list_pairs") and calls(mx_src, "list_pairs") == 0
    # the ballot over the ids occurs once; the only other ballots of the three files walk moemlp's presence bytes
    assert shared.count("__ballot(") == 2 and "__ballot(" not in src and mlp_src.count("__ballot(") == 2 and "present[" in mlp_src
    assert calls(src, "check_expert_call") == 1 == calls(src, "check_expert_pointers") and calls(mx_src, "check_expert_call") == 0


def test_argument_errors_are_a_status_before_any_device_access():
    lib = moen.lib()
    err = lambda: lib.mbnb_moe_last_error()
    P = 4096                                                 # an aligned address that is never dereferenced: every call below fails first

    def experts(x=P, T=4, A=2, slot=0, K=64, xd=1, w=P, s=P, E=3, N=8, ids=P, bias=None, bd=0, out=P, od=1):
        return lib.mbnb_moe_mxfp4_experts(x, T, A, slot, K, xd, w, s, E, N, ids, bias, bd, out, od, None)

    assert experts(xd=7) == moen.ERR_ARG and b"dtype" in err()
    assert experts(xd=-1) == moen.ERR_ARG and b"dtype" in err()
    assert experts(od=3) == moen.ERR_ARG and b"dtype" in err()
    assert experts(bias=P, bd=9) == moen.ERR_ARG and b"dtype" in err()
    assert experts(xd=2) == moen.ERR_ARG and b"16-bit activations" in err()
    assert experts(xd=2, slot=1) == moen.ERR_ARG and b"16-bit activations" in err()
    assert experts(K=80) == moen.ERR_SHAPE and b"multiple" in err()
    assert experts(K=0) == moen.ERR_SHAPE and experts(K=-32) == moen.ERR_SHAPE
    assert experts(E=0) == moen.ERR_SHAPE and experts(E=-1) == moen.ERR_SHAPE
    assert experts(N=0) == moen.ERR_SHAPE and experts(N=-3) == moen.ERR_SHAPE
    assert experts(T=-1) == moen.ERR_SHAPE and experts(A=-1) == moen.ERR_SHAPE
    # MAX_PAIRS pairs pass the shape check (the next refusal is the NULL x); one more does not
    assert experts(T=moen.MAX_PAIRS // 4, A=4, x=None) == moen.ERR_ARG and b"NULL" in err()
    assert experts(T=moen.MAX_PAIRS, A=1, x=None) == moen.ERR_ARG and b"NULL" in err()
    assert experts(T=moen.MAX_PAIRS + 1, A=1) == moen.ERR_SHAPE and b"pairs" in err()
    assert experts(T=1, A=moen.MAX_PAIRS + 1) == moen.ERR_SHAPE and b"pairs" in err()
    assert experts(T=2 ** 40, A=2 ** 40) == moen.ERR_SHAPE and b"pairs" in err()
    # E x N x K within one launch
    assert experts(E=2 ** 10, N=2 ** 20, K=2 ** 10) == moen.ERR_SHAPE and b"exceed" in err()
    assert experts(E=4, N=2 ** 30, K=2 ** 10) == moen.ERR_SHAPE and b"exceed" in err()
    # the launch grid: 2^31 experts of one tile each
    assert experts(E=2 ** 31, N=1, K=32) == moen.ERR_SHAPE and b"workgroups" in err()
    assert experts(E=2 ** 31 - 1, N=1, K=32, x=None) == moen.ERR_ARG and b"NULL" in err()
    for name in ("x", "w", "s", "ids", "out"):
        assert experts(**{name: None}) == moen.ERR_ARG and b"NULL" in err(), name
    assert experts(x=P + 8) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(w=P + 2) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(ids=P + 2) == moen.ERR_ARG and b"misaligned" in err() and b"ids" in err()
    assert experts(ids=P + 1) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(out=P + 1) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(out=P + 2, od=2) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(bias=P + 2, bd=2) == moen.ERR_ARG and b"misaligned" in err()
    assert experts(bias=P + 1, bd=1) == moen.ERR_ARG and b"misaligned" in err()
    # empty work: a no-op success, pointers unread
    assert experts(T=0, x=None, w=None, s=None, ids=None, out=None) == 0
    assert experts(A=0, x=None, w=None, s=None, ids=None, out=None) == 0
    assert experts(T=0, A=0, slot=1, x=None, w=None, s=None, ids=None, out=None) == 0
    with pytest.raises(RuntimeError, match="status -1"):
        moen.check(-1, "unit")


# ----------------------------------------------------------------------------- the Python surface
def test_signatures_and_exports():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(bnb.matmul_mxfp4_experts) == [("input", E), ("weight", E), ("weight_scales", E), ("expert_ids", E), ("bias", None), ("dtype", None)]
    assert params(bnb.ExpertsMXFP4.__init__) == [("self", E), ("num_experts", E), ("in_features", E), ("out_features", E), ("bias", True),
                                                 ("device", None), ("compute_dtype", torch.bfloat16)]
    assert params(bnb.ExpertsMXFP4.forward) == [("self", E), ("x", E), ("expert_ids", E)]
    assert params(bnb.ExpertsMXFP4.from_weights)[:2] == [("weight", E), ("bias", None)]
    for name in ("matmul_mxfp4_experts", "ExpertsMXFP4"):
        assert name in bnb.__all__ and hasattr(bnb, name), name
    assert "ExpertsMXFP4" in bnb.nn.__all__ and bnb.nn.ExpertsMXFP4 is bnb.ExpertsMXFP4
    assert bnb.matmul_mxfp4_experts is bnb.functional.matmul_mxfp4_experts
    assert len(bnb.__all__) == len(set(bnb.__all__)) and len(bnb.nn.__all__) == len(set(bnb.nn.__all__))


def _cpu_operands(E=3, N=8, K=64, T=4, A=2, dtype=torch.bfloat16):
    return (torch.zeros(T, K, dtype=dtype), torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 32, dtype=torch.uint8),
            torch.zeros(T, A, dtype=torch.int32))


def test_what_is_refused():
    x, w, s, ids = _cpu_operands()
    f = bnb.matmul_mxfp4_experts
    with pytest.raises(ValueError, match="cuda"):            # well-formed operands: the refusal left is the CPU tensor
        f(x, w, s, ids)
    with pytest.raises(ValueError, match="cuda"):            # the checkpoint's blocks layout is accepted and viewed
        f(x, w.reshape(3, 8, 2, 16), s, ids)
    with pytest.raises(ValueError, match="cuda"):            # a row per slot, int64 ids, a bias
        f(torch.zeros(4, 2, 64, dtype=torch.float16), w, s, ids.long(), torch.zeros(3, 8))
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        f(x.float(), w, s, ids)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        f(x.double(), w, s, ids)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        f(x.to(torch.int8), w, s, ids)
    with pytest.raises(ValueError, match="blocks layout"):
        f(x, w.reshape(3, 8, 4, 8), s, ids)
    with pytest.raises(ValueError, match="uint8"):
        f(x, w.to(torch.int8), s, ids)
    with pytest.raises(ValueError, match="uint8"):
        f(x, w[0], s[0], ids)                                # one expert's 2-D tensors: that is matmul_mxfp4
    with pytest.raises(ValueError, match="multiple of the MX block"):
        f(torch.zeros(4, 48, dtype=torch.bfloat16), torch.zeros(3, 8, 24, dtype=torch.uint8), torch.zeros(3, 8, 1, dtype=torch.uint8), ids)
    with pytest.raises(ValueError, match="weight_scales"):
        f(x, w, s[:, :, :1], ids)
    with pytest.raises(ValueError, match="weight_scales"):
        f(x, w, s[:2], ids)
    with pytest.raises(ValueError, match="expert_ids"):
        f(x, w, s, ids.float())
    with pytest.raises(ValueError, match="expert_ids"):
        f(x, w, s, ids.reshape(-1))
    with pytest.raises(ValueError, match="expert_ids"):
        f(x, w, s, ids.bool())
    with pytest.raises(ValueError, match="does not match expert_ids"):
        f(x[:3], w, s, ids)                                  # T
    with pytest.raises(ValueError, match="does not match expert_ids"):
        f(torch.zeros(4, 32, dtype=torch.bfloat16), w, s, ids)                         # K
    with pytest.raises(ValueError, match="does not match expert_ids"):
        f(torch.zeros(4, 3, 64, dtype=torch.bfloat16), w, s, ids)                      # A of a per-slot input
    with pytest.raises(ValueError, match=r"\[T, K\]"):
        f(x[0], w, s, ids)
    with pytest.raises(ValueError, match=r"\[T, K\]"):
        f(torch.zeros(2, 2, 2, 64, dtype=torch.bfloat16), w, s, ids)
    with pytest.raises(ValueError, match="bias"):
        f(x, w, s, ids, torch.zeros(8))
    with pytest.raises(ValueError, match="bias"):
        f(x, w, s, ids, torch.zeros(8, 3))
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x.clone().requires_grad_(), w, s, ids)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x, w, s, ids, torch.zeros(3, 8, requires_grad=True))
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        f(x.clone().requires_grad_(), w, s, ids)


def test_the_module_state_dict_round_trip_and_repr():
    layer = bnb.ExpertsMXFP4(3, 64, 8)
    assert tuple(layer.weight.shape) == (3, 8, 32) and layer.weight.dtype == torch.uint8
    assert tuple(layer.weight_scales.shape) == (3, 8, 2) and bool((layer.weight_scales == 127).all())
    assert isinstance(layer.bias, torch.nn.Parameter) and tuple(layer.bias.shape) == (3, 8) and layer.bias.dtype == torch.bfloat16
    assert "num_experts=3" in repr(layer) and "in_features=64" in repr(layer) and "out_features=8" in repr(layer) and "mxfp4" in repr(layer)
    sd = layer.state_dict()
    assert set(sd) == {"weight", "weight_scales", "bias"}
    sd["weight"] = torch.arange(3 * 8 * 32, dtype=torch.int32).to(torch.uint8).reshape(3, 8, 32)
    sd["weight_scales"] = torch.arange(48, dtype=torch.uint8).reshape(3, 8, 2)
    sd["bias"] = torch.arange(24, dtype=torch.bfloat16).reshape(3, 8)
    other = bnb.ExpertsMXFP4(3, 64, 8, compute_dtype=torch.float16)
    other.load_state_dict(sd)
    assert torch.equal(other.weight, sd["weight"]) and torch.equal(other.weight_scales, sd["weight_scales"])
    assert torch.equal(other.bias.data.float(), sd["bias"].float()) and other.bias.dtype == torch.float16
    bare = bnb.ExpertsMXFP4(2, 32, 5, bias=False)
    assert bare.bias is None and set(bare.state_dict()) == {"weight", "weight_scales"} and "bias=False" in repr(bare)
    for bad in ((0, 64, 8), (3, 48, 8), (3, 0, 8), (3, 64, 0)):
        with pytest.raises(ValueError):
            bnb.ExpertsMXFP4(*bad)
    x, _, _, ids = _cpu_operands()
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer(x, ids)                                        # the bias Parameter requires grad
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        layer(x, ids)
    with pytest.raises(ValueError, match=r"\[E, N, K\]"):
        bnb.ExpertsMXFP4.from_weights(torch.zeros(8, 64))
    with pytest.raises(ValueError, match="bias"):
        bnb.ExpertsMXFP4.from_weights(torch.zeros(3, 8, 64), torch.zeros(8))


# ----------------------------------------------------------------------------- the tables
def _walk(rows, codes, scales):
    """(block partial sums P[m, n, b] = sum_{k in b} x * value(code), unscaled; their scaled values) in float64, as the decode loop forms them"""
    M = rows.shape[0]
    c = emul.unpack(codes, "fp4").astype(np.int64)
    v = np.where(c & 8, -emul.FP4_GRID[c & 7], emul.FP4_GRID[c & 7])
    P = np.einsum("mbk,nbk->mnb", rows.reshape(M, -1, 32), v.reshape(v.shape[0], -1, 32))
    return P, np.ldexp(P, (scales.astype(np.int64) - 127)[None, :, :])


def _normal_or_zero(a):
    a = np.abs(a[a != 0])
    return a.size == 0 or (a.min() >= NORMAL_MIN and a.max() < NORMAL_MAX)


@pytest.mark.parametrize("index", range(len(cases.EXACT_CASES)))
def test_every_exact_case_is_exact_in_f32_in_any_order(index):
    """Every row of the call against every row of every expert (a superset of the routed pairs): the sum of the product
    magnitudes of an output, and of a block, is below 2^24 units of its product grid; operands, partial sums and results are normal."""
    _assert_exact_in_any_order(cases.EXACT_CASES[index], *cases.exact_operands(cases.EXACT_CASES[index], index))


def _assert_exact_in_any_order(case, x, w, bias, ids):
    E, N, K, T, A, counts, x_dtype, _, _, per_slot = case
    assert x.shape == ((T, A, K) if per_slot else (T, K)) and ids.shape == (T, A) and ids.dtype == np.int32
    assert np.bincount(ids.reshape(-1), minlength=E).tolist() == list(counts) and len(counts) == E and T * A <= cases.MAX_PAIRS
    rows = x.reshape(-1, K)
    assert (cases.to_dtype(rows, x_dtype).double().numpy() == rows).all()
    codes, scales = cases.quantize_experts(w)
    assert (cases.decode_experts(codes, scales) == w).all()
    w2, c2, s2 = w.reshape(E * N, K), codes.reshape(E * N, -1), scales.reshape(E * N, -1)
    unit = 2.0 ** -4                                          # x and w are multiples of 2^-2; the unscaled products too (values of 2^-1 up)
    total = np.abs(rows) @ np.abs(w2).T + (0 if bias is None else np.abs(bias).reshape(-1)[None, :])
    assert total.max() / unit < 2.0 ** 24, total.max()
    P, scaled = _walk(rows, c2, s2)
    assert (P % 2.0 ** -3 == 0).all() and (scaled % unit == 0).all() and np.abs(P).max() < 2.0 ** 20
    assert (scaled.sum(axis=2) == rows @ w2.T).all()
    assert _normal_or_zero(rows) and _normal_or_zero(P) and _normal_or_zero(scaled) and _normal_or_zero(rows @ w2.T)
    want = cases.reference_f64(x, w, bias, ids)
    assert want.shape == (T * A, N) and _normal_or_zero(want) and (want % unit == 0).all()


def test_the_exact_cases_cover_every_listed_size():
    Es, Ns, Ks = ({c[i] for c in cases.EXACT_CASES} for i in range(3))
    assert Es == {1, 2, 5, 9} and Ns >= {1, 15, 16, 17, 33} and Ks == {32, 64, 96, 128, 160, 1056, 2080}
    assert Ks == {32, 64, cases.STEP - 32, cases.STEP, cases.STEP + 32, cases.ROUND + 32, 2 * cases.ROUND + 32}
    assert {c[3] * c[4] for c in cases.EXACT_CASES} >= {1, cases.SCAN - 1, cases.SCAN, cases.SCAN + 1, 70, cases.MAX_PAIRS}
    big = [c for c in cases.EXACT_CASES if c[3] * c[4] == cases.MAX_PAIRS]
    assert [c[:3] for c in big] == [(2, 5, 32)]
    assert {(c[6], c[7]) for c in cases.EXACT_CASES} == {(xd, od) for xd in cases.X16 for od in cases.DTYPES}
    assert {(c[8], c[9]) for c in cases.EXACT_CASES} == {(b, s) for b in (True, False) for s in (True, False)}
    # single experts with 0, 1, 15, 16, 17 and 33 pairs inside ONE call, with a shared and with a per-slot input
    assert cases.EDGE_COUNTS == (0, 1, 15, 16, 17, 33)
    assert {c[9] for c in cases.EXACT_CASES if set(c[5]) >= set(cases.EDGE_COUNTS)} == {True, False}
    assert any(max(c[5]) == c[3] * c[4] and c[0] > 1 for c in cases.EXACT_CASES)             # all pairs on one expert
    assert any(set(c[5]) == {1} and c[0] == 9 for c in cases.EXACT_CASES)                    # every pair on a different expert
    assert any(c[0] == 1 and c[4] > 1 for c in cases.EXACT_CASES)                            # the same expert twice within a token
    assert cases.launch_text(torch.bfloat16, False, 32, 64) == "mx_experts bf16 shared E32 P64"
    assert cases.launch_text(torch.float16, True, 4, 5) == "mx_experts f16 slot E4 P5"


def test_the_walk_table_has_the_steps_tails_waves_and_passes_it_names():
    """From K by formula: step c of ceil(KB / 4) runs on wave c % 8 in pass c // 8; the last step holds KB - 4 (steps - 1) blocks"""
    want = {352: (3, 3, 2, 0), 448: (4, 2, 3, 0), 992: (8, 3, 7, 0), 1024: (8, 4, 7, 0), 1216: (10, 2, 1, 1), 2016: (16, 3, 7, 1),
            2048: (16, 4, 7, 1), 2880: (23, 2, 6, 2), 3104: (25, 1, 0, 3)}
    assert tuple(want) == cases.WALK_KS
    walks = {}
    for K in cases.WALK_KS:
        assert K % 32 == 0
        KB = K // 32
        steps = (KB + 3) // 4                                # csrc/mx_decode.h tile_walk, csrc/moegemm_kernels.hip
        owner = [c % 8 for c in range(steps)]
        tail = sum(1 for q in range(4) if 4 * (steps - 1) + q < KB)
        walks[K] = (steps, tail, owner[-1], sum(1 for c in range(steps - 1) if c % 8 == owner[-1]))
        got = cases.walk_of(K)
        assert (got["steps"], got["tail"], got["wave"], got["passes"]) == walks[K] == want[K], K
        assert got["first"] == 4 * (steps - 1) and cases.walk_nan_blocks(K) == tuple(sorted({got["first"], KB - 1}))
        assert cases.walk_bad_ks(K) == (128 * (steps - 1), K - 1)
    assert {w[1] for w in walks.values()} == {1, 2, 3, 4}
    ragged = {w[2] for w in walks.values() if w[1] < 4}
    assert 0 in ragged and 7 in ragged and ragged & set(range(1, 7))
    assert {w[3] for w in walks.values()} == {0, 1, 2, 3}
    assert {K for K in cases.WALK_KS if K % cases.ROUND == 0} == {1024, 2048} and 2880 in cases.WALK_KS
    assert any(w[0] >= 25 for w in walks.values())            # tile_walk's second outer iteration has a live u = 1 step from 25 steps on
    assert not set(cases.WALK_KS) & {c[2] for c in cases.EXACT_CASES}
    # what the older table leaves out, by the same formula: ragged steps on waves 0 and 1 only, of 2 or 3 blocks only alone on wave 0
    old = {K: cases.walk_of(K) for K in sorted({c[2] for c in cases.EXACT_CASES})}
    assert {w["wave"] for w in old.values() if w["tail"] < 4} == {0, 1} and {w["tail"] for w in old.values() if w["steps"] > 1} == {1}
    assert max(w["passes"] for w in old.values()) == 2
    assert set(cases.WALK_NONFINITE_KS) <= set(cases.WALK_KS) and all(cases.walk_of(K)["wave"] != 0 and cases.walk_of(K)["tail"] < 4 for K in cases.WALK_NONFINITE_KS)
    assert all(len(cases.walk_nan_blocks(K)) == 2 for K in cases.WALK_NONFINITE_KS)


@pytest.mark.parametrize("index", range(len(cases.WALK_CASES)))
def test_every_walk_case_is_exact_in_f32_in_any_order(index):
    case = cases.WALK_CASES[index]
    assert case[:6] == (3, 17, cases.WALK_KS[index], 11, 3, (17, 0, 16)) and case[1] == cases.TILE + 1
    assert 3104 * 144 / 2.0 ** -4 < 2.0 ** 24                 # the worst case of lossless rows at the longest K
    _assert_exact_in_any_order(case, *cases.exact_operands(case, cases.WALK_SEED + index))


def test_the_walk_cases_alternate_every_form():
    W = cases.WALK_CASES
    assert [c[2] for c in W] == list(cases.WALK_KS)
    assert {c[6] for c in W} == set(cases.X16) and {c[7] for c in W} == set(cases.DTYPES) and {c[8] for c in W} == {True, False} == {c[9] for c in W}
    assert all(W[i][6] != W[i + 1][6] and W[i][7] != W[i + 1][7] for i in range(len(W) - 1))
    for K in cases.WALK_NONFINITE_KS:                        # the planted column and expert have a weight at both planted k
        x, w, ids = cases.walk_nan_operands(K)
        assert x.shape == (cases.NAN_SHAPE[3], K) and w.shape == (3, cases.NAN_SHAPE[1], K) and (np.abs(x) @ np.abs(w.reshape(-1, K)).T).max() < 2.0 ** 20


@pytest.mark.parametrize("which", ("low", "high"))
def test_every_wide_case_is_exact_and_normal(which):
    E, N, K, T, A = cases.WIDE_SHAPE
    x, w, codes, scales, ids, a, c = cases.wide_operands(which)
    assert (cases.to_dtype(x, torch.bfloat16).double().numpy() == x).all() and _normal_or_zero(x)
    assert (cases.decode_experts(codes, scales) == w).all()
    assert sorted(ids[0].tolist()) == [0, 1, 2] and ids.shape == (T, A)
    live = (emul.unpack(codes[1], "fp4").reshape(N, K // 32, 32) & 7).any(axis=2)
    nb = K // 32
    ends, union = ({0, 1} if which == "low" else {253, 254}), set()
    for b in (0, nb // 2, nb - 1):                           # the first, the middle and the last block carry the extreme offset t[0]
        seen = set(scales[1][live[:, b], b].tolist())
        assert seen & ends and seen <= (set(range(5)) if which == "low" else set(range(250, 255))), (b, sorted(seen))
        union |= seen
    assert union >= ends, sorted(union)
    every = set(np.unique(scales[1]).tolist())
    assert every >= ({0, 1, 2, 3, 4} if which == "low" else {250, 251, 252, 253, 254}), sorted(every)
    for e in range(E):
        ce = np.roll(c, 1) if e == 0 else c
        P, scaled = _walk(x, codes[e], scales[e])
        unit = np.ldexp(1.0, a[:, None] + ce[None, :] - 4)
        assert (scaled % unit[..., None] == 0).all()
        r = x @ w[e].T
        assert ((np.abs(x) @ np.abs(w[e]).T) / unit).max() < 2.0 ** 24
        assert (scaled.sum(axis=2) == r).all() and (r != 0).all()
        assert _normal_or_zero(P) and _normal_or_zero(scaled) and _normal_or_zero(r)
        assert (np.abs(r) < 2.0 ** 100).all() and (np.abs(r) > 2.0 ** -100).all()


def test_the_ids_nan_random_and_offset_tables():
    E, N, K, T, A = cases.IDS_SHAPE
    assert cases.OUT_OF_RANGE == (-1, E, 2 ** 31 - 1, -2 ** 31) and len(set(cases.OUT_OF_RANGE_PLACES)) == 4
    x, w, bias, ids = cases.ids_operands()
    assert (bias != 0).all() and ids.min() >= 0 and ids.max() < E and (np.abs(x) @ np.abs(w.reshape(E * N, K)).T).max() + 8 < 2.0 ** 20
    E, N, K, T, A = cases.NAN_SHAPE
    x, w, ids = cases.nan_operands()
    assert cases.NAN_BLOCKS == (0, K // 64, K // 32 - 1) and cases.X_BAD_KS == (0, 31, 32, K - 1)
    routed = (ids == cases.NAN_EXPERT).any(axis=1)
    assert routed.any() and not routed.all() and (ids[3] == cases.NAN_EXPERT).all()          # some tokens miss the expert; one has it twice
    assert (ids[cases.X_BAD_TOKEN] != ids[cases.X_BAD_TOKEN][::-1]).any() and (np.abs(x) @ np.abs(w.reshape(E * N, K)).T).max() < 2.0 ** 20
    assert cases.RANDOM_SHAPES == ((5, 3, 4, 33, 1056), (16, 4, 9, 17, 2080)) and {c[1] for c in cases.RANDOM_CASES} == set(cases.X16)
    for shape in cases.RANDOM_SHAPES:
        ids = cases.random_operands(shape, torch.bfloat16)[3]
        assert ids.shape == shape[:2] and all(len(set(row)) == shape[1] for row in ids.tolist())
    for off in cases.OFFSETS:
        assert off["x"] % 16 == 0 and off["w_codes"] % 16 == 0
    assert {o["x"] for o in cases.OFFSETS} == {0, 16, 32, 48} == {o["w_codes"] for o in cases.OFFSETS}
    assert {o["ids"] % 4 for o in cases.OFFSETS} == {0, 1, 2, 3} and any(o["out"] % 2 for o in cases.OFFSETS)
    T, A, E, N, K = cases.CUT_SHAPE
    assert T * A > cases.MAX_PAIRS and (cases.MAX_PAIRS // A) * 2 > T > cases.MAX_PAIRS // A
