"""The block-scaled FP8 linear without a GPU: exports, refusals, workspace sizes and the Python surface."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8blk_native as fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 0, 1, 2


def test_header_binding_and_library_agree_on_the_exports():
    header = open(os.path.join(ROOT, "include", "mbnb_fp8blk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_fp8blk_\w+)\s*\(", code)))
    out = subprocess.run(["nm", "-D", "--defined-only", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert declared == sorted(fn.EXPORTED_SYMBOLS) == sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))
    assert len(declared) == 8 and fn.lib().mbnb_fp8blk_abi_version() == fn.ABI_VERSION == int(re.search(r"MBNB_FP8BLK_ABI_VERSION (\d+)", header).group(1))
    needed = subprocess.run(["readelf", "-d", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in "".join(line for line in needed.splitlines() if "NEEDED" in line)
    for macro, value in dict(BLOCK=fn.BLOCK, TILE_M=fn.TM, TILE_N=fn.TN, K_STEP=fn.KS, STEPS_IN_FLIGHT=fn.STEPS_IN_FLIGHT).items():
        assert int(re.search(rf"#define MBNB_FP8BLK_{macro} (\d+)", header).group(1)) == value


P = 4096            # a pointer that is aligned and never dereferenced: every call below is refused, or has no rows
ARGS = {      # in the order of the C signature; the stream (NULL) follows
    "quantize_groups": dict(x=P, xdt=F32, M=4, K=32, q=P, s=P),
    "quantize_blocks": dict(x=P, xdt=F32, M=4, K=32, q=P, s=P),
    "matmul": dict(a=P, sA=P, M=4, K=32, w=P, sW=P, N=8, bias=None, bdt=BF16, out=P, odt=BF16),
    "linear": dict(x=P, xdt=BF16, M=4, K=32, w=P, sW=P, N=8, bias=None, bdt=BF16, out=P, odt=BF16, ws=P, wsb=1 << 20),
}


def _call(name, **kw):
    return getattr(fn.lib(), "mbnb_fp8blk_" + name)(*{**ARGS[name], **kw}.values(), None)


REFUSALS = [(q, *r) for q in ("quantize_groups", "quantize_blocks") for r in (
    (dict(xdt=3), fn.ERR_ARG, "unknown dtype"), (dict(K=24), fn.ERR_SHAPE, "multiple of 16"), (dict(K=0), fn.ERR_SHAPE, "K = 0"),
    (dict(M=-1), fn.ERR_SHAPE, " = -1"), (dict(M=1 << 31), fn.ERR_SHAPE, "exceed one launch"), (dict(q=None), fn.ERR_ARG, "NULL"),
    (dict(x=P + 8), fn.ERR_ARG, "misaligned input or q"), (dict(q=P + 4), fn.ERR_ARG, "misaligned input or q"), (dict(s=P + 2), fn.ERR_ARG, "misaligned scales"))] + [
    ("matmul", dict(odt=-1), fn.ERR_ARG, "unknown dtype"), ("matmul", dict(bias=P, bdt=7), fn.ERR_ARG, "unknown dtype"),
    ("matmul", dict(K=40), fn.ERR_SHAPE, "multiple of 16"), ("matmul", dict(K=-16), fn.ERR_SHAPE, "K = -16"),
    ("matmul", dict(N=0), fn.ERR_SHAPE, "N = 0"), ("matmul", dict(M=-2), fn.ERR_SHAPE, "M = -2"),
    ("matmul", dict(M=1 << 30, N=1 << 30), fn.ERR_SHAPE, "N = "), ("matmul", dict(a=None), fn.ERR_ARG, "NULL a or sA"),
    ("matmul", dict(sW=None), fn.ERR_ARG, "NULL w, sW or out"), ("matmul", dict(a=P + 1), fn.ERR_ARG, "misaligned a"),
    ("matmul", dict(sA=P + 2), fn.ERR_ARG, "misaligned sA"), ("matmul", dict(w=P + 8), fn.ERR_ARG, "misaligned w"),
    ("matmul", dict(out=P + 1), fn.ERR_ARG, "misaligned sW, out or bias"),
    ("linear", dict(xdt=5), fn.ERR_ARG, "unknown dtype"), ("linear", dict(K=8), fn.ERR_SHAPE, "multiple of 16"),
    ("linear", dict(x=None), fn.ERR_ARG, "NULL x"), ("linear", dict(x=P + 2), fn.ERR_ARG, "misaligned x"),
    ("linear", dict(w=None), fn.ERR_ARG, "NULL w, sW or out"), ("linear", dict(ws=None), fn.ERR_WORKSPACE, "workspace of 0 bytes, 512 needed"),
    ("linear", dict(wsb=511), fn.ERR_WORKSPACE, "workspace of 511 bytes, 512 needed"), ("linear", dict(ws=P + 8), fn.ERR_ARG, "misaligned workspace"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_every_refusal_is_a_status_and_a_text_before_any_hip_call(index):
    name, args, status, text = REFUSALS[index]
    assert _call(name, **args) == status and text in fn.lib().mbnb_fp8blk_last_error().decode(), (args, fn.lib().mbnb_fp8blk_last_error())


def test_no_rows_is_a_no_op_and_the_workspace_is_codes_then_scales():
    for q in ("quantize_groups", "quantize_blocks"):
        assert _call(q, M=0, x=None, q=None, s=None) == 0
    assert _call("matmul", M=0, a=None, sA=None, w=None, sW=None, out=None) == 0
    assert _call("linear", M=0, x=None, w=None, sW=None, out=None, ws=None, wsb=0) == 0 == fn.workspace_bytes(0, 16)
    # 4 x 32: 128 -> 256 of codes, 4 x 1 scales -> 256; 33 x 1024: 33 x 8 scales = 1056 -> 1280; 5 x 400: 2000 -> 2048, 5 x 4 -> 256
    assert fn.workspace_bytes(4, 32) == 512 and fn.workspace_bytes(33, 1024) == 33 * 1024 + 1280 and fn.workspace_bytes(5, 400) == 2048 + 256
    assert fn.lib().mbnb_fp8blk_workspace_bytes(4, 8) == fn.ERR_SHAPE


def test_signatures_and_refusals_of_the_python_surface():
    for f, names, default in ((bnb.quantize_fp8_groups, ["tensor"], None), (bnb.quantize_fp8_blocks, ["tensor"], None),
                              (bnb.linear_fp8_block, ["input", "weight", "weight_scales", "bias", "dtype"], None),
                              (bnb.matmul_fp8_block, ["A", "A_scales", "weight", "weight_scales", "bias", "dtype"], torch.bfloat16)):
        sig = inspect.signature(f).parameters
        assert list(sig) == names and getattr(bnb.functional, f.__name__) is f and f.__name__ in bnb.__all__
        assert "dtype" not in sig or sig["dtype"].default is default
    assert "LinearFP8Block" in bnb.__all__ and "LinearFP8Block" in bnb.nn.__all__ and bnb.nn.LinearFP8Block is bnb.LinearFP8Block
    x, w, s = torch.zeros(2, 32), torch.zeros(8, 32, dtype=torch.uint8), torch.ones(1, 1)
    for call in (lambda: bnb.quantize_fp8_groups(x), lambda: bnb.quantize_fp8_blocks(x), lambda: bnb.linear_fp8_block(x, w, s),
                 lambda: bnb.matmul_fp8_block(w, torch.ones(8, 1), w, s), lambda: bnb.LinearFP8Block(32, 8)(x)):
        with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
            call()
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.linear_fp8_block(x.requires_grad_(), w, s)
    with pytest.raises(NotImplementedError, match="inference-only"):
        bnb.matmul_fp8_block(w, torch.ones(8, 1), w, s, bias=torch.zeros(8, requires_grad=True))


def test_linear_fp8_block_loads_a_checkpoint_state_dict():
    assert list(inspect.signature(bnb.LinearFP8Block.__init__).parameters)[1:4] == ["in_features", "out_features", "bias"]
    layer, bare = bnb.LinearFP8Block(400, 129, bias=True), bnb.LinearFP8Block(400, 129)
    assert sorted(layer.state_dict()) == ["bias", "weight", "weight_scale_inv"] and sorted(bare.state_dict()) == ["weight", "weight_scale_inv"]
    assert layer.weight.dtype == torch.uint8 and tuple(layer.weight_scale_inv.shape) == (2, 4) and not list(layer.parameters())
    codes = torch.arange(129 * 400, dtype=torch.int64).remainder(0x7F).to(torch.uint8).reshape(129, 400)
    state = {"weight": codes.view(torch.float8_e4m3fn), "weight_scale_inv": torch.rand(2, 4)}        # as a checkpoint holds them
    bare.load_state_dict(state, strict=True)
    assert bare.weight.dtype == torch.uint8 and torch.equal(bare.weight, codes) and torch.equal(bare.weight_scale_inv, state["weight_scale_inv"])
