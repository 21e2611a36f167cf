"""The weight-only decode of block-scaled FP8 weights without a GPU: exports, refusals and the Python surface."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8dec_native as fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 0, 1, 2


def test_header_binding_and_library_agree_on_the_exports():
    header = open(os.path.join(ROOT, "include", "mbnb_fp8dec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mbnb_fp8dec_\w+)\s*\(", code)))
    out = subprocess.run(["nm", "-D", "--defined-only", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert declared == sorted(fn.EXPORTED_SYMBOLS) == sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))
    assert len(declared) == 4 and fn.lib().mbnb_fp8dec_abi_version() == fn.ABI_VERSION == int(re.search(r"MBNB_FP8DEC_ABI_VERSION (\d+)", header).group(1))
    needed = subprocess.run(["readelf", "-d", fn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in "".join(line for line in needed.splitlines() if "NEEDED" in line)
    for macro, value in dict(BLOCK=fn.BLOCK, ROWS=fn.ROWS).items():
        assert int(re.search(rf"#define MBNB_FP8DEC_{macro} (\d+)", header).group(1)) == value


P = 4096            # a pointer that is aligned and never dereferenced: every call below is refused, or has no rows
ARGS = dict(x=P, xdt=BF16, M=4, K=32, w=P, sW=P, N=8, bias=None, bdt=BF16, out=P, odt=BF16)      # in the order of the C signature


def _call(**kw):
    return fn.lib().mbnb_fp8dec_linear_weight_only(*{**ARGS, **kw}.values(), None)


REFUSALS = [
    (dict(xdt=3), fn.ERR_ARG, "unknown dtype"), (dict(odt=-1), fn.ERR_ARG, "unknown dtype"), (dict(bias=P, bdt=7), fn.ERR_ARG, "unknown dtype"),
    (dict(K=40), fn.ERR_SHAPE, "multiple of 16"), (dict(K=0), fn.ERR_SHAPE, "K = 0"), (dict(K=-16), fn.ERR_SHAPE, "K = -16"),
    (dict(N=0), fn.ERR_SHAPE, "N = 0"), (dict(M=-2), fn.ERR_SHAPE, "M = -2"),
    (dict(M=0, K=1 << 31), fn.ERR_SHAPE, "exceeds 2^31 - 1"), (dict(M=0, N=1 << 31), fn.ERR_SHAPE, "exceeds 2^31 - 1"),
    (dict(x=None), fn.ERR_ARG, "NULL"), (dict(w=None), fn.ERR_ARG, "NULL"), (dict(sW=None), fn.ERR_ARG, "NULL"), (dict(out=None), fn.ERR_ARG, "NULL"),
    (dict(x=P + 8), fn.ERR_ARG, "misaligned x or w"), (dict(w=P + 4), fn.ERR_ARG, "misaligned x or w"),
    (dict(sW=P + 2), fn.ERR_ARG, "misaligned sW, out or bias"), (dict(out=P + 1), fn.ERR_ARG, "misaligned sW, out or bias"),
    (dict(out=P + 2, odt=F32), fn.ERR_ARG, "misaligned sW, out or bias"), (dict(bias=P + 2, bdt=F32), fn.ERR_ARG, "misaligned sW, out or bias"),
    # 2^27 tiles of 16 weight rows x 2^27 chunks of 16 rows (the MFMA form); 2^29 tiles of 4 x 2^30 chunks of 4 rows (f32: the FMA form)
    (dict(M=1 << 31, N=(1 << 31) - 1), fn.ERR_SHAPE, "workgroups exceed one launch"),
    (dict(xdt=F32, M=1 << 32, N=(1 << 31) - 1), fn.ERR_SHAPE, "workgroups exceed one launch"),
    (dict(M=(1 << 63) - 1), fn.ERR_SHAPE, "workgroups exceed one launch"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_every_refusal_is_a_status_and_a_text_before_any_hip_call(index):
    args, status, text = REFUSALS[index]
    assert _call(**args) == status and text in fn.lib().mbnb_fp8dec_last_error().decode(), (args, fn.lib().mbnb_fp8dec_last_error())


def test_no_rows_is_a_no_op():
    assert _call(M=0, x=None, w=None, sW=None, out=None) == 0


def test_signature_and_refusals_of_the_python_surface():
    f = bnb.linear_fp8_block_weight_only
    sig = inspect.signature(f).parameters
    assert list(sig) == ["input", "weight", "weight_scales", "bias", "dtype"] and sig["dtype"].default is None and sig["bias"].default is None
    assert bnb.functional.linear_fp8_block_weight_only is f and f.__name__ in bnb.__all__
    x, w, s = torch.zeros(2, 32), torch.zeros(8, 32, dtype=torch.uint8), torch.ones(1, 1)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        f(x, w, s)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x.clone().requires_grad_(), w, s)
    with pytest.raises(NotImplementedError, match="inference-only"):
        f(x, w, s, bias=torch.zeros(8, requires_grad=True))


def test_act_format_selects_the_forward_and_leaves_the_module_as_it_was(monkeypatch):
    assert bnb.LinearFP8Block.act_format == "fp8"
    layer, x, calls = bnb.LinearFP8Block(32, 8, bias=True), torch.zeros(2, 32), []
    keys = sorted(layer.state_dict())
    for name in ("linear_fp8_block", "linear_fp8_block_weight_only"):
        monkeypatch.setattr(bnb.functional, name, lambda *a, _name=name: calls.append((_name, a)) or a[0])
    layer(x)
    layer.act_format = "none"
    layer(x)
    assert [c[0] for c in calls] == ["linear_fp8_block", "linear_fp8_block_weight_only"]
    assert all(a[0] is x and a[1] is layer.weight and a[2] is layer.weight_scale_inv and a[3] is layer.bias for _, a in calls)
    layer.act_format = "fp4"
    with pytest.raises(ValueError, match="'fp8', 'none'"):           # before any device work: neither function is reached
        layer(x)
    assert len(calls) == 2 and sorted(layer.state_dict()) == keys == ["bias", "weight", "weight_scale_inv"]
    assert bnb.LinearFP8Block.act_format == "fp8" and bnb.LinearFP8Block(32, 8).act_format == "fp8"
