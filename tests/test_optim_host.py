"""CPU-side checks of the 8-bit optimizers: the reference's public surface (signatures, defaults, error texts), the state
layout, the launch plan, the host scalars, and the C ABI of libmbnb_optim.so (loads, exports what its header declares,
reports argument errors through status / last error without touching a device)."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _optim():
    from mps_bitsandbytes_amd import optim
    return optim


def test_public_names():
    optim = _optim()
    for n in ("Adam8bit", "AdamW8bit", "Lion8bit", "SGD8bit", "quantize_state", "dequantize_state",
              "quantize_state_unsigned", "dequantize_state_unsigned"):
        assert hasattr(optim, n), n


def test_signatures_and_defaults_match_the_reference():
    optim = _optim()

    def defaults(cls):
        return {k: v.default for k, v in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "params")}

    adam = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, block_size=256, max_grad_norm=None)
    assert defaults(optim.Adam8bit) == adam
    assert defaults(optim.AdamW8bit) == dict(adam, weight_decay=1e-2)
    assert defaults(optim.Lion8bit) == dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0, block_size=256)
    sgd = defaults(optim.SGD8bit)
    assert sgd.pop("lr") is inspect.Parameter.empty
    assert sgd == dict(momentum=0, dampening=0, weight_decay=0, nesterov=False, block_size=256)


@pytest.mark.parametrize("cls,kw,msg", [
    ("Adam8bit", dict(lr=-1), "Invalid learning rate: -1"),
    ("AdamW8bit", dict(eps=-1.0), "Invalid epsilon: -1.0"),
    ("Adam8bit", dict(betas=(1.0, 0.9)), "Invalid beta1: 1.0"),
    ("AdamW8bit", dict(betas=(0.9, -0.1)), "Invalid beta2: -0.1"),
    ("Adam8bit", dict(weight_decay=-1e-3), "Invalid weight_decay: -0.001"),
    ("AdamW8bit", dict(max_grad_norm=0.0), "Invalid max_grad_norm: 0.0"),
    ("Lion8bit", dict(lr=-0.5), "Invalid learning rate: -0.5"),
    ("Lion8bit", dict(betas=(0.9, 1.5)), "Invalid beta2: 1.5"),
    ("SGD8bit", dict(lr=0.1, momentum=-1), "Invalid momentum: -1"),
    ("SGD8bit", dict(lr=0.1, weight_decay=-1), "Invalid weight_decay: -1"),
    ("SGD8bit", dict(lr=0.1, nesterov=True), "Nesterov momentum requires momentum > 0 and zero dampening"),
    ("SGD8bit", dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True), "Nesterov momentum requires momentum > 0 and zero dampening"),
])
def test_value_errors(cls, kw, msg):
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match=re.escape(msg)):
        getattr(_optim(), cls)([p], **kw)


@pytest.mark.parametrize("cls,kw", [("Adam8bit", {}), ("AdamW8bit", {}), ("Lion8bit", {}), ("SGD8bit", dict(lr=0.1, momentum=0.9)),
                                    ("SGD8bit", dict(lr=0.1))])
def test_cpu_parameters_raise_the_package_error(cls, kw):
    p = torch.nn.Parameter(torch.zeros(10))
    p.grad = torch.ones(10)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        getattr(_optim(), cls)([p], **kw).step()


@pytest.mark.parametrize("cls,kw", [("Adam8bit", {}), ("AdamW8bit", {}), ("Lion8bit", {}), ("SGD8bit", dict(lr=0.1))])
def test_sparse_gradients_raise_the_reference_text(cls, kw):
    p = torch.nn.Parameter(torch.zeros(10))
    p.grad = torch.zeros(10).to_sparse()
    with pytest.raises(RuntimeError, match=f"{cls} does not support sparse gradients"):
        getattr(_optim(), cls)([p], **kw).step()


def test_params_without_grad_are_skipped_and_closure_is_called():
    p = torch.nn.Parameter(torch.zeros(10))
    opt = _optim().AdamW8bit([p])
    calls = []
    assert opt.step(lambda: calls.append(1) or 3.5) == 3.5
    assert calls == [1] and len(opt.state[p]) == 0 and torch.equal(p.detach(), torch.zeros(10))


def test_state_layout_after_initialisation():
    from mps_bitsandbytes_amd.optim._base import new_state
    p = torch.zeros(16, 65)
    q, m = new_state(p, 256, signed=True)
    assert q.shape == p.shape and q.dtype == torch.int8 and not q.any()
    assert m.shape == (5,) and m.dtype == torch.float32 and torch.equal(m, torch.full((5,), 1e-8))
    q, m = new_state(p, 100, signed=False)
    assert q.dtype == torch.uint8 and m.shape == (11,) and torch.equal(m, torch.full((11,), 1e-12))
    # the quantisation of zeros by the state utilities gives the same
    optim = _optim()
    q2, m2 = optim.quantize_state(torch.zeros(16, 65), 256)
    assert torch.equal(q2, torch.zeros(16, 65, dtype=torch.int8)) and torch.equal(m2, torch.full((5,), 1e-8))
    q3, m3 = optim.quantize_state_unsigned(torch.zeros(16, 65), 100)
    assert q3.dtype == torch.uint8 and torch.equal(m3, torch.full((11,), 1e-12))


def test_state_utilities_round_trip():
    optim = _optim()
    x = torch.randn(1000)
    q, a = optim.quantize_state(x, 256)
    assert (optim.dequantize_state(q, a, 256) - x).abs().max() <= a.max() / 127
    v = x * x
    q, mx = optim.quantize_state_unsigned(v, 64)
    assert (optim.dequantize_state_unsigned(q, mx, 64) - v).abs().max() <= mx.max() * 2 / 255


class _StubLib:
    """Stands in for libmbnb_optim.so: records what each mbnb_optim_step call receives (no device involved)."""

    def __init__(self):
        self.calls = []

    def mbnb_optim_step(self, kind, pdt, gdt, block_size, scalars, table, n, flags, stream):
        from mps_bitsandbytes_amd import _optim_native as on
        sc = scalars._obj
        self.calls.append(dict(kind=kind, pdt=pdt, gdt=gdt, block_size=block_size, n=n, flags=flags,
                               scalars={f: getattr(sc, f) for f, _ in on.Scalars._fields_},
                               table=[{f: getattr(table[i], f) for f, _ in on.TensorDesc._fields_} for i in range(n)]))
        return 0


@pytest.fixture
def stub(monkeypatch):
    """Run the optimizers' real host path on CPU tensors: device gate and stream query bypassed, library call recorded."""
    from mps_bitsandbytes_amd import _native, _optim_native
    from mps_bitsandbytes_amd.optim import _base
    lib = _StubLib()
    monkeypatch.setattr(_base, "_check_device", lambda t, op: None)
    monkeypatch.setattr(_native, "stream_ptr", lambda dev: None)
    monkeypatch.setattr(_optim_native, "lib", lambda: lib)
    _optim_native.reset_launch_log()
    return lib


def _params(shapes, dtype=torch.float16, grad_dtype=None):
    ps = []
    for shp in shapes:
        p = torch.nn.Parameter(torch.zeros(shp, dtype=dtype))
        p.grad_dtype = None
        p.grad = torch.zeros(shp, dtype=grad_dtype or dtype)
        ps.append(p)
    return ps


def test_step_chunks_at_the_kernarg_limit_in_tensor_order(stub):
    """What AdamW8bit.step hands the library: at most 48 descriptors per call, every tensor once, in group order, per dtype pair."""
    from mps_bitsandbytes_amd import _optim_native as on
    assert on.MAX_TENSORS == 48
    shapes = [(1,), (255,), (256,), (257,), (3, 100), (65536,), (16, 96)] * 20       # 140 tensors
    ps = _params(shapes) + _params([(5,)] * 3, torch.bfloat16)
    _optim().AdamW8bit(ps).step()
    f16 = [c for c in stub.calls if c["pdt"] == on.F16]
    bf16 = [c for c in stub.calls if c["pdt"] == on.BF16]
    assert [c["n"] for c in f16] == [48, 48, 44] and [c["n"] for c in bf16] == [3]
    ptrs = [d["param"] for c in f16 for d in c["table"]]
    assert ptrs == [p.data_ptr() for p in ps[:140]]
    assert [d["numel"] for c in f16 for d in c["table"]] == [p.numel() for p in ps[:140]]
    assert all(c["block_size"] == 256 and c["kind"] == on.ADAMW for c in stub.calls)
    assert [n for _, _, _, n in on.launch_log] == [48, 48, 44, 3]
    # the block layout the library forms from those numels: each tensor starts its own blocks (none straddles two)
    chunks = on.plan([p.numel() for p in ps[:140]], 256)
    for c in chunks:
        first = 0
        for i, f, nb in c:
            assert f == first and nb == math.ceil(ps[i].numel() / 256)
            first += nb
    # the kernel-argument structure fits 4 KiB: scalars + header + 49 offsets + 48 descriptors
    assert ctypes.sizeof(on.Scalars) == 40 and ctypes.sizeof(on.TensorDesc) == 64 == on.DESC_DTYPE.itemsize
    assert ctypes.sizeof(on.Scalars) + 16 + 8 * (on.MAX_TENSORS + 1) + on.MAX_TENSORS * ctypes.sizeof(on.TensorDesc) <= 4096


def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


def _alpha(x, dtype):
    return torch.tensor(x, dtype=torch.float32).to(dtype).to(torch.float32).item()


@pytest.mark.parametrize("cls", ["Adam8bit", "AdamW8bit"])
def test_adam_scalars_are_the_reference_formulas(stub, cls):
    """The scalars Adam8bit / AdamW8bit build, per step and per tensor: the reference's double formulas
    (adam8bit.py: bias_correction1/2, step_size, bias_correction2 ** 0.5, 1 - lr * wd) rounded once to f32."""
    from mps_bitsandbytes_amd import _optim_native as on
    lr, b1, b2, eps, wd = 3e-3, 0.85, 0.995, 1e-7, 0.02
    a, b = _params([(300,), (40,)])
    opt = getattr(_optim(), cls)([a, b], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for step in range(1, 4):
        if step == 2:
            b.grad = None                      # b misses a step: its own step count
        elif step == 3:
            b.grad = torch.zeros(40, dtype=torch.float16)
        opt.step()
    steps = [[1, 1], [2], [3, 2]]
    for call, want_steps in zip(stub.calls, steps):
        sc = call["scalars"]
        assert call["kind"] == (on.ADAM if cls == "Adam8bit" else on.ADAMW)
        assert sc["beta1"] == _f32(b1) and sc["one_minus_beta1"] == _f32(1 - b1)
        assert sc["beta2"] == _f32(b2) and sc["one_minus_beta2"] == _f32(1 - b2) and sc["eps"] == _f32(eps)
        assert sc["weight_decay"] == _f32(wd) and sc["decay"] == _f32(1 - lr * wd) and sc["flags"] == on.WEIGHT_DECAY
        for d, t in zip(call["table"], want_steps):
            assert d["bc2_sqrt"] == _f32(math.sqrt(1 - b2 ** t))
            assert d["neg_step_size"] == _f32(-(lr / (1 - b1 ** t)))
    assert opt.state[a]["step"] == 3 and opt.state[b]["step"] == 2
    opt.param_groups[0]["weight_decay"] = 0
    opt.step()
    assert stub.calls[-1]["scalars"]["flags"] == 0          # the reference skips the decay when wd == 0


@pytest.mark.parametrize("pdt,gdt", [(torch.float16, torch.float16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)])
def test_lion_and_sgd_scalars(stub, pdt, gdt):
    """Lion: -lr as the parameter dtype rounds an alpha; SGD: -lr in the parameter dtype, wd in the gradient dtype."""
    from mps_bitsandbytes_amd import _optim_native as on
    lr, b1, b2, wd = 1e-2, 0.9, 0.99, 0.1
    (p,) = _params([(70,)], pdt, gdt)
    _optim().Lion8bit([p], lr=lr, betas=(b1, b2), weight_decay=wd).step()
    sc = stub.calls[-1]["scalars"]
    assert stub.calls[-1]["kind"] == on.LION and stub.calls[-1]["table"][0]["state2"] is None
    assert sc["beta1"] == _f32(b1) and sc["one_minus_beta1"] == _f32(1 - b1)
    assert sc["beta2"] == _f32(b2) and sc["one_minus_beta2"] == _f32(1 - b2)
    assert sc["decay"] == _f32(1 - lr * wd) and sc["neg_lr"] == _alpha(-lr, pdt) and sc["flags"] == on.WEIGHT_DECAY
    (q,) = _params([(70,)], pdt, gdt)
    _optim().SGD8bit([q], lr=lr, momentum=0.8, dampening=0.25, weight_decay=wd).step()
    sc = stub.calls[-1]["scalars"]
    assert stub.calls[-1]["kind"] == on.SGD_MOMENTUM
    assert sc["beta1"] == _f32(0.8) and sc["one_minus_beta1"] == _f32(0.75)
    assert sc["neg_lr"] == _alpha(-lr, pdt) and sc["weight_decay"] == _alpha(wd, gdt) and sc["flags"] == on.WEIGHT_DECAY
    _optim().SGD8bit([q], lr=lr, momentum=0.8, nesterov=True).step()
    assert stub.calls[-1]["kind"] == on.SGD_NESTEROV and stub.calls[-1]["scalars"]["flags"] == 0


def test_state_that_does_not_fit_the_parameter_is_refused_before_any_launch(stub):
    """The kernel addresses the state through raw pointers sized by the parameter; state of another shape, dtype,
    block size or layout must raise, never reach it."""
    optim = _optim()
    (small,) = _params([(8, 64)])
    src = optim.AdamW8bit([small])
    src.step()
    calls = len(stub.calls)
    (big,) = _params([(16, 64)])                 # a rank-8 adapter's checkpoint loaded into a rank-16 model
    dst = optim.AdamW8bit([big])
    dst.load_state_dict(src.state_dict())
    with pytest.raises(ValueError, match="do not fit the parameter"):
        dst.step()
    (p,) = _params([(1000,)])
    opt = optim.AdamW8bit([p])
    opt.step()
    calls = len(stub.calls)
    opt.param_groups[0]["block_size"] = 64       # block_size changed after the state exists
    with pytest.raises(ValueError, match="maxima do not fit"):
        opt.step()
    opt.param_groups[0]["block_size"] = 0
    with pytest.raises(ValueError, match="block_size must be a positive int"):
        opt.step()
    opt.param_groups[0]["block_size"] = 256
    st = opt.state[p]
    good = st["exp_avg_int8"]
    st["exp_avg_int8"] = good.to(torch.int16)
    with pytest.raises(ValueError, match="codes do not fit"):
        opt.step()
    st["exp_avg_int8"] = torch.zeros(2000, dtype=torch.int8)[::2]
    with pytest.raises(ValueError, match="non-contiguous"):
        opt.step()
    st["exp_avg_int8"] = good
    del st["exp_avg_sq_max"]
    with pytest.raises(ValueError, match="missing"):
        opt.step()
    assert len(stub.calls) == calls              # nothing reached the library
    (m,) = _params([(100,)])
    sgd = optim.SGD8bit([m], lr=0.1, momentum=0.9)
    sgd.step()
    sgd.state[m]["momentum_absmax"] = torch.zeros(2, dtype=torch.float16)
    with pytest.raises(ValueError, match="maxima do not fit"):
        sgd.step()


def test_load_state_dict_does_not_share_tensors_with_the_source(stub):
    optim = _optim()
    (a,) = _params([(300,)], torch.float32)
    src = optim.AdamW8bit([a])
    src.step()
    (b,) = _params([(300,)], torch.float32)
    dst = optim.AdamW8bit([b])
    dst.load_state_dict(src.state_dict())
    for k in ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"):
        assert dst.state[b][k].data_ptr() != src.state[a][k].data_ptr(), k
        assert torch.equal(dst.state[b][k], src.state[a][k]), k


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text)))


def _exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(rf"\b({prefix}[a-z0-9_]*)$", out, flags=re.M)))


def test_optim_library_exports_exactly_its_header():
    from mps_bitsandbytes_amd import _optim_native as on
    lib = on.lib()
    names = _declared("mbnb_optim.h")
    assert names == sorted(on.EXPORTED_SYMBOLS) == ["mbnb_optim_abi_version", "mbnb_optim_last_error", "mbnb_optim_step"]
    assert _exported(on.LIB_PATH, "mbnb_") == names
    assert lib.mbnb_optim_abi_version() == on.ABI_VERSION == 1
    assert re.search(r"#define MBNB_OPTIM_MAX_TENSORS 48\b", open(os.path.join(ROOT, "include", "mbnb_optim.h")).read())


def test_main_library_exports_are_unchanged():
    """libmbnb_hip.so keeps its 30 version-2 symbols: none of the optimizer entry points landed there."""
    from mps_bitsandbytes_amd import _native
    exported = _exported(_native.LIB_PATH, "mbnb_")
    assert exported == sorted(_native.EXPORTED_SYMBOLS) and len(exported) == 30
    assert not [n for n in exported if "optim" in n]


def test_argument_errors_use_status_and_last_error():
    from mps_bitsandbytes_amd import _optim_native as on
    lib = on.lib()
    s = on.Scalars()
    t = on.TensorDesc(256, 256, 256, 256, 256, 256, 1000, 1.0, -1.0)
    table = (on.TensorDesc * 1)(t)
    assert lib.mbnb_optim_step(7, 0, 0, 256, ctypes.byref(s), table, 1, 0, None) == -1 and b"kind" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 5, 5, 256, ctypes.byref(s), table, 1, 0, None) == -1 and b"dtype" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 2, 0, 256, ctypes.byref(s), table, 1, 0, None) == -1 and b"gradient dtype" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 0, 0, 0, ctypes.byref(s), table, 1, 0, None) == -1 and b"block_size" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), table, 49, 0, None) == -1 and b"0..48" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), table, 1, 4, None) == -1 and b"flags" in lib.mbnb_optim_last_error()
    assert lib.mbnb_optim_step(0, 0, 0, 256, None, table, 1, 0, None) == -1
    bad = (on.TensorDesc * 1)(on.TensorDesc(256, 256, 256, 256, None, None, 1000, 1.0, -1.0))   # Adam without its second moment
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), bad, 1, 0, None) == -1 and b"NULL" in lib.mbnb_optim_last_error()
    mis = (on.TensorDesc * 1)(on.TensorDesc(264, 256, 256, 256, 256, 256, 1000, 1.0, -1.0))   # parameter 8-byte aligned only
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), mis, 1, 0, None) == -1 and b"misaligned" in lib.mbnb_optim_last_error()
    neg = (on.TensorDesc * 1)(on.TensorDesc(256, 256, 256, 256, 256, 256, -1, 1.0, -1.0))
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), neg, 1, 0, None) == -2
    # empty work is a no-op success, without a device
    assert lib.mbnb_optim_step(0, 0, 0, 256, ctypes.byref(s), table, 0, 0, None) == 0
    empty = (on.TensorDesc * 1)(on.TensorDesc(None, None, None, None, None, None, 0, 1.0, -1.0))
    assert lib.mbnb_optim_step(2, 1, 2, 100, ctypes.byref(s), empty, 1, 0, None) == 0
    with pytest.raises(RuntimeError, match="status -1"):
        on.check(-1, "unit")


def test_optimizers_never_import_the_oracle():
    pkg = os.path.join(ROOT, "mps_bitsandbytes_amd", "optim")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
