"""CPU-side checks of the paged optimizers and libmbnb_paged.so, without a GPU: the public names and the root `__all__`, signatures,
defaults and error texts, the C ABI (loads, exports what include/mbnb_paged.h declares, argument errors as a status before any
device access), the page plan, and the numpy emulation (tests/paged_emul.py) against the reference's three classes run on CPU
tensors (tests/golden/g14_paged.npz), step by step from the reference's own state."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, _optim_native, _paged_native, optim
from mps_bitsandbytes_amd.optim import paged
from tests import paged_cases, paged_emul as emul

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
HEADER = os.path.join(ROOT, "include", "mbnb_paged.h")

# the reference's root __all__ (mps_bitsandbytes/__init__.py), a list of names
REFERENCE_ROOT_OPTIM = ["Adam8bit", "AdamW8bit", "Lion8bit", "SGD8bit", "PagedAdam", "PagedAdamW", "PagedLion", "quantize_state",
                        "dequantize_state"]


# ----------------------------------------------------------------------------- the public surface
def test_names_are_exported_from_optim_and_the_package_root():
    for name in ("PagedAdam", "PagedAdamW", "PagedLion"):
        assert getattr(optim, name) is getattr(paged, name) and name in optim.__all__
    for name in REFERENCE_ROOT_OPTIM:
        assert getattr(bnb, name) is getattr(optim, name), name
        assert name in bnb.__all__, name
    assert issubclass(bnb.PagedAdam, bnb.PagedAdamW) and issubclass(bnb.PagedAdamW, torch.optim.Optimizer)
    assert issubclass(bnb.PagedLion, torch.optim.Optimizer) and not issubclass(bnb.PagedLion, bnb.PagedAdamW)
    assert len(bnb.__all__) == len(set(bnb.__all__))
    for name in bnb.__all__:
        assert hasattr(bnb, name), name


def test_signatures_and_defaults_are_the_references():
    want = {
        "PagedAdamW": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, page_to_cpu=True),
        "PagedAdam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, page_to_cpu=True),
        "PagedLion": dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0, page_to_cpu=True),
    }
    for name, defaults in want.items():
        sig = inspect.signature(getattr(bnb, name).__init__)
        assert list(sig.parameters) == ["self", "params"] + list(defaults), name
        for k, v in defaults.items():
            assert sig.parameters[k].default == v, (name, k)
        o = getattr(bnb, name)([torch.nn.Parameter(torch.zeros(4))])
        assert {k: o.defaults[k] for k in defaults} == defaults
        assert callable(o.synchronize) and o.synchronize() is None
        assert isinstance(type(o)._page_elems, int) and type(o)._page_elems % paged.PAGE_ALIGN == 0 and type(o)._slots == 3


@pytest.mark.parametrize("name", ["PagedAdamW", "PagedAdam", "PagedLion"])
def test_error_texts(name):
    cls = getattr(bnb, name)
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match=r"^Invalid learning rate: -1$"):
        cls(p, lr=-1)
    with pytest.raises(ValueError, match=r"^Invalid beta1: 1\.0$"):
        cls(p, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match=r"^Invalid beta2: -0\.1$"):
        cls(p, betas=(0.9, -0.1))
    if name != "PagedLion":
        with pytest.raises(ValueError, match=r"^Invalid epsilon: -1e-08$"):
            cls(p, eps=-1e-8)
        with pytest.raises(ValueError, match=r"^Invalid weight_decay: -0\.5$"):
            cls(p, weight_decay=-0.5)


@pytest.mark.parametrize("name", ["PagedAdamW", "PagedAdam", "PagedLion"])
@pytest.mark.parametrize("page_to_cpu", [True, False])
def test_cpu_parameters_sparse_gradients_dtypes_and_closures(name, page_to_cpu):
    cls = getattr(bnb, name)
    p = torch.nn.Parameter(torch.zeros(8))
    o = cls([p], page_to_cpu=page_to_cpu)
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        return torch.tensor(3.5)

    assert o.step() is None                              # no gradient anywhere: nothing to do, no device needed
    assert float(o.step(closure)) == 3.5 and calls == [True]
    assert len(o.state) == 0
    p.grad = torch.zeros(8)
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        o.step()
    assert len(o.state[p]) == 0                          # refused before any state exists
    p.grad = torch.zeros(8).to_sparse()
    with pytest.raises(RuntimeError, match=rf"^{name} does not support sparse gradients$"):
        o.step()


def test_paged_module_never_imports_the_oracle_or_a_fallback():
    src = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "optim", "paged.py")).read()
    assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M)
    assert "_paged_native.step(" in src and not re.search(r"\.(addcdiv_|addcmul_|sqrt|mul_|add_)\(", src)


# ----------------------------------------------------------------------------- the C ABI
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


def test_library_exports_exactly_its_header():
    lib = _paged_native.lib()
    names = _declared("mbnb_paged.h")
    assert names == sorted(_paged_native.EXPORTED_SYMBOLS) == ["mbnb_paged_abi_version", "mbnb_paged_last_error", "mbnb_paged_step"]
    assert _exported(_paged_native.LIB_PATH) == names
    assert lib.mbnb_paged_abi_version() == _paged_native.ABI_VERSION == 1
    header = open(HEADER).read()
    assert re.search(r"#define MBNB_PAGED_MAX_SEGMENTS 48\b", header) and _paged_native.MAX_SEGMENTS == 48
    assert re.search(r"MBNB_PAGED_ADAM = 0,", header) and re.search(r"MBNB_PAGED_ADAMW = 1,", header) and re.search(r"MBNB_PAGED_LION = 2,", header)
    assert (_paged_native.ADAM, _paged_native.ADAMW, _paged_native.LION) == (0, 1, 2)
    assert ctypes.sizeof(_paged_native.Segment) == _paged_native.SEG_DTYPE.itemsize == 48
    assert ctypes.sizeof(_paged_native.Scalars) == 40


def test_the_other_libraries_export_what_they_did():
    assert _exported(_optim_native.LIB_PATH) == ["mbnb_optim_abi_version", "mbnb_optim_last_error", "mbnb_optim_step"]
    main = _exported(_native.LIB_PATH)
    assert main == sorted(_native.EXPORTED_SYMBOLS) and len(main) == 30
    assert not [n for n in main if "paged" in n]
    src = open(os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "paged_kernels.hip")).read()
    assert "set_kernel_name" not in src and len(re.findall(r"__global__", src)) == 1


def test_argument_errors_return_a_status_before_any_device_access():
    pn = _paged_native
    lib = pn.lib()
    err = lib.mbnb_paged_last_error
    s = pn.Scalars()
    one = (pn.Segment * 1)(pn.Segment(256, 256, 256, 256, 1000, 1.0, -1.0))
    step = lambda kind, dt, sc, tab, n, flags: lib.mbnb_paged_step(kind, dt, sc, tab, n, flags, None)
    assert step(3, 0, ctypes.byref(s), one, 1, 0) == -1 and b"kind" in err()
    assert step(-1, 0, ctypes.byref(s), one, 1, 0) == -1 and b"kind" in err()
    assert step(0, 3, ctypes.byref(s), one, 1, 0) == -1 and b"dtype" in err()
    assert step(0, 0, ctypes.byref(s), one, 1, 2) == -1 and b"flags" in err()
    assert step(0, 0, ctypes.byref(s), one, 49, 0) == -1 and b"0..48" in err()
    assert step(0, 0, ctypes.byref(s), one, -1, 0) == -1
    assert step(0, 0, None, one, 1, 0) == -1 and b"NULL" in err()
    assert step(0, 0, ctypes.byref(s), None, 1, 0) == -1 and b"NULL" in err()
    no_v = (pn.Segment * 1)(pn.Segment(256, 256, 256, None, 1000, 1.0, -1.0))           # Adam without its second moment
    assert step(0, 1, ctypes.byref(s), no_v, 1, 0) == -1 and b"NULL" in err()
    assert step(1, 1, ctypes.byref(s), no_v, 1, 0) == -1 and b"NULL" in err()
    no_g = (pn.Segment * 1)(pn.Segment(256, None, 256, None, 1000, 1.0, -1.0))
    assert step(2, 1, ctypes.byref(s), no_g, 1, 0) == -1 and b"NULL" in err()
    odd = (pn.Segment * 1)(pn.Segment(257, 256, 256, 256, 1000, 1.0, -1.0))             # not aligned to a 16-bit element
    assert step(0, 0, ctypes.byref(s), odd, 1, 0) == -1 and b"misaligned" in err()
    half = (pn.Segment * 1)(pn.Segment(256, 258, 256, 256, 1000, 1.0, -1.0))            # 2 bytes: fine for 16 bits, not for f32
    assert step(0, 2, ctypes.byref(s), half, 1, 0) == -1 and b"misaligned" in err()
    neg = (pn.Segment * 1)(pn.Segment(256, 256, 256, 256, -1, 1.0, -1.0))
    assert step(0, 0, ctypes.byref(s), neg, 1, 0) == -2 and b"numel" in err()
    # empty work is a no-op success, without a device
    assert step(0, 0, ctypes.byref(s), one, 0, 0) == 0
    assert step(0, 0, None, None, 0, 0) == 0
    empty = (pn.Segment * 2)(pn.Segment(None, None, None, None, 0, 1.0, -1.0), pn.Segment(None, None, None, None, 0, 1.0, -1.0))
    assert step(2, 1, ctypes.byref(s), empty, 2, 0) == 0
    with pytest.raises(RuntimeError, match="status -1"):
        pn.check(-1, "unit")


# ----------------------------------------------------------------------------- the page plan
def _check_plan(numels, page_elems):
    pages = paged.plan_pages(numels, page_elems)
    flat = [seg for page in pages for seg in page]
    # every element exactly once, tensors in order, each tensor's ranges in order
    nxt = {}
    last_tensor = -1
    for ti, start, count in flat:
        assert count > 0 and start % paged.PAGE_ALIGN == 0
        assert ti >= last_tensor
        last_tensor = ti
        assert start == nxt.get(ti, 0), (ti, start)
        nxt[ti] = start + count
    for ti, n in enumerate(numels):
        assert nxt.get(ti, 0) == n, (ti, n)
    for page in pages:
        assert page, "an empty page"
        assert sum(c for _, _, c in page) <= page_elems
        assert sum(-(-c // paged.PAGE_ALIGN) * paged.PAGE_ALIGN for _, _, c in page) <= page_elems   # as laid out in a slot
    return pages


def test_plan_pages():
    assert paged.plan_pages([], 64) == [] and paged.plan_pages([0, 0], 64) == []
    assert _check_plan([64], 64) == [[(0, 0, 64)]]                                       # ends exactly on the boundary
    assert _check_plan([65], 64) == [[(0, 0, 64)], [(0, 64, 1)]]                         # one element past it
    pages = _check_plan([5 * 64 + 3], 64)
    assert len(pages) == 6 and pages[-1] == [(0, 320, 3)]
    assert _check_plan([0, 8, 0, 8], 64) == [[(1, 0, 8), (3, 0, 8)]]                     # empty tensors take nothing
    pages = _check_plan([8] * 60, 2048)
    assert len(pages) == 1 and len(pages[0]) == 60                                       # many small tensors share one page
    pages = _check_plan([3, 5, 100, 1, 64, 7], 64)
    assert pages[0][:3] == [(0, 0, 3), (1, 0, 5), (2, 0, 48)] and pages[1][0] == (2, 48, 52)
    rng = np.random.default_rng(7)
    for _ in range(50):
        _check_plan([int(x) for x in rng.integers(0, 700, size=int(rng.integers(1, 12)))], int(rng.integers(1, 40)) * 8)
    for bad in (0, 4, 12, -8):
        with pytest.raises(ValueError, match="multiple of 8"):
            paged.plan_pages([10], bad)


# ----------------------------------------------------------------------------- the emulation against the reference
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_paged.json")))
CASES = MANIFEST["g14"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g14_paged.npz"))


def _ordered(b: np.ndarray) -> np.ndarray:
    """Bit patterns of sign-magnitude floats as integers in value order: the difference of two is their distance in ulps."""
    w = b.dtype.itemsize * 8
    b = b.astype(np.int64)
    sign = b >> (w - 1)
    mag = b & ((1 << (w - 1)) - 1)
    return np.where(sign == 1, -mag, mag)


def _ulps(got, want):
    return np.abs(_ordered(emul.bits(got)) - _ordered(np.asarray(want)))


def _hp(case) -> dict:
    """The case's hyperparameters with the class defaults filled in (test_signatures_and_defaults_are_the_references)."""
    two = case["opt"] in emul.TWO_MOMENTS
    hp = dict(betas=(0.9, 0.999) if two else (0.9, 0.99), eps=1e-8, weight_decay=1e-2 if case["opt"] == "adamw" else 0)
    hp.update(case["kwargs"])
    return hp


def test_fixture_covers_what_it_should():
    assert os.path.getsize(os.path.join(GOLD, "g14_paged.npz")) <= os.path.getsize(os.path.join(GOLD, "g10_optim.npz"))
    seen = {(c["opt"], c["dtype"], c["shapes"][0][0] % 32 != 0, c["kwargs"].get("weight_decay", None) not in (0, None))
            for c in CASES if len(c["shapes"]) == 1 and not c["start_step"]}
    for opt in emul.RULES:
        for dt in ("f16", "bf16", "f32"):
            assert {(opt, dt, False, True), (opt, dt, True, True)} & seen and {(opt, dt, False, False), (opt, dt, True, False)} & seen
            assert {t for o, d, t, _ in seen if (o, d) == (opt, dt)} == {False, True}
    assert any(len(c["shapes"]) == 3 and any(c["none_steps"]) for c in CASES)
    assert any(c["opt"] == "adam" and c["start_step"] >= 1000 for c in CASES)
    assert all(c["steps"] == 4 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"c{c['id']}-{c['opt']}-{c['dtype']}-{c['shapes'][0][0]}")
def test_emulation_reproduces_the_reference_step_by_step(case, gold):
    """Each step starts from the reference's parameter and moments after the previous step.  16-bit: exact outside the last
    numel % 32 elements (torch's scalar tail loop rounds alpha * x twice), at most 1 ulp inside them.  f32: the moments exact, the
    parameter at most 1 ulp away on at most 1 % of a tensor's elements per step (torch's vectorised sqrt is 1 ulp low on some inputs)."""
    ci, opt, dt = case["id"], case["opt"], case["dtype"]
    two = opt in emul.TWO_MOMENTS
    for j, shape in enumerate(case["shapes"]):
        n = int(np.prod(shape))
        tail = n % 32
        p = paged_cases.initial_param(case, j).reshape(-1)
        if case["start_step"]:
            m, v = (t.reshape(-1) for t in paged_cases.initial_moments(case, j))
            assert np.array_equal(emul.bits(m), gold[f"c{ci}_p{j}_s0_exp_avg"].reshape(-1))
            assert np.array_equal(emul.bits(v), gold[f"c{ci}_p{j}_s0_exp_avg_sq"].reshape(-1))
        else:
            m, v = torch.zeros_like(p), (torch.zeros_like(p) if two else None)
        count = case["start_step"]
        for s in range(1, case["steps"] + 1):
            key = f"c{ci}_p{j}_s{s}"
            if s in case["none_steps"][j]:
                assert np.array_equal(emul.bits(p), gold[key]), f"{key}: a parameter without a gradient moved"
                assert (f"{key}_exp_avg" in gold.files) == (count > 0)
                continue
            count += 1
            np_, nm, nv = emul.step_tensors(opt, _hp(case), count, p, paged_cases.gradient(case, j, s).reshape(-1), m, v)
            got = dict(p=np_, exp_avg=nm, exp_avg_sq=nv)
            for name, suffix in (("p", ""), ("exp_avg", "_exp_avg"), ("exp_avg_sq", "_exp_avg_sq")):
                if got[name] is None:
                    continue
                want = gold[key + suffix]
                d = _ulps(got[name], want)
                tag = f"{key} {name}"
                if dt != "f32":
                    assert not d[:n - tail].any(), f"{tag}: {np.count_nonzero(d[:n - tail])} differ outside the tail"
                    assert d.max(initial=0) <= 1, f"{tag}: {d.max()} ulps in the tail"
                elif name != "p":
                    assert not d.any(), f"{tag}: {np.count_nonzero(d)} of {n} differ"
                else:
                    assert d.max(initial=0) <= 1, f"{tag}: {d.max()} ulps"
                    assert np.count_nonzero(d) <= 0.01 * n, f"{tag}: {np.count_nonzero(d)} of {n} differ"
            # the next step starts from the reference's state
            p = emul.from_bits(gold[key], dt)
            m = emul.from_bits(gold[key + "_exp_avg"], dt)
            v = emul.from_bits(gold[key + "_exp_avg_sq"], dt) if two else None
