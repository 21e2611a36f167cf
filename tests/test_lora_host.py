"""CPU-side checks of the LoRA decode path (libmbnb_lora.so, functional.matmul_4bit_lora_grouped, nn.Linear4bitLoRA /
Linear4bitLoRAGroup), without a GPU: the library loads and exports exactly its header, libmbnb_hip.so and libmbnb_group.so export none of
it, every argument error and every condition of the fused launches answers before anything is dereferenced (fake aligned pointers),
the adapter struct has the header's layout in both of the binding's mirrors, the tables are cut into calls of at most 16 members, the
modules keep their members' own state, and the fused cases of tests/lora_cases.py can tell an adapter from none."""
import ctypes
import os
import re
import subprocess
import threading

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _lora_native as ln
from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F
from tests import lora_cases as lc
from tests.lora_bound import lora_bound, lora_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_lora.h")
SOURCE = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "lora_kernels.hip")
NAMES = ["mbnb_lora_abi_version", "mbnb_lora_gemv4", "mbnb_lora_last_error", "mbnb_lora_last_launch"]
P = 256            # any non-NULL, 16-byte aligned value: every check must answer before a dereference


def _header():
    return open(HEADER).read()


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the library and its exports
def test_library_loads_and_exports_exactly_its_header():
    lib = ln.lib()
    assert ln.available()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text))) == sorted(ln.EXPORTED_SYMBOLS) == NAMES
    assert _exported(ln.LIB_PATH) == NAMES
    assert lib.mbnb_lora_abi_version() == ln.ABI_VERSION == 1
    assert re.search(r"#define MBNB_LORA_ABI_VERSION 1\b", _header())
    assert re.search(r"#define MBNB_LORA_MAX_R 256\b", _header()) and ln.MAX_R == 256
    assert re.search(r"\bMBNB_LORA_NOT_APPLICABLE = 65536\b", _header()) and ln.NOT_APPLICABLE == 65536
    assert '#include "mbnb_group.h"' in _header() and "struct mbnb_group_member *members" in _header()
    assert ln.MAX_MEMBERS == gn.MAX_MEMBERS == 16 and ln.Member is gn.Member


def test_the_other_libraries_export_none_of_it():
    assert not [n for n in _exported(_native.LIB_PATH) if "lora" in n]
    assert _exported(gn.LIB_PATH) == sorted(gn.EXPORTED_SYMBOLS)
    assert not [n for n in _exported(gn.LIB_PATH) if "lora" in n]


def test_source_reports_through_its_own_export():
    """The kernel-name closure tests scan every csrc file for these two calls; this library reports through mbnb_lora_last_launch()."""
    for path in (SOURCE, os.path.join(os.path.dirname(SOURCE), "gemv4_group.h")):
        src = open(path).read()
        assert "set_kernel_name" not in src and "set_kernel_variant" not in src, path
    assert "mbnb_lora_last_launch" in open(SOURCE).read()


def test_names_are_public():
    assert bnb.matmul_4bit_lora_grouped is F.matmul_4bit_lora_grouped
    assert bnb.Linear4bitLoRA is bnb.nn.Linear4bitLoRA and bnb.Linear4bitLoRAGroup is bnb.nn.Linear4bitLoRAGroup
    for name in ("matmul_4bit_lora_grouped", "Linear4bitLoRA", "Linear4bitLoRAGroup"):
        assert name in bnb.__all__
    assert "Linear4bitLoRA" in bnb.nn.__all__ and "Linear4bitLoRAGroup" in bnb.nn.__all__
    assert len(bnb.__all__) == len(set(bnb.__all__))


def test_a_missing_library_and_another_abi_version_fail_loudly(monkeypatch, tmp_path):
    ln.lib()
    monkeypatch.setattr(ln, "_lib", None)
    monkeypatch.setattr(ln, "_load_error", None)
    monkeypatch.setattr(ln, "ABI_VERSION", 999)
    with pytest.raises(RuntimeError, match="ABI version mismatch"):
        ln.lib()
    assert ln.available() is False
    monkeypatch.setattr(ln, "_load_error", None)
    monkeypatch.setattr(ln, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no Python fallback"):
        ln.lib()


# ----------------------------------------------------------------------------- the adapter struct
def test_adapter_struct_has_the_headers_layout():
    defines = dict(re.findall(r"#define MBNB_LORA_ADAPTER_(\w+) (\d+)\b", _header()))
    size = int(defines.pop("BYTES"))
    fields = [f for f, _ in ln.Adapter._fields_]
    offsets = {f: int(defines.pop("OFF_" + f.upper())) for f in fields}
    assert not defines and fields == ["a", "b", "t", "R", "scaling"]
    for name in fields:      # each constant is static_asserted against offsetof in the header itself
        assert re.search(rf"offsetof\(struct mbnb_lora_adapter, {name}\) == MBNB_LORA_ADAPTER_OFF_{name.upper()}\)", _header()), name
    assert "sizeof(struct mbnb_lora_adapter) == MBNB_LORA_ADAPTER_BYTES" in _header()
    assert ctypes.sizeof(ln.Adapter) == ln.ADAPTER_DTYPE.itemsize == size == 32
    assert list(ln.ADAPTER_DTYPE.names) == fields
    for f in fields:
        assert getattr(ln.Adapter, f).offset == ln.ADAPTER_DTYPE.fields[f][1] == offsets[f], f
        assert getattr(ln.Adapter, f).size == ln.ADAPTER_DTYPE.fields[f][0].itemsize, f
    assert len(ln.NO_ADAPTER) == len(fields) and ln.NO_ADAPTER[3] == 0


# ----------------------------------------------------------------------------- argument paths (nothing is dereferenced)
def _members(*members):
    return (gn.Member * len(members))(*members)


def _adapters(*adapters):
    return (ln.Adapter * len(adapters))(*adapters)


def _plain(N=8, packed=P):
    return gn.Member(packed, P, None, None, None, P, N, 0, 0)


def _nested(N=8, bs2=256, codes=P):
    return gn.Member(P, None, codes, P, None, P, N, bs2, 0)


def _rank(R=16, a=P, b=P, t=P, scaling=0.25):
    return ln.Adapter(a, b, t, R, scaling)


NONE = ln.Adapter(None, None, None, 0, 0.0)


def _call(members, adapters, K=4096, qt=0, dt=1, bs=64, flags=0, x=P, n=None):
    n = len(members) if n is None else n
    return ln.lib().mbnb_lora_gemv4(x, K, qt, dt, bs, _members(*members) if members else None, _adapters(*adapters) if adapters else None,
                                    n, flags, None)


def _in_a_fresh_thread(fn):
    """Run fn on a new thread (the error text and the launch report are thread-local: a new thread starts with both empty, whatever
    ran in this process before) and re-raise what it raised."""
    caught = []

    def run():
        try:
            fn()
        except BaseException as e:      # noqa: BLE001  (handed to the test's thread)
            caught.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if caught:
        raise caught[0]


ARGUMENT_ERRORS = [
    # those of mbnb_group_gemv4
    ("n=17", dict(n=17), [_plain()], [_rank()], -1, b"0..16"),
    ("n=-1", dict(n=-1), [_plain()], [_rank()], -1, b"0..16"),
    ("NULL members", dict(n=1), [], [_rank()], -1, b"NULL member table"),
    ("NULL x", dict(x=None), [_plain()], [_rank()], -1, b"NULL x"),
    ("dtype", dict(dt=3), [_plain()], [_rank()], -1, b"dtype"),
    ("quant type", dict(qt=2), [_plain()], [_rank()], -1, b"quant type"),
    ("flags", dict(flags=1), [_plain()], [_rank()], -1, b"flags"),
    ("NULL packed", dict(), [_plain(packed=None)], [_rank()], -1, b"NULL packed or out"),
    ("NULL out", dict(), [gn.Member(P, P, None, None, None, None, 8, 0, 0)], [_rank()], -1, b"NULL packed or out"),
    ("no absmax", dict(), [gn.Member(P, None, None, None, None, P, 8, 0, 0)], [_rank()], -1, b"no absmax"),
    ("codes without absmax2", dict(), [gn.Member(P, None, P, None, None, P, 8, 256, 0)], [_rank()], -1, b"absmax2"),
    ("N=0", dict(), [_plain(), _plain(N=0)], [_rank(), _rank()], -2, b"member 1 has N = 0"),
    ("K=0", dict(K=0), [_plain()], [_rank()], -2, b"K = 0"),
    # the adapter table's; they come before every NOT_APPLICABLE (K = 512 alone would be one)
    ("NULL adapters", dict(n=1, K=512), [_plain()], [], -1, b"NULL adapter table"),
    ("R<0", dict(K=512), [_plain(), _plain()], [_rank(), _rank(R=-1)], -2, b"member 1 has R = -1"),
    ("NULL a", dict(K=512), [_plain()], [_rank(a=None)], -1, b"NULL a or b"),
    ("NULL b", dict(K=512), [_plain()], [_rank(b=None)], -1, b"NULL a or b"),
]


@pytest.mark.parametrize("name, kw, members, adapters, code, text", ARGUMENT_ERRORS, ids=[c[0] for c in ARGUMENT_ERRORS])
def test_argument_errors_are_negative_with_a_text(name, kw, members, adapters, code, text):
    def body():
        lib = ln.lib()
        assert _call(members, adapters, **kw) == code
        assert text in lib.mbnb_lora_last_error(), lib.mbnb_lora_last_error()
        assert lib.mbnb_lora_last_error().startswith(b"mbnb_lora_gemv4: ")
        assert lib.mbnb_lora_last_launch() == b""

    _in_a_fresh_thread(body)


def test_an_empty_group_is_a_no_op_and_check_raises_with_the_text():
    assert _call([], [], n=0) == 0
    assert _call([_plain()], [_rank()], n=0, K=512, dt=2, bs=128) == 0
    with pytest.raises(RuntimeError, match=r"^mps_bitsandbytes_amd\.lora\.unit failed \(status -1\): "):
        ln.check(-1, "unit")


NOT_APPLICABLE = [
    # all conditions of mbnb_group_gemv4
    ("K=512", dict(K=512), [_plain()], [_rank()], b"1024 <= K"),
    ("K=1056", dict(K=1056), [_plain()], [_rank()], b"K % 64"),
    ("K=16448", dict(K=16448), [_plain()], [_rank()], b"K <= 16384"),
    ("blocksize=128", dict(bs=128), [_plain()], [_rank()], b"blocksize 64"),
    ("f32", dict(dt=2), [_plain()], [_rank()], b"16-bit"),
    ("packed+8", dict(), [_plain(), _plain(packed=P + 8)], [_rank(), _rank()], b"member 1's packed weight is not 16-byte aligned"),
    ("x+8", dict(x=P + 8), [_plain()], [_rank()], b"x is not 16-byte aligned"),
    ("nested K/64 % 4", dict(K=1088), [_nested()], [_rank()], b"(K / 64) % 4"),
    ("nested bs2", dict(), [_nested(bs2=96)], [_rank()], b"power of two"),
    ("nested codes+2", dict(), [_nested(codes=P + 2)], [_rank()], b"4-byte aligned"),
    ("nested with plain", dict(), [_nested(), _plain()], [_rank(), _rank()], b"plain and double-quantised"),
    ("plain with nested", dict(), [_plain(), _plain(), _nested()], [_rank(), NONE, _rank()], b"member 2 differs"),
    ("2^40 bytes", dict(K=16384), [_plain(N=1 << 27)], [_rank()], b"2^40"),
    ("2^31 workgroups", dict(K=1024), [_plain(N=(1 << 31) - 4)] * 4 + [_plain(N=16)], [_rank()] * 5, b"2^31 workgroups"),
    # the adapters'
    ("R=257", dict(), [_plain(), _plain()], [_rank(), _rank(R=257)], b"member 1 has R = 257, 1 <= R <= 256"),
    ("a+8", dict(), [_plain()], [_rank(a=P + 8)], b"member 0's a is not 16-byte aligned"),
    ("b+1", dict(), [_plain()], [_rank(b=P + 1)], b"member 0's b is not 2-byte aligned"),
    ("t+2", dict(), [_plain()], [_rank(t=P + 2)], b"member 0's t is NULL or not 4-byte aligned"),
    ("NULL t", dict(), [_plain()], [_rank(t=None)], b"member 0's t is NULL or not 4-byte aligned"),
    ("scaling inf", dict(), [_plain()], [_rank(scaling=float("inf"))], b"scaling is not finite"),
    ("scaling nan", dict(), [_plain(), _plain()], [NONE, _rank(scaling=float("nan"))], b"member 1's scaling is not finite"),
    ("no adapter at all", dict(), [_plain(), _plain()], [NONE, ln.Adapter(P + 1, P + 1, None, 0, float("nan"))], b"no member has an adapter"),
]


@pytest.mark.parametrize("name, kw, members, adapters, text", NOT_APPLICABLE, ids=[c[0] for c in NOT_APPLICABLE])
def test_every_condition_of_the_fused_launches_answers_not_applicable(name, kw, members, adapters, text):
    """Each of these would otherwise launch; the answer comes first, and the launch report is still empty."""
    def body():
        lib = ln.lib()
        assert lib.mbnb_lora_last_launch() == b"" and lib.mbnb_lora_last_error() == b""
        rc = _call(members, adapters, **kw)
        assert rc == ln.NOT_APPLICABLE > 0, (rc, lib.mbnb_lora_last_error())
        assert text in lib.mbnb_lora_last_error(), lib.mbnb_lora_last_error()
        assert lib.mbnb_lora_last_launch() == b"" and ln.last_launch() == ""

    _in_a_fresh_thread(body)


# ----------------------------------------------------------------------------- chunking into calls of at most 16
class _StubLib:
    """Stands in for libmbnb_lora.so: records what each mbnb_lora_gemv4 call receives (no device involved)."""

    def __init__(self, decline=()):
        self.calls, self.decline = [], set(decline)

    def mbnb_lora_gemv4(self, x, K, qt, dt, bs, members, adapters, n, flags, stream):
        self.calls.append(dict(x=x, K=K, qt=qt, dt=dt, bs=bs, n=n, flags=flags, stream=stream,
                               members=[{f: getattr(members[i], f) for f, _ in gn.Member._fields_} for i in range(n)],
                               adapters=[{f: getattr(adapters[i], f) for f, _ in ln.Adapter._fields_} for i in range(n)]))
        return ln.NOT_APPLICABLE if len(self.calls) - 1 in self.decline else 0


def _rows(count):
    return [(4096 + 16 * i, 8192 + 4 * i, 0, 0, 0 if i % 2 else 12288 + 2 * i, 16384 + 2 * i, 1 + i % 5, 0, 0) for i in range(count)]


def _ranks(count):
    return [ln.NO_ADAPTER if i % 3 == 0 else (20480 + 16 * i, 24576 + 2 * i, 28672 + 4 * i, 1 + i % 5, 0.5 * i) for i in range(count)]


@pytest.mark.parametrize("count, want", [(1, [1]), (16, [16]), (17, [16, 1]), (33, [16, 16, 1]), (0, [])])
def test_tables_are_cut_into_calls_of_at_most_sixteen(monkeypatch, count, want):
    stub = _StubLib()
    monkeypatch.setattr(ln, "_lib", stub)
    ln.reset_launch_log()
    rows, ranks = _rows(count), _ranks(count)
    done = ln.gemv4(P, 2112, "fp4", torch.bfloat16, 64, rows, ranks, 77)
    assert done == [True] * len(want)
    assert [c["n"] for c in stub.calls] == want
    assert ln.launch_log == [(n, sum(r[3] for r in ranks[16 * c:16 * c + 16]), 2112, torch.bfloat16) for c, n in enumerate(want)]
    seen_m = [m for c in stub.calls for m in c["members"]]
    seen_a = [a for c in stub.calls for a in c["adapters"]]
    assert len(seen_m) == len(seen_a) == count
    for row, m in zip(rows, seen_m):       # every member once, in order, field for field (a 0 address reads back as None)
        assert tuple(m[f] or 0 for f, _ in gn.Member._fields_) == row
    for rank, a in zip(ranks, seen_a):     # and its adapter with it
        assert tuple(a[f] or 0 for f, _ in ln.Adapter._fields_) == rank
    for c in stub.calls:
        assert (c["x"], c["K"], c["qt"], c["dt"], c["bs"], c["flags"], c["stream"]) == (P, 2112, _native.FP4, _native.BF16, 64, 0, 77)
    ln.reset_launch_log()
    assert ln.launch_log == []


def test_a_declined_chunk_is_reported_and_not_logged_and_a_failed_call_raises(monkeypatch):
    stub = _StubLib(decline=[0])
    monkeypatch.setattr(ln, "_lib", stub)
    ln.reset_launch_log()
    assert ln.gemv4(P, 1024, "nf4", torch.float16, 64, _rows(17), _ranks(17), None) == [False, True]
    assert ln.launch_log == [(1, 2, 1024, torch.float16)]
    ln.reset_launch_log()
    with pytest.raises(ValueError, match="2 members but 1 adapters"):
        ln.gemv4(P, 1024, "nf4", torch.float16, 64, _rows(2), _ranks(1), None)

    class Failing(_StubLib):
        def mbnb_lora_gemv4(self, *a):
            return -1

        def mbnb_lora_last_error(self):
            return b"stub"

    monkeypatch.setattr(ln, "_lib", Failing())
    with pytest.raises(RuntimeError, match=r"lora\.gemv4 failed \(status -1\): stub"):
        ln.gemv4(P, 1024, "nf4", torch.float16, 64, _rows(1), _ranks(2)[1:], None)
    assert ln.launch_log == []


# ----------------------------------------------------------------------------- the function, on CPU tensors
def test_all_none_adapters_reach_matmul_4bit_grouped(monkeypatch):
    seen = []

    def stand_in(A, weights, biases=None, compute_dtype=None):
        seen.append((A, weights, biases, compute_dtype))
        return ("grouped",)

    monkeypatch.setattr(F, "matmul_4bit_grouped", stand_in)
    st = F.QuantState(absmax=torch.ones(4), shape=torch.Size([4, 64]))
    A, w, b = torch.zeros(1, 64), [(torch.zeros(128, dtype=torch.uint8), st)] * 2, [None, torch.zeros(4)]
    assert F.matmul_4bit_lora_grouped(A, w, [None, None], b, torch.float16) == ("grouped",)
    assert len(seen) == 1 and seen[0][0] is A and seen[0][1] == w and seen[0][2] == b and seen[0][3] is torch.float16
    assert F.matmul_4bit_lora_grouped(A, [], []) == ("grouped",) and seen[1][1] == []


def test_count_mismatches_and_cpu_tensors_raise():
    st = F.QuantState(absmax=torch.ones(4), shape=torch.Size([4, 64]))
    w = [(torch.zeros(128, dtype=torch.uint8), st)]
    ad = (torch.zeros(2, 64), torch.zeros(4, 2), 1.0)
    with pytest.raises(ValueError, match="1 weights but 2 biases"):
        F.matmul_4bit_lora_grouped(torch.zeros(1, 64), w, [ad], [None, None])
    with pytest.raises(ValueError, match="1 weights but 2 adapters"):
        F.matmul_4bit_lora_grouped(torch.zeros(1, 64), w, [ad, None])
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):      # the composed form raises what matmul_4bit raises
        F.matmul_4bit_lora_grouped(torch.zeros(1, 64), w, [ad])


# ----------------------------------------------------------------------------- the modules, on CPU tensors
def _layer(out_features, in_features=128, bias=True, nested=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    layer = bnb.Linear4bit(in_features, out_features, bias=bias, compute_dtype=torch.bfloat16)
    layer.weight.copy_(torch.randint(0, 256, layer.weight.shape, generator=g, dtype=torch.uint8))
    nblk = out_features * in_features // 64
    if nested:
        st2 = F.QuantState(absmax=torch.rand(1, generator=g) + 1, shape=torch.Size([nblk]), blocksize=256, quant_type="int8",
                           dtype=torch.float32)
        absmax = torch.randint(-127, 128, (nblk,), generator=g, dtype=torch.int8)
    else:
        st2, absmax = None, torch.rand(nblk, generator=g) + 0.5
    layer.weight_quant_state = F.QuantState(absmax=absmax, shape=torch.Size([out_features, in_features]), blocksize=64,
                                            quant_type="nf4", dtype=torch.bfloat16, state2=st2)
    return layer


def test_lora_layer_has_pefts_init_and_the_bases_own_keys():
    base = _layer(8)
    layer = bnb.Linear4bitLoRA(base, r=4, lora_alpha=16)
    assert layer.base is base and layer.scaling == 4.0 and (layer.in_features, layer.out_features, layer.r) == (128, 8, 4)
    assert layer.lora_A.shape == (4, 128) and layer.lora_B.shape == (8, 4)
    assert layer.lora_A.dtype == layer.lora_B.dtype == torch.bfloat16 and layer.lora_A.requires_grad and layer.lora_B.requires_grad
    assert not bool(layer.lora_B.any())
    bound = 1.0 / 128 ** 0.5              # kaiming_uniform_(a = sqrt(5)) over fan_in 128: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert 0.5 * bound < float(layer.lora_A.detach().abs().max()) <= bound * (1 + 2.0 ** -8)
    assert bnb.Linear4bitLoRA(base, r=4).scaling == 0.25
    assert sorted(layer.state_dict()) == sorted(["lora_A", "lora_B"] + ["base." + k for k in base.state_dict()])
    assert sorted(base.state_dict()) == ["bias", "weight", "weight_quant_state"]
    assert "r=4, lora_alpha=16" in repr(layer)
    with pytest.raises(TypeError, match="base is a Linear"):
        bnb.Linear4bitLoRA(torch.nn.Linear(8, 8), r=4)
    with pytest.raises(ValueError, match="positive integer"):
        bnb.Linear4bitLoRA(base, r=0)
    with pytest.raises(RuntimeError, match="Weight not quantized"):
        bnb.Linear4bitLoRA(bnb.Linear4bit(128, 8), r=2)(torch.zeros(1, 128))


def test_lora_group_keeps_each_members_keys_and_round_trips():
    src = bnb.Linear4bitLoRAGroup([bnb.Linear4bitLoRA(_layer(8), r=4), bnb.Linear4bitLoRA(_layer(12, bias=False, nested=True, seed=2), r=2)])
    assert isinstance(src.layers, torch.nn.ModuleList) and len(src.layers) == 2 and src.in_features == 128
    with torch.no_grad():
        src.layers[0].lora_B.copy_(torch.arange(32).reshape(8, 4))
    sd = src.state_dict()
    assert sorted(sd) == sorted(["layers.0.lora_A", "layers.0.lora_B", "layers.0.base.weight", "layers.0.base.bias",
                                 "layers.0.base.weight_quant_state", "layers.1.lora_A", "layers.1.lora_B", "layers.1.base.weight",
                                 "layers.1.base.weight_quant_state"])
    for i, layer in enumerate(src.layers):
        assert sorted(layer.state_dict()) == sorted(k[len(f"layers.{i}."):] for k in sd if k.startswith(f"layers.{i}."))
    assert "out_features=(8, 12)" in repr(src)
    dst = bnb.Linear4bitLoRAGroup([bnb.Linear4bitLoRA(bnb.Linear4bit(128, 8, compute_dtype=torch.bfloat16), r=4),
                                   bnb.Linear4bitLoRA(bnb.Linear4bit(128, 12, bias=False, compute_dtype=torch.bfloat16), r=2)])
    assert dst.layers[1].base.weight_quant_state is None
    result = dst.load_state_dict(sd)
    assert not result.missing_keys and not result.unexpected_keys
    for a, b in zip(src.layers, dst.layers):
        assert torch.equal(a.lora_A, b.lora_A) and torch.equal(a.lora_B, b.lora_B) and torch.equal(a.base.weight, b.base.weight)
        sa, sb = a.base.weight_quant_state, b.base.weight_quant_state
        assert torch.equal(sa.absmax, sb.absmax) and sa.absmax.dtype == sb.absmax.dtype and (sa.state2 is None) == (sb.state2 is None)
        assert (tuple(sa.shape), sa.blocksize, sa.quant_type, sa.dtype) == (tuple(sb.shape), sb.blocksize, sb.quant_type, sb.dtype)
    with pytest.raises(ValueError, match="layer 1 has in_features=64, layer 0 has in_features=128"):
        bnb.Linear4bitLoRAGroup([bnb.Linear4bitLoRA(_layer(8), r=1), bnb.Linear4bitLoRA(_layer(8, in_features=64), r=1)])
    with pytest.raises(ValueError, match="at least one"):
        bnb.Linear4bitLoRAGroup([])
    with pytest.raises(TypeError, match="layer 0 is a Linear4bit, not a Linear4bitLoRA"):
        bnb.Linear4bitLoRAGroup([_layer(8)])


# ----------------------------------------------------------------------------- the table tells an adapter from none
@pytest.mark.parametrize("Ns, K, qt, nested, bias, Rs, dt", [p[1:] for p in lc.FUSED_PARAMS], ids=[p[0] for p in lc.FUSED_PARAMS])
def test_reference_without_its_adapter_term_violates_the_fused_bound(Ns, K, qt, nested, bias, Rs, dt):
    """What a kernel that dropped the adapter would return -- the base term rounded to T -- lies outside the bound in every case, so
    each fused case of tests/test_gpu_lora.py can fail for that reason.  Per member it need not: S carries the adapter's own
    |s| (|X| . |A|^T) . |B|^T, about four times the base's |X| . |Wd|^T at scaling 4 / R, so at R = 256 and K >= 8192 the g S term of
    the bound reaches the adapter term's own size (about 4 sqrt(K / R)); there the smaller-R member of the case is the one that tells."""
    T = lc.DT[dt]
    X = lc.x(K, dt)
    assert len(Ns) == len(Rs)
    telling = adapted = 0
    for i, (N, R) in enumerate(zip(Ns, Rs)):
        if R is None:
            continue
        Wd = lc.member(N, K, dt, qt, nested, seed=i)[3]
        b = lc.bias(N, dt, i) if i in bias else None
        ad = lc.adapter(N, K, R, dt, i)
        r, S, R_ = lora_reference(X, Wd, b, ad)
        assert R_ == R and ad[2] == 4.0 / R
        base = lora_reference(X, Wd, b, None)[0].to(T).double()
        outside = (base - r).abs() > lora_bound(r, S, R, K, T, "fused")
        adapted += 1
        telling += bool(outside.any())
    print(f"{telling} of {adapted} adapted members have a row outside the bound without the adapter")
    assert telling >= 1
