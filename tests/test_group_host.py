"""CPU-side checks of the grouped M = 1 GEMV (libmbnb_group.so, functional.matmul_4bit_grouped, nn.Linear4bitGroup), without a GPU:
the library loads and exports exactly its header, libmbnb_hip.so exports none of it, every argument error and every condition of
the fused launch answers before anything is dereferenced (fake aligned pointers), the member struct has the header's layout in
both of the binding's mirrors, the table is cut into calls of at most 16 members, and the layer keeps its members' own state."""
import ctypes
import os
import re
import subprocess
import threading

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_group.h")
SOURCE = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "group_kernels.hip")
NAMES = ["mbnb_group_abi_version", "mbnb_group_gemv4", "mbnb_group_last_error", "mbnb_group_last_launch"]
P = 256            # any non-NULL, 16-byte aligned value: every check must answer before a dereference


def _header():
    return open(HEADER).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the library and its exports
def test_library_loads_and_exports_exactly_its_header():
    lib = gn.lib()
    assert gn.available()
    assert _declared() == sorted(gn.EXPORTED_SYMBOLS) == NAMES
    assert _exported(gn.LIB_PATH) == NAMES
    assert lib.mbnb_group_abi_version() == gn.ABI_VERSION == 1
    assert re.search(r"#define MBNB_GROUP_ABI_VERSION 1\b", _header())
    assert re.search(r"#define MBNB_GROUP_MAX_MEMBERS 16\b", _header()) and gn.MAX_MEMBERS == 16
    assert re.search(r"\bMBNB_GROUP_NOT_APPLICABLE = 65536\b", _header()) and gn.NOT_APPLICABLE == 65536


def test_main_library_exports_none_of_it():
    exported = _exported(_native.LIB_PATH)
    assert exported == sorted(_native.EXPORTED_SYMBOLS)
    assert not [n for n in exported if "group" in n]


def test_source_reports_through_its_own_export():
    """The kernel-name closure tests scan every csrc file for these two calls; this library reports through mbnb_group_last_launch()."""
    src = open(SOURCE).read()
    assert "set_kernel_name" not in src and "set_kernel_variant" not in src
    assert "mbnb_group_last_launch" in src


def test_names_are_public():
    assert bnb.matmul_4bit_grouped is F.matmul_4bit_grouped
    assert bnb.Linear4bitGroup is bnb.nn.Linear4bitGroup
    assert "matmul_4bit_grouped" in bnb.__all__ and "Linear4bitGroup" in bnb.__all__ and "Linear4bitGroup" in bnb.nn.__all__
    assert len(bnb.__all__) == len(set(bnb.__all__))


def test_load_path_is_the_shared_one(monkeypatch, tmp_path):
    """What tests/test_native_abi.py holds for the other five bindings: a missing library and another ABI version fail loudly."""
    gn.lib()
    monkeypatch.setattr(gn, "_lib", None)
    monkeypatch.setattr(gn, "_load_error", None)
    monkeypatch.setattr(gn, "ABI_VERSION", 999)
    with pytest.raises(RuntimeError, match="ABI version mismatch"):
        gn.lib()
    assert gn.available() is False
    monkeypatch.setattr(gn, "_load_error", None)
    monkeypatch.setattr(gn, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no Python fallback"):
        gn.lib()


# ----------------------------------------------------------------------------- the member struct
def test_member_struct_has_the_headers_layout():
    defines = dict(re.findall(r"#define MBNB_GROUP_MEMBER_(\w+) (\d+)\b", _header()))
    size = int(defines.pop("BYTES"))
    fields = [f for f, _ in gn.Member._fields_]
    offsets = {f: int(defines.pop("OFF_" + f.upper())) for f in fields}
    assert not defines and len(fields) == 9
    for name in fields:      # each constant is static_asserted against offsetof in the header itself
        assert re.search(rf"offsetof\(struct mbnb_group_member, {name}\) == MBNB_GROUP_MEMBER_OFF_{name.upper()}\)", _header()), name
    assert "sizeof(struct mbnb_group_member) == MBNB_GROUP_MEMBER_BYTES" in _header()
    assert ctypes.sizeof(gn.Member) == gn.MEMBER_DTYPE.itemsize == size == 64
    assert list(gn.MEMBER_DTYPE.names) == fields
    for f in fields:
        assert getattr(gn.Member, f).offset == gn.MEMBER_DTYPE.fields[f][1] == offsets[f], f
        assert getattr(gn.Member, f).size == gn.MEMBER_DTYPE.fields[f][0].itemsize, f


# ----------------------------------------------------------------------------- argument paths (nothing is dereferenced)
def _table(*members):
    return (gn.Member * len(members))(*members)


def _plain(N=8, packed=P):
    return gn.Member(packed, P, None, None, None, P, N, 0, 0)


def _nested(N=8, bs2=256, codes=P):
    return gn.Member(P, None, codes, P, None, P, N, bs2, 0)


def _call(table, n, K=4096, qt=0, dt=1, bs=64, flags=0, x=P):
    return gn.lib().mbnb_group_gemv4(x, K, qt, dt, bs, table, n, flags, None)


def test_argument_errors_are_negative_with_a_text():
    lib = gn.lib()
    one = _table(_plain())
    assert _call(one, 17) == -1 and b"0..16" in lib.mbnb_group_last_error()
    assert _call(one, -1) == -1
    assert _call(None, 1) == -1 and b"NULL member table" in lib.mbnb_group_last_error()
    assert _call(one, 1, x=None) == -1 and b"NULL x" in lib.mbnb_group_last_error()
    assert _call(one, 1, dt=3) == -1 and b"dtype" in lib.mbnb_group_last_error()
    assert _call(one, 1, qt=2) == -1 and b"quant type" in lib.mbnb_group_last_error()
    assert _call(one, 1, flags=1) == -1 and b"flags" in lib.mbnb_group_last_error()
    assert _call(_table(_plain(packed=None)), 1) == -1 and b"NULL packed or out" in lib.mbnb_group_last_error()
    assert _call(_table(gn.Member(P, P, None, None, None, None, 8, 0, 0)), 1) == -1 and b"NULL packed or out" in lib.mbnb_group_last_error()
    assert _call(_table(gn.Member(P, None, None, None, None, P, 8, 0, 0)), 1) == -1 and b"no absmax" in lib.mbnb_group_last_error()
    assert _call(_table(gn.Member(P, None, P, None, None, P, 8, 256, 0)), 1) == -1 and b"absmax2" in lib.mbnb_group_last_error()
    assert _call(_table(_plain(), _plain(N=0)), 2) == -2 and b"member 1 has N = 0" in lib.mbnb_group_last_error()
    assert _call(one, 1, K=0) == -2
    # an empty group is a no-op success, whatever else is passed
    assert _call(None, 0) == 0
    assert _call(one, 0, K=512, dt=2, bs=128) == 0
    with pytest.raises(RuntimeError, match=r"^mps_bitsandbytes_amd\.group\.unit failed \(status -1\): "):
        gn.check(-1, "unit")


NOT_APPLICABLE = [
    ("K=512", dict(K=512), [_plain()], b"1024 <= K"),
    ("K=1056", dict(K=1056), [_plain()], b"K % 64"),
    ("K=16448", dict(K=16448), [_plain()], b"K <= 16384"),
    ("blocksize=128", dict(bs=128), [_plain()], b"blocksize 64"),
    ("f32", dict(dt=2), [_plain()], b"16-bit"),
    ("packed+8", dict(), [_plain(), _plain(packed=P + 8)], b"member 1's packed weight is not 16-byte aligned"),
    ("x+8", dict(x=P + 8), [_plain()], b"x is not 16-byte aligned"),
    ("nested K/64 % 4", dict(K=1088), [_nested()], b"(K / 64) % 4"),
    ("nested bs2", dict(), [_nested(bs2=96)], b"power of two"),
    ("nested codes+2", dict(), [_nested(codes=P + 2)], b"4-byte aligned"),
    ("nested with plain", dict(), [_nested(), _plain()], b"plain and double-quantised"),
    ("plain with nested", dict(), [_plain(), _plain(), _nested()], b"member 2 differs"),
    ("2^40 bytes", dict(K=16384), [_plain(N=1 << 27)], b"2^40"),
    ("2^31 workgroups", dict(K=1024), [_plain(N=(1 << 31) - 4)] * 4 + [_plain(N=16)], b"2^31 workgroups"),
]


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


@pytest.mark.parametrize("name, kw, members, text", NOT_APPLICABLE, ids=[c[0] for c in NOT_APPLICABLE])
def test_every_condition_of_the_fused_launch_answers_not_applicable(name, kw, members, text):
    """Each of these would otherwise launch; the answer comes first, and the launch report is still empty."""
    def body():
        lib = gn.lib()
        assert lib.mbnb_group_last_launch() == b"" and lib.mbnb_group_last_error() == b""
        rc = _call(_table(*members), len(members), **kw)
        assert rc == gn.NOT_APPLICABLE > 0, (rc, lib.mbnb_group_last_error())
        assert text in lib.mbnb_group_last_error(), lib.mbnb_group_last_error()
        assert lib.mbnb_group_last_launch() == b"" and gn.last_launch() == ""

    _in_a_fresh_thread(body)


# ----------------------------------------------------------------------------- chunking into calls of at most 16
class _StubLib:
    """Stands in for libmbnb_group.so: records what each mbnb_group_gemv4 call receives (no device involved)."""

    def __init__(self, decline=()):
        self.calls, self.decline = [], set(decline)

    def mbnb_group_gemv4(self, x, K, qt, dt, bs, table, n, flags, stream):
        self.calls.append(dict(x=x, K=K, qt=qt, dt=dt, bs=bs, n=n, flags=flags, stream=stream,
                               table=[{f: getattr(table[i], f) for f, _ in gn.Member._fields_} for i in range(n)]))
        return gn.NOT_APPLICABLE if len(self.calls) - 1 in self.decline else 0


def _rows(count):
    return [(4096 + 16 * i, 8192 + 4 * i, 0, 0, 0 if i % 2 else 12288 + 2 * i, 16384 + 2 * i, 1 + i % 5, 0, 0) for i in range(count)]


@pytest.mark.parametrize("count, want", [(1, [1]), (16, [16]), (17, [16, 1]), (33, [16, 16, 1]), (0, [])])
def test_table_is_cut_into_calls_of_at_most_sixteen(monkeypatch, count, want):
    stub = _StubLib()
    monkeypatch.setattr(gn, "_lib", stub)
    gn.reset_launch_log()
    rows = _rows(count)
    done = gn.gemv4(P, 2112, "fp4", torch.bfloat16, 64, rows, 77)
    assert done == [True] * len(want)
    assert [c["n"] for c in stub.calls] == want
    assert gn.launch_log == [(n, 2112, torch.bfloat16) for n in want]
    seen = [m for c in stub.calls for m in c["table"]]
    assert len(seen) == count
    for row, m in zip(rows, seen):         # every member once, in order, field for field (a 0 address reads back as None)
        assert tuple(m[f] or 0 for f, _ in gn.Member._fields_) == row
    for c in stub.calls:
        assert (c["x"], c["K"], c["qt"], c["dt"], c["bs"], c["flags"], c["stream"]) == (P, 2112, _native.FP4, _native.BF16, 64, 0, 77)
    gn.reset_launch_log()
    assert gn.launch_log == []


def test_a_declined_chunk_is_reported_and_not_logged(monkeypatch):
    stub = _StubLib(decline=[0])
    monkeypatch.setattr(gn, "_lib", stub)
    gn.reset_launch_log()
    assert gn.gemv4(P, 1024, "nf4", torch.float16, 64, _rows(17), None) == [False, True]
    assert gn.launch_log == [(1, 1024, torch.float16)]
    gn.reset_launch_log()


def test_a_failed_call_raises(monkeypatch):
    class Failing(_StubLib):
        def mbnb_group_gemv4(self, *a):
            return -1

        def mbnb_group_last_error(self):
            return b"stub"

    monkeypatch.setattr(gn, "_lib", Failing())
    gn.reset_launch_log()
    with pytest.raises(RuntimeError, match=r"group\.gemv4 failed \(status -1\): stub"):
        gn.gemv4(P, 1024, "nf4", torch.float16, 64, _rows(1), None)
    assert gn.launch_log == []


def test_grouped_call_without_members_and_with_a_bias_count_mismatch():
    assert F.matmul_4bit_grouped(torch.zeros(1, 64), []) == ()
    st = F.QuantState(absmax=torch.ones(4), shape=torch.Size([4, 64]))
    with pytest.raises(ValueError, match="1 weights but 2 biases"):
        F.matmul_4bit_grouped(torch.zeros(1, 64), [(torch.zeros(128, dtype=torch.uint8), st)], [None, None])
    # CPU tensors: the member-by-member path raises what matmul_4bit raises
    with pytest.raises(ValueError, match="requires tensor on a 'cuda'"):
        F.matmul_4bit_grouped(torch.zeros(1, 64), [(torch.zeros(128, dtype=torch.uint8), st)])


# ----------------------------------------------------------------------------- the layer, on CPU tensors
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


def test_layer_group_keeps_each_members_own_state_dict_keys():
    group = bnb.Linear4bitGroup([_layer(8), _layer(4, bias=False, seed=1), _layer(12, nested=True, seed=2)])
    assert isinstance(group.layers, torch.nn.ModuleList) and len(group.layers) == 3 and group.in_features == 128
    sd = group.state_dict()
    assert sorted(sd) == sorted(["layers.0.weight", "layers.0.bias", "layers.0.weight_quant_state", "layers.1.weight",
                                 "layers.1.weight_quant_state", "layers.2.weight", "layers.2.bias", "layers.2.weight_quant_state"])
    for i, layer in enumerate(group.layers):
        alone = layer.state_dict()
        assert sorted(alone) == sorted(k[len(f"layers.{i}."):] for k in sd if k.startswith(f"layers.{i}."))
    assert "out_features=(8, 4, 12)" in repr(group)


def test_layer_group_round_trips_a_members_quant_state():
    src = bnb.Linear4bitGroup([_layer(8), _layer(12, nested=True, seed=2)])
    dst = bnb.Linear4bitGroup([bnb.Linear4bit(128, 8, compute_dtype=torch.bfloat16), bnb.Linear4bit(128, 12, compute_dtype=torch.bfloat16)])
    assert dst.layers[1].weight_quant_state is None
    result = dst.load_state_dict(src.state_dict())
    assert not result.missing_keys and not result.unexpected_keys
    for a, b in zip(src.layers, dst.layers):
        sa, sb = a.weight_quant_state, b.weight_quant_state
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
        assert torch.equal(sa.absmax, sb.absmax) and sa.absmax.dtype == sb.absmax.dtype
        assert (tuple(sa.shape), sa.blocksize, sa.quant_type, sa.dtype) == (tuple(sb.shape), sb.blocksize, sb.quant_type, sb.dtype)
        assert (sa.state2 is None) == (sb.state2 is None)
        if sa.state2 is not None:
            assert torch.equal(sa.state2.absmax, sb.state2.absmax) and sa.state2.blocksize == sb.state2.blocksize == 256


def test_layer_group_refuses_what_is_no_group():
    with pytest.raises(ValueError, match="layer 1 has in_features=64, layer 0 has in_features=128"):
        bnb.Linear4bitGroup([_layer(8), _layer(8, in_features=64)])
    with pytest.raises(ValueError, match="at least one"):
        bnb.Linear4bitGroup([])
    with pytest.raises(TypeError, match="layer 0 is a Linear"):
        bnb.Linear4bitGroup([torch.nn.Linear(8, 8)])
    group = bnb.Linear4bitGroup([bnb.Linear4bit(128, 8), _layer(8)])
    with pytest.raises(RuntimeError, match="Weight not quantized"):
        group(torch.zeros(1, 128))
