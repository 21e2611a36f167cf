"""CPU-side checks of the 2 ... 16 row decode path (libmbnb_batch.so, functional.matmul_4bit_grouped / matmul_4bit_lora_grouped), without
a GPU: the library loads and exports exactly its header, the other seven libraries export none of it, every argument error and every
condition of the fused launches answers before anything is dereferenced (fake aligned pointers), the tables are cut into calls of at
most 16 members, the two functions hand 2 ... 16 rows to this library and nothing else (a recording stand-in; tensors that only claim to
live on the GPU), a declined chunk falls back, and the adapter cases of tests/batch_cases.py can tell an adapter from none in every row."""
import contextlib
import os
import re
import subprocess
import threading

import pytest
import torch

from mps_bitsandbytes_amd import _batch_native as bn
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _lora_native as ln
from mps_bitsandbytes_amd import _native, _optim_native, _paged_native, _sparse_native, _train_native
from mps_bitsandbytes_amd import functional as F
from tests import batch_cases as bc
from tests import lora_cases as lc
from tests.lora_bound import lora_bound, lora_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_batch.h")
SOURCE = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "batch_kernels.hip")
NAMES = ["mbnb_batch_abi_version", "mbnb_batch_gemm4", "mbnb_batch_gemm4_lora", "mbnb_batch_last_error", "mbnb_batch_last_launch"]
P = 256            # any non-NULL, 16-byte aligned value: every check must answer before a dereference


def _header():
    return open(HEADER).read()


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the library and its exports
def test_library_loads_and_exports_exactly_its_header():
    lib = bn.lib()
    assert bn.available()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text))) == sorted(bn.EXPORTED_SYMBOLS) == NAMES
    assert _exported(bn.LIB_PATH) == NAMES
    assert lib.mbnb_batch_abi_version() == bn.ABI_VERSION == 1
    assert re.search(r"#define MBNB_BATCH_ABI_VERSION 1\b", _header())
    assert re.search(r"\bMBNB_BATCH_NOT_APPLICABLE = 65536\b", _header()) and bn.NOT_APPLICABLE == 65536
    assert re.search(r"#define MBNB_BATCH_MIN_M 2\b", _header()) and re.search(r"#define MBNB_BATCH_MAX_M 16\b", _header())
    assert (bn.MIN_M, bn.MAX_M) == (2, 16)
    assert '#include "mbnb_group.h"' in _header() and '#include "mbnb_lora.h"' in _header()
    assert "struct mbnb_group_member *members" in _header() and "struct mbnb_lora_adapter *adapters" in _header()
    assert bn.MAX_MEMBERS == gn.MAX_MEMBERS == 16 and bn.Member is gn.Member and bn.Adapter is ln.Adapter


def test_the_other_seven_libraries_export_none_of_it_and_it_links_none_of_them():
    others = (_native, _optim_native, _train_native, _sparse_native, _paged_native, gn, ln)
    assert len({b.LIB_PATH for b in others}) == 7
    for binding in others:
        assert not [n for n in _exported(binding.LIB_PATH) if n.startswith("mbnb_batch")], binding.LIB_PATH
    assert _exported(gn.LIB_PATH) == sorted(gn.EXPORTED_SYMBOLS) and _exported(ln.LIB_PATH) == sorted(ln.EXPORTED_SYMBOLS)
    needed = subprocess.run(["readelf", "-d", bn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed


def test_source_reports_through_its_own_export():
    """The kernel-name closure tests scan every csrc file for these two calls; this library reports through mbnb_batch_last_launch()."""
    shared = os.path.join(os.path.dirname(SOURCE), "skinny4_group.h")
    for path in (SOURCE, shared, HEADER, bn.__file__):
        src = open(path).read()
        assert "set_kernel_name" not in src and "set_kernel_variant" not in src, path
    src = open(SOURCE).read()
    assert "mbnb_batch_last_launch" in src
    for path in (SOURCE, shared):
        assert "atomic" not in open(path).read().replace("no atomics", ""), path
    makefile = open(os.path.join(os.path.dirname(SOURCE), "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*batch$", makefile, flags=re.M) and re.search(r"^batch_SRCS\s*:=\s*batch_kernels\.hip$", makefile, flags=re.M)
    assert "batch" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1)


def test_a_missing_library_and_another_abi_version_fail_loudly(monkeypatch, tmp_path):
    bn.lib()
    monkeypatch.setattr(bn, "_lib", None)
    monkeypatch.setattr(bn, "_load_error", None)
    monkeypatch.setattr(bn, "ABI_VERSION", 999)
    with pytest.raises(RuntimeError, match="ABI version mismatch"):
        bn.lib()
    assert bn.available() is False
    monkeypatch.setattr(bn, "_load_error", None)
    monkeypatch.setattr(bn, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no Python fallback"):
        bn.lib()


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


def _call(members, adapters=None, M=8, K=4096, qt=0, dt=1, bs=64, flags=0, x=P, n=None):
    """mbnb_batch_gemm4 (adapters None) or mbnb_batch_gemm4_lora on fake pointers."""
    n = len(members) if n is None else n
    table = _members(*members) if members else None
    if adapters is None:
        return bn.lib().mbnb_batch_gemm4(x, M, K, qt, dt, bs, table, n, flags, None)
    return bn.lib().mbnb_batch_gemm4_lora(x, M, K, qt, dt, bs, table, _adapters(*adapters) if adapters else None, n, flags, None)


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


# (id, keywords, members, code, text): each for both entry points; K = 192 / M = 17 alone would be a NOT_APPLICABLE, and comes later
ARGUMENT_ERRORS = [
    ("n=17", dict(n=17), [_plain()], -1, b"0..16"),
    ("n=-1", dict(n=-1), [_plain()], -1, b"0..16"),
    ("NULL members", dict(n=1), [], -1, b"NULL member table"),
    ("NULL x", dict(x=None), [_plain()], -1, b"NULL x"),
    ("dtype", dict(dt=3), [_plain()], -1, b"dtype"),
    ("quant type", dict(qt=2), [_plain()], -1, b"quant type"),
    ("flags", dict(flags=1), [_plain()], -1, b"flags"),
    ("NULL packed", dict(), [_plain(packed=None)], -1, b"NULL packed or out"),
    ("NULL out", dict(), [gn.Member(P, P, None, None, None, None, 8, 0, 0)], -1, b"NULL packed or out"),
    ("no absmax", dict(), [gn.Member(P, None, None, None, None, P, 8, 0, 0)], -1, b"no absmax"),
    ("codes without absmax2", dict(), [gn.Member(P, None, P, None, None, P, 8, 256, 0)], -1, b"absmax2"),
    ("N=0", dict(K=192), [_plain(), _plain(N=0)], -2, b"member 1 has N = 0"),
    ("K=0", dict(K=0), [_plain()], -2, b"K = 0"),
    ("blocksize=0", dict(bs=0, M=17), [_plain()], -2, b"blocksize = 0"),
    ("M=0", dict(M=0, K=192), [_plain()], -2, b"M = 0"),
    ("M=-3", dict(M=-3, dt=2), [_plain()], -2, b"M = -3"),
]
LORA_ARGUMENT_ERRORS = [
    ("NULL adapters", dict(n=1, K=192), [_plain()], [], -1, b"NULL adapter table"),
    ("R<0", dict(K=192), [_plain(), _plain()], [_rank(), _rank(R=-1)], -2, b"member 1 has R = -1"),
    ("NULL a", dict(M=17), [_plain()], [_rank(a=None)], -1, b"NULL a or b"),
    ("NULL b", dict(M=1), [_plain()], [_rank(b=None)], -1, b"NULL a or b"),
]


@pytest.mark.parametrize("lora", [False, True], ids=["gemm4", "gemm4_lora"])
@pytest.mark.parametrize("name, kw, members, code, text", ARGUMENT_ERRORS, ids=[c[0] for c in ARGUMENT_ERRORS])
def test_argument_errors_are_negative_with_a_text(name, kw, members, code, text, lora):
    def body():
        lib = bn.lib()
        assert _call(members, [_rank()] * len(members) if lora else None, **kw) == code
        assert text in lib.mbnb_batch_last_error(), lib.mbnb_batch_last_error()
        assert lib.mbnb_batch_last_error().startswith(b"mbnb_batch_gemm4_lora: " if lora else b"mbnb_batch_gemm4: ")
        assert lib.mbnb_batch_last_launch() == b""

    _in_a_fresh_thread(body)


@pytest.mark.parametrize("name, kw, members, adapters, code, text", LORA_ARGUMENT_ERRORS, ids=[c[0] for c in LORA_ARGUMENT_ERRORS])
def test_adapter_argument_errors_come_before_every_not_applicable(name, kw, members, adapters, code, text):
    def body():
        lib = bn.lib()
        assert _call(members, adapters, **kw) == code
        assert text in lib.mbnb_batch_last_error(), lib.mbnb_batch_last_error()
        assert lib.mbnb_batch_last_error().startswith(b"mbnb_batch_gemm4_lora: ")
        assert lib.mbnb_batch_last_launch() == b""

    _in_a_fresh_thread(body)


def test_an_empty_group_is_a_no_op_and_check_raises_with_the_text():
    assert _call([], n=0) == 0 and _call([], [], n=0) == 0
    assert _call([_plain()], n=0, M=0, K=-5, dt=9, bs=-1) == 0 and _call([_plain()], [_rank()], n=0, K=192, dt=2, bs=48) == 0
    with pytest.raises(RuntimeError, match=r"^mps_bitsandbytes_amd\.batch\.unit failed \(status -1\): "):
        bn.check(-1, "unit")


# (id, keywords, members, text): the conditions of mbnb_batch_gemm4, for both entry points
NOT_APPLICABLE = [
    ("M=1", dict(M=1), [_plain()], b"2 <= M <= 16 is needed, got M = 1"),
    ("M=17", dict(M=17), [_plain()], b"2 <= M <= 16 is needed, got M = 17"),
    ("f32", dict(dt=2), [_plain()], b"16-bit"),
    ("blocksize=16", dict(bs=16), [_plain()], b"power of two >= 32"),
    ("blocksize=96", dict(bs=96, K=4224), [_plain()], b"power of two >= 32"),
    ("K=192", dict(K=192), [_plain()], b"K % 128"),
    ("K=64", dict(K=64), [_plain()], b"128 <= K"),
    ("K=256 blocksize 512", dict(K=256, bs=512), [_plain()], b"K % blocksize"),
    ("K=16512", dict(K=16512), [_plain()], b"K <= 16384"),
    ("x+8", dict(x=P + 8), [_plain()], b"x is not 16-byte aligned"),
    ("packed+8", dict(), [_plain(), _plain(packed=P + 8)], b"member 1's packed weight is not 16-byte aligned"),
    ("2^40 bytes", dict(K=16384), [_plain(N=1 << 27)], b"2^40"),
    ("2^31 workgroups", dict(K=128), [_plain(N=(1 << 33) - 16)] * 4 + [_plain(N=80)], b"2^31 workgroups"),      # 4 (2^29 - 1) + 5
    ("nested with plain", dict(), [_nested(), _plain()], b"plain and double-quantised"),
    ("plain with nested", dict(), [_plain(), _plain(), _nested()], b"member 2 differs"),
    ("nested blocksize2=0", dict(), [_nested(), _nested(bs2=0)], b"member 1's blocksize2 is 0"),
]
LORA_NOT_APPLICABLE = [
    ("R=257", dict(), [_plain(), _plain()], [_rank(), _rank(R=257)], b"member 1 has R = 257, 1 <= R <= 256"),
    ("a+8", dict(), [_plain()], [_rank(a=P + 8)], b"member 0's a is not 16-byte aligned"),
    ("b+1", dict(), [_plain()], [_rank(b=P + 1)], b"member 0's b is not 2-byte aligned"),
    ("t+2", dict(), [_plain()], [_rank(t=P + 2)], b"member 0's t is NULL or not 4-byte aligned"),
    ("NULL t", dict(), [_plain()], [_rank(t=None)], b"member 0's t is NULL or not 4-byte aligned"),
    ("scaling inf", dict(), [_plain()], [_rank(scaling=float("inf"))], b"scaling is not finite"),
    ("scaling nan", dict(), [_plain(), _plain()], [NONE, _rank(scaling=float("nan"))], b"member 1's scaling is not finite"),
    ("no adapter at all", dict(), [_plain(), _plain()], [NONE, ln.Adapter(P + 1, P + 1, None, 0, float("nan"))], b"no member has an adapter"),
]


def _declines(members, adapters, kw, text):
    def body():
        lib = bn.lib()
        assert lib.mbnb_batch_last_launch() == b"" and lib.mbnb_batch_last_error() == b""
        rc = _call(members, adapters, **kw)
        assert rc == bn.NOT_APPLICABLE > 0, (rc, lib.mbnb_batch_last_error())
        assert text in lib.mbnb_batch_last_error(), lib.mbnb_batch_last_error()
        assert lib.mbnb_batch_last_launch() == b"" and bn.last_launch() == "" and text.decode() in bn.last_error()

    _in_a_fresh_thread(body)


@pytest.mark.parametrize("lora", [False, True], ids=["gemm4", "gemm4_lora"])
@pytest.mark.parametrize("name, kw, members, text", NOT_APPLICABLE, ids=[c[0] for c in NOT_APPLICABLE])
def test_every_condition_of_the_fused_launch_answers_not_applicable(name, kw, members, text, lora):
    """Each of these would otherwise launch; the answer comes first, and the launch report is still empty."""
    _declines(members, [_rank()] * len(members) if lora else None, kw, text)


@pytest.mark.parametrize("name, kw, members, adapters, text", LORA_NOT_APPLICABLE, ids=[c[0] for c in LORA_NOT_APPLICABLE])
def test_every_condition_of_the_adapters_answers_not_applicable(name, kw, members, adapters, text):
    _declines(members, adapters, kw, text)


# ----------------------------------------------------------------------------- chunking into calls of at most 16
class _StubLib:
    """Stands in for libmbnb_batch.so: records what each call receives (no device involved)."""

    def __init__(self, decline=()):
        self.calls, self.decline = [], set(decline)

    def _record(self, x, M, K, qt, dt, bs, members, adapters, n, flags, stream):
        self.calls.append(dict(x=x, M=M, K=K, qt=qt, dt=dt, bs=bs, n=n, flags=flags, stream=stream, lora=adapters is not None,
                               members=[{f: getattr(members[i], f) for f, _ in gn.Member._fields_} for i in range(n)],
                               adapters=None if adapters is None else
                               [{f: getattr(adapters[i], f) for f, _ in ln.Adapter._fields_} for i in range(n)]))
        return bn.NOT_APPLICABLE if len(self.calls) - 1 in self.decline else 0

    def mbnb_batch_gemm4(self, x, M, K, qt, dt, bs, members, n, flags, stream):
        return self._record(x, M, K, qt, dt, bs, members, None, n, flags, stream)

    def mbnb_batch_gemm4_lora(self, x, M, K, qt, dt, bs, members, adapters, n, flags, stream):
        return self._record(x, M, K, qt, dt, bs, members, adapters, n, flags, stream)

    def mbnb_batch_last_error(self):
        return b"stub"


def _rows(count):
    return [(4096 + 16 * i, 8192 + 4 * i, 0, 0, 0 if i % 2 else 12288 + 2 * i, 16384 + 2 * i, 1 + i % 5, 0, 0) for i in range(count)]


def _ranks(count):
    return [ln.NO_ADAPTER if i % 3 == 0 else (20480 + 16 * i, 24576 + 2 * i, 28672 + 4 * i, 1 + i % 5, 0.5 * i) for i in range(count)]


@pytest.mark.parametrize("count, want", [(1, [1]), (16, [16]), (17, [16, 1]), (33, [16, 16, 1]), (0, [])])
def test_tables_are_cut_into_calls_of_at_most_sixteen(monkeypatch, count, want):
    stub = _StubLib()
    monkeypatch.setattr(bn, "_lib", stub)
    bn.reset_launch_log()
    rows, ranks = _rows(count), _ranks(count)
    assert bn.gemm4(P, 5, 2176, "fp4", torch.bfloat16, 32, rows, 77) == [True] * len(want)
    assert bn.gemm4_lora(P, 9, 2176, "nf4", torch.float16, 128, rows, ranks, 78) == [True] * len(want)
    plain, lora = stub.calls[:len(want)], stub.calls[len(want):]
    assert [c["n"] for c in plain] == [c["n"] for c in lora] == want
    assert bn.launch_log == [(n, 5, 2176, torch.bfloat16) for n in want] + \
        [(n, sum(r[3] for r in ranks[16 * c:16 * c + 16]), 9, 2176, torch.float16) for c, n in enumerate(want)]
    for calls in (plain, lora):
        seen = [m for c in calls for m in c["members"]]
        assert len(seen) == count
        for row, m in zip(rows, seen):       # every member once, in order, field for field (a 0 address reads back as None)
            assert tuple(m[f] or 0 for f, _ in gn.Member._fields_) == row
    assert all(c["adapters"] is None for c in plain)
    for rank, a in zip(ranks, [a for c in lora for a in c["adapters"]]):
        assert tuple(a[f] or 0 for f, _ in ln.Adapter._fields_) == rank
    for c in plain:
        assert (c["x"], c["M"], c["K"], c["qt"], c["dt"], c["bs"], c["flags"], c["stream"]) == (P, 5, 2176, _native.FP4, _native.BF16, 32, 0, 77)
    for c in lora:
        assert (c["x"], c["M"], c["K"], c["qt"], c["dt"], c["bs"], c["flags"], c["stream"]) == (P, 9, 2176, _native.NF4, _native.F16, 128, 0, 78)
    bn.reset_launch_log()
    assert bn.launch_log == []


def test_a_declined_chunk_is_reported_and_not_logged_and_a_failed_call_raises(monkeypatch):
    stub = _StubLib(decline=[0, 3])
    monkeypatch.setattr(bn, "_lib", stub)
    bn.reset_launch_log()
    assert bn.gemm4(P, 2, 1024, "nf4", torch.float16, 64, _rows(17), None) == [False, True]
    assert bn.gemm4_lora(P, 2, 1024, "nf4", torch.float16, 64, _rows(17), _ranks(17), None) == [True, False]
    assert bn.launch_log == [(1, 2, 1024, torch.float16), (16, sum(r[3] for r in _ranks(16)), 2, 1024, torch.float16)]
    bn.reset_launch_log()
    with pytest.raises(ValueError, match="2 members but 1 adapters"):
        bn.gemm4_lora(P, 2, 1024, "nf4", torch.float16, 64, _rows(2), _ranks(1), None)

    class Failing(_StubLib):
        def _record(self, *a):
            return -1

    monkeypatch.setattr(bn, "_lib", Failing())
    with pytest.raises(RuntimeError, match=r"batch\.gemm4 failed \(status -1\): stub"):
        bn.gemm4(P, 2, 1024, "nf4", torch.float16, 64, _rows(1), None)
    with pytest.raises(RuntimeError, match=r"batch\.gemm4_lora failed \(status -1\): stub"):
        bn.gemm4_lora(P, 2, 1024, "nf4", torch.float16, 64, _rows(1), _ranks(2)[1:], None)
    assert bn.launch_log == []


# ----------------------------------------------------------------------------- the two functions, on tensors that claim to be on the GPU
class _OnGpu(torch.Tensor):
    """A CPU tensor whose .device says cuda: functional's plan for a fused call can be followed up to the library call (a stand-in)."""
    device = property(lambda self: torch.device("cuda"))


class _TorchOnCpu:
    """``torch`` as functional.py sees it here: empty() allocates on the CPU whatever device is asked for."""

    def empty(self, *args, **kwargs):
        return torch.empty(*args, **dict(kwargs, device="cpu")).as_subclass(_OnGpu)

    def __getattr__(self, name):
        return getattr(torch, name)


class _GroupStub:
    def __init__(self):
        self.calls = []

    def mbnb_group_gemv4(self, *a):
        self.calls.append("group")
        return 0

    def mbnb_lora_gemv4(self, *a):
        self.calls.append("lora")
        return 0


@pytest.fixture
def routed(monkeypatch):
    """(batch stub, group / lora stub, the matmul_4bit stand-in's calls) with functional's device plumbing neutralised."""
    batch, single, by_member = _StubLib(), _GroupStub(), []
    batch.real = bn.lib()
    monkeypatch.setattr(bn, "_lib", batch)
    monkeypatch.setattr(gn, "_lib", single)
    monkeypatch.setattr(ln, "_lib", single)
    monkeypatch.setattr(F, "torch", _TorchOnCpu())
    monkeypatch.setattr(F, "on_device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(F, "stream_ptr", lambda device: 77)

    def matmul_4bit(A, B, state, bias=None, compute_dtype=None):
        by_member.append(int(state.shape[0]))
        return torch.full((*A.shape[:-1], int(state.shape[0])), float(len(by_member)))

    monkeypatch.setattr(F, "matmul_4bit", matmul_4bit)
    bn.reset_launch_log()
    gn.reset_launch_log()
    ln.reset_launch_log()
    yield batch, single, by_member
    bn.reset_launch_log()
    gn.reset_launch_log()
    ln.reset_launch_log()


def _gpu(t):
    return t.as_subclass(_OnGpu)


def _fake_group(Ns, K, T=torch.bfloat16, bs=64):
    weights = []
    for N in Ns:
        st = F.QuantState(absmax=_gpu(torch.ones(N * K // bs)), shape=torch.Size([N, K]), blocksize=bs, quant_type="nf4", dtype=T)
        weights.append((_gpu(torch.zeros(N * K // 2, dtype=torch.uint8)), st))
    return weights


def _fake_adapters(Ns, K, Rs, T=torch.bfloat16):
    return [None if R is None else (_gpu(torch.zeros(R, K, dtype=T)), _gpu(torch.zeros(N, R, dtype=T)), 0.5) for N, R in zip(Ns, Rs)]


@pytest.mark.parametrize("shape, M", [((2, 256), 2), ((16, 256), 16), ((2, 3, 256), 6), ((1, 1, 1, 256), 1), ((256,), 1), ((17, 256), 17),
                                      ((3, 6, 256), 18), ((0, 256), 0)])
def test_only_two_to_sixteen_rows_reach_the_batch_library(routed, shape, M):
    batch, single, by_member = routed
    K, Ns, Rs = 256, (5, 3, 20), (4, None, 9)
    A = _gpu(torch.zeros(shape, dtype=torch.bfloat16))
    weights, adapters = _fake_group(Ns, K), _fake_adapters(Ns, K, Rs)
    bias = [None, _gpu(torch.zeros(3, dtype=torch.bfloat16)), None]
    ys = F.matmul_4bit_grouped(A, weights, bias)
    zs = F.matmul_4bit_lora_grouped(A, weights, adapters, bias)
    assert len(ys) == len(zs) == 3
    if 2 <= M <= 16:
        assert single.calls == [] and by_member == [] and [c["lora"] for c in batch.calls] == [False, True]
        assert bn.launch_log == [(3, M, K, torch.bfloat16), (3, 13, M, K, torch.bfloat16)] and gn.launch_log == ln.launch_log == []
        plain, lora = batch.calls
        for c in batch.calls:
            assert (c["M"], c["K"], c["bs"], c["n"], c["qt"], c["dt"], c["stream"], c["flags"]) == (M, K, 64, 3, _native.NF4, _native.BF16, 77, 0)
            # the outputs: dense [M, N_g] blocks of ONE allocation, in member order; each a view shaped like A
            outs = [m["out"] for m in c["members"]]
            assert [b - a for a, b in zip(outs, outs[1:])] == [2 * M * N for N in Ns[:-1]]
            assert [m["N"] for m in c["members"]] == list(Ns) and [bool(m["bias"]) for m in c["members"]] == [False, True, False]
        for group, call in ((ys, plain), (zs, lora)):
            for y, N, m in zip(group, Ns, call["members"]):
                assert y.shape == shape[:-1] + (N,) and y.dtype == torch.bfloat16 and y.is_contiguous() and y.data_ptr() == m["out"]
        # the workspaces: f32 [M, R_g] blocks of ONE allocation, none for the member without an adapter
        t = [a["t"] for a in lora["adapters"]]
        assert [a["R"] for a in lora["adapters"]] == [4, 0, 9] and t[1] is None and t[2] - t[0] == 4 * M * 4
        assert lora["adapters"][0]["a"] == adapters[0][0].data_ptr() and lora["adapters"][2]["b"] == adapters[2][1].data_ptr()
    elif M == 1:
        assert batch.calls == [] and bn.launch_log == [] and by_member == [] and single.calls == ["group", "lora"]
        assert gn.launch_log == [(3, K, torch.bfloat16)] and ln.launch_log == [(3, 13, K, torch.bfloat16)]
    else:
        assert batch.calls == [] and single.calls == [] and bn.launch_log == gn.launch_log == ln.launch_log == []
        assert by_member == [5, 3, 20] * 2      # member by member, and the composed form's matmul_4bit per member


@pytest.mark.parametrize("why", ["gradient", "f32 weights", "mixed formats", "other compute_dtype", "f32 adapter"])
def test_what_went_member_by_member_still_does(routed, monkeypatch, why):
    """A gradient, mixed formats, another compute_dtype and adapters of another dtype never reach the library; f32 weights do, as
    they reach libmbnb_group.so with one row, and the library (the real one here: it answers before it dereferences) declines."""
    batch, single, by_member = routed
    K, Ns = 256, (5, 3)
    A = _gpu(torch.zeros(4, K, dtype=torch.bfloat16))
    weights, adapters, cd = _fake_group(Ns, K), _fake_adapters(Ns, K, (4, 2)), None
    if why == "gradient":
        A.requires_grad_(True)
    elif why == "f32 weights":
        weights, A = _fake_group(Ns, K, torch.float32), _gpu(torch.zeros(4, K))
        adapters = _fake_adapters(Ns, K, (4, 2), torch.float32)
        monkeypatch.setattr(bn, "_lib", batch.real)
    elif why == "mixed formats":
        weights[1][1].quant_type = "fp4"
    elif why == "other compute_dtype":
        cd = torch.float32
    else:
        adapters[1] = (adapters[1][0].float(), adapters[1][1].float(), 0.5)
    F.matmul_4bit_lora_grouped(A, weights, adapters, compute_dtype=cd)
    if why != "f32 adapter":
        F.matmul_4bit_grouped(A, weights, compute_dtype=cd)
    assert batch.calls == [] and single.calls == [] and bn.launch_log == []
    assert by_member == [5, 3] * (1 if why == "f32 adapter" else 2)
    if why == "f32 weights":
        assert "16-bit" in bn.last_error()


def test_a_declined_chunk_falls_back_and_the_other_chunk_stays_fused(routed, monkeypatch):
    batch, single, by_member = routed
    batch.decline = {0, 3}      # the first chunk of the grouped call, the second of the adapter call
    K, Ns = 256, (3,) * 17
    A = _gpu(torch.zeros(2, K, dtype=torch.bfloat16))
    weights = _fake_group(Ns, K)
    ys = F.matmul_4bit_grouped(A, weights)
    assert [c["n"] for c in batch.calls] == [16, 1] and bn.launch_log == [(1, 2, K, torch.bfloat16)]
    assert by_member == [3] * 16 and [float(y[0, 0]) for y in ys[:16]] == [float(i + 1) for i in range(16)]      # the stand-in's values
    assert ys[16].data_ptr() == batch.calls[1]["members"][0]["out"]
    del by_member[:]
    composed_members = []
    real = F._lora_composed

    def composed(A, B, state, bias, adapter, compute_dtype):
        composed_members.append(int(state.shape[0]))
        return real(A, B, state, bias, None, compute_dtype)      # the stand-in's base alone: no torch GEMM on these tensors

    monkeypatch.setattr(F, "_lora_composed", composed)
    zs = F.matmul_4bit_lora_grouped(A, weights, _fake_adapters(Ns, K, (2,) * 17))
    assert [c["n"] for c in batch.calls[2:]] == [16, 1] and bn.launch_log[1:] == [(16, 32, 2, K, torch.bfloat16)]
    assert composed_members == [3] and by_member == [3] and len(zs) == 17
    assert single.calls == []


# ----------------------------------------------------------------------------- the bounds, and what the adapter cases can tell
def test_the_fused_bound_lies_inside_the_composed_bound():
    """tests/test_gpu_lora.py checks its 2, 3 and 6 row cases against the composed bound; they now run fused.  u (|r| + g S) <=
    u (1 + 4u) (|r| + 3 S) because g = (K + R + 6) 2^-23 < 3 for every K and R the library takes."""
    assert (16384 + 256 + 6) * 2.0 ** -23 < 3
    g = torch.Generator().manual_seed(0)
    for T in (torch.float16, torch.bfloat16):
        for K, R in ((128, 1), (1024, 8), (16384, 256)):
            r = torch.randn(64, 64, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 4, (64, 64), generator=g)
            S = r.abs() * (1 + 10.0 ** torch.randint(-3, 6, (64, 64), generator=g))
            r[0, :8], S[0, :4] = 0.0, 0.0
            assert bool((lora_bound(r, S, R, K, T, "fused") <= lora_bound(r, S, R, K, T, "composed")).all())


_ADAPTER_CASES: dict = {}      # (Ns, K, qt, nested, bs, bias, Rs, dt) -> its row counts
for _args in bc.ARGS:
    _ADAPTER_CASES.setdefault(_args[:8], []).append(_args[8])


@pytest.mark.parametrize("Ns, K, qt, nested, bs, bias, Rs, dt", list(_ADAPTER_CASES),
                         ids=[f"N{'x'.join(map(str, c[0][:3]))}-K{c[1]}-{c[2]}-bs{c[4]}-{c[7]}" for c in _ADAPTER_CASES])
def test_reference_without_its_adapter_term_violates_the_fused_bound_in_every_row(Ns, K, qt, nested, bs, bias, Rs, dt):
    """What a kernel that dropped the epilogue would return -- the base term rounded to T -- lies outside the bound in at least one
    element of EVERY row, at every row count of the case, so each adapter case of tests/test_gpu_batch.py can fail for that reason
    in each row."""
    T = bc.DT[dt]
    for rows in _ADAPTER_CASES[(Ns, K, qt, nested, bs, bias, Rs, dt)]:
        X = bc.x(K, dt, rows)
        telling = torch.zeros(rows, dtype=torch.bool)
        for i, (N, R) in enumerate(zip(Ns, Rs)):
            if R is None:
                continue
            Wd = lc.member(N, K, dt, qt, nested, bs, seed=i)[3]
            b = lc.bias(N, dt, i) if i in bias else None
            ad = lc.adapter(N, K, R, dt, i)
            r, S, R_ = lora_reference(X, Wd, b, ad)
            assert R_ == R and ad[2] == 4.0 / R and r.shape == (rows, N)
            base = lora_reference(X, Wd, b, None)[0].to(T).double()
            telling |= ((base - r).abs() > lora_bound(r, S, R, K, T, "fused")).any(dim=1)
        assert bool(telling.all()), f"M = {rows}: rows {(~telling).nonzero().flatten().tolist()} cannot tell a dropped adapter"
