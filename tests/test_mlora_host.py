"""CPU-side checks of the per-row adapter path (libmbnb_mlora.so, functional.matmul_4bit_multilora_grouped, Linear4bitMultiLoRA), without a
GPU: the library loads and exports exactly its header, the other eight libraries export none of it, every argument error and every
condition of the fused launches answers before anything is dereferenced (fake aligned pointers), the tables are cut into calls of at
most 16 members, the function hands 2 ... 16 rows to this library and nothing else and everything else to the composed form (recording
stand-ins; tensors that only claim to live on the GPU), the modules keep their keys and addresses, and every case of
tests/mlora_cases.py can tell a row's adapter from the next slot's and from none."""
import contextlib
import os
import re
import subprocess
import threading

import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _batch_native as bn
from mps_bitsandbytes_amd import _group_native as gn
from mps_bitsandbytes_amd import _lora_native as ln
from mps_bitsandbytes_amd import _mlora_native as mn
from mps_bitsandbytes_amd import _native, _optim_native, _paged_native, _sparse_native, _train_native
from mps_bitsandbytes_amd import functional as F
from tests import lora_cases as lc
from tests import mlora_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbnb_mlora.h")
SOURCE = os.path.join(ROOT, "mps_bitsandbytes_amd", "csrc", "mlora_kernels.hip")
NAMES = ["mbnb_mlora_abi_version", "mbnb_mlora_gemm4", "mbnb_mlora_last_error", "mbnb_mlora_last_launch"]
P = 256            # any non-NULL, 16-byte aligned value: every check must answer before a dereference


def _header():
    return open(HEADER).read()


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]*)$", out, flags=re.M)))


# ----------------------------------------------------------------------------- the library and its exports
def test_library_loads_and_exports_exactly_its_header():
    lib = mn.lib()
    assert mn.available()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mbnb_[a-z0-9_]+)\s*\(", text))) == sorted(mn.EXPORTED_SYMBOLS) == NAMES
    assert _exported(mn.LIB_PATH) == NAMES
    assert lib.mbnb_mlora_abi_version() == mn.ABI_VERSION == 1
    assert re.search(r"#define MBNB_MLORA_ABI_VERSION 1\b", _header())
    assert re.search(r"\bMBNB_MLORA_NOT_APPLICABLE = 65536\b", _header())
    assert mn.NOT_APPLICABLE == bn.NOT_APPLICABLE == gn.NOT_APPLICABLE == ln.NOT_APPLICABLE == 65536
    assert re.search(r"#define MBNB_MLORA_MIN_M 2\b", _header()) and re.search(r"#define MBNB_MLORA_MAX_M 16\b", _header())
    assert re.search(r"#define MBNB_MLORA_MAX_R 64\b", _header()) and (mn.MIN_M, mn.MAX_M, mn.MAX_R) == (2, 16, 64)
    assert '#include "mbnb_group.h"' in _header() and '#include "mbnb_batch.h"' not in _header() and '#include "mbnb_lora.h"' not in _header()
    assert "struct mbnb_group_member *members" in _header() and "struct mbnb_mlora_bank *banks" in _header()
    assert mn.MAX_MEMBERS == gn.MAX_MEMBERS == 16 and mn.Member is gn.Member


def test_the_other_eight_libraries_export_none_of_it_and_it_needs_none_of_them():
    others = (_native, _optim_native, _train_native, _sparse_native, _paged_native, gn, ln, bn)
    assert len({b.LIB_PATH for b in others} | {mn.LIB_PATH}) == 9
    for binding in others:
        assert not [n for n in _exported(binding.LIB_PATH) if n.startswith("mbnb_mlora")], binding.LIB_PATH
    needed = subprocess.run(["readelf", "-d", mn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmbnb_" not in needed, needed
    assert not hasattr(mn, "_REQUIRES")


def test_source_reports_through_its_own_export_and_accumulates_nothing_in_memory():
    """The kernel-name closure tests scan every csrc file for these two calls; this library reports through mbnb_mlora_last_launch()."""
    for path in (SOURCE, os.path.join(os.path.dirname(SOURCE), "skinny4_group.h"), HEADER, mn.__file__):
        src = open(path).read()
        assert "set_kernel_name" not in src and "set_kernel_variant" not in src, path
        assert "atomic" not in src.replace("no atomics", "").lower(), path
    src = open(SOURCE).read()
    assert "mbnb_mlora_last_launch" in src and '#include "host.h"' in src
    makefile = open(os.path.join(os.path.dirname(SOURCE), "Makefile")).read()
    assert re.search(r"^LIBS\s*\+=\s*mlora$", makefile, flags=re.M) and re.search(r"^mlora_SRCS\s*:=\s*mlora_kernels\.hip$", makefile, flags=re.M)
    assert "mlora" not in re.search(r"^NEEDS_HIP\s*:=(.*)$", makefile, flags=re.M).group(1)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert re.search(r"for binding in \([^)]*_mlora_native\)", entry)


def test_the_bank_struct_has_the_headers_layout_in_both_mirrors():
    offsets = {name: int(value) for name, value in re.findall(r"#define MBNB_MLORA_BANK_OFF_([A-Z]+) (\d+)", _header())}
    assert offsets == {"A": 0, "B": 8, "SCALING": 16, "T": 24, "R": 32, "S": 36}
    size = int(re.search(r"#define MBNB_MLORA_BANK_BYTES (\d+)", _header()).group(1))
    assert size == 40 == mn.BANK_DTYPE.itemsize
    import ctypes
    assert ctypes.sizeof(mn.Bank) == size
    assert [name for name, _ in mn.Bank._fields_] == list(mn.BANK_DTYPE.names) == ["a", "b", "scaling", "t", "R", "S"]
    for name, _ in mn.Bank._fields_:
        assert getattr(mn.Bank, name).offset == mn.BANK_DTYPE.fields[name][1] == offsets[name.upper()], name
    assert len(mn.NO_BANK) == len(mn.BANK_DTYPE.names) and not any(mn.NO_BANK)


def test_a_missing_library_and_another_abi_version_fail_loudly(monkeypatch, tmp_path):
    mn.lib()
    monkeypatch.setattr(mn, "_lib", None)
    monkeypatch.setattr(mn, "_load_error", None)
    monkeypatch.setattr(mn, "ABI_VERSION", 999)
    with pytest.raises(RuntimeError, match="ABI version mismatch"):
        mn.lib()
    assert mn.available() is False
    monkeypatch.setattr(mn, "_load_error", None)
    monkeypatch.setattr(mn, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no Python fallback"):
        mn.lib()


# ----------------------------------------------------------------------------- argument paths (nothing is dereferenced)
def _members(*members):
    return (gn.Member * len(members))(*members)


def _plain(N=8, packed=P):
    return gn.Member(packed, P, None, None, None, P, N, 0, 0)


def _nested(N=8, bs2=256, codes=P):
    return gn.Member(P, None, codes, P, None, P, N, bs2, 0)


def _bank(R=16, S=4, a=P, b=P, scaling=P, t=P):
    return mn.Bank(a, b, scaling, t, R, S)


NONE = mn.Bank(None, None, None, None, 0, 0)
DEFAULT = object()


def _call(members, banks=DEFAULT, M=8, K=4096, qt=0, dt=1, bs=64, flags=0, x=P, n=None, ids=P):
    """mbnb_mlora_gemm4 on fake pointers; banks DEFAULT: one bank per member, None: a NULL table."""
    n = len(members) if n is None else n
    table = _members(*members) if members else None
    if banks is DEFAULT:
        banks = [_bank()] * len(members)
    bank_table = (mn.Bank * len(banks))(*banks) if banks else None
    return mn.lib().mbnb_mlora_gemm4(x, M, K, qt, dt, bs, table, bank_table, ids, n, flags, None)


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


# (id, keywords, members, banks, code, text); K = 192, M = 17, ids + 2, R = 65 alone would be a NOT_APPLICABLE: the error comes first
ARGUMENT_ERRORS = [
    ("n=17", dict(n=17), [_plain()], DEFAULT, -1, b"0..16"),
    ("n=-1", dict(n=-1), [_plain()], DEFAULT, -1, b"0..16"),
    ("NULL members", dict(n=1), [], [_bank()], -1, b"NULL member table"),
    ("NULL x", dict(x=None), [_plain()], DEFAULT, -1, b"NULL x"),
    ("dtype", dict(dt=3), [_plain()], DEFAULT, -1, b"dtype"),
    ("quant type", dict(qt=2), [_plain()], DEFAULT, -1, b"quant type"),
    ("flags", dict(flags=1), [_plain()], DEFAULT, -1, b"flags"),
    ("NULL packed", dict(), [_plain(packed=None)], DEFAULT, -1, b"NULL packed or out"),
    ("NULL out", dict(), [gn.Member(P, P, None, None, None, None, 8, 0, 0)], DEFAULT, -1, b"NULL packed or out"),
    ("no absmax", dict(), [gn.Member(P, None, None, None, None, P, 8, 0, 0)], DEFAULT, -1, b"no absmax"),
    ("codes without absmax2", dict(), [gn.Member(P, None, P, None, None, P, 8, 256, 0)], DEFAULT, -1, b"absmax2"),
    ("N=0", dict(K=192), [_plain(), _plain(N=0)], DEFAULT, -2, b"member 1 has N = 0"),
    ("K=0", dict(K=0), [_plain()], DEFAULT, -2, b"K = 0"),
    ("blocksize=0", dict(bs=0, M=17), [_plain()], DEFAULT, -2, b"blocksize = 0"),
    ("M=0", dict(M=0, K=192), [_plain()], DEFAULT, -2, b"M = 0"),
    ("M=-3", dict(M=-3, dt=2), [_plain()], DEFAULT, -2, b"M = -3"),
    ("NULL banks", dict(n=1, K=192), [_plain()], None, -1, b"NULL bank table"),
    ("NULL ids", dict(ids=None, M=17), [_plain()], DEFAULT, -1, b"NULL ids"),
    ("R<0", dict(K=192), [_plain(), _plain()], [_bank(), _bank(R=-1)], -2, b"member 1 has R = -1"),
    ("S<0", dict(ids=P + 2), [_plain(), _plain()], [_bank(), _bank(S=-2)], -2, b"member 1 has R = 16, S = -2"),
    ("NULL a", dict(M=17), [_plain()], [_bank(a=None)], -1, b"NULL a or b"),
    ("NULL b", dict(M=1), [_plain()], [_bank(b=None, R=65)], -1, b"NULL a or b"),
]


@pytest.mark.parametrize("name, kw, members, banks, code, text", ARGUMENT_ERRORS, ids=[c[0] for c in ARGUMENT_ERRORS])
def test_argument_errors_are_negative_and_come_before_every_not_applicable(name, kw, members, banks, code, text):
    def body():
        lib = mn.lib()
        assert _call(members, banks, **kw) == code
        assert text in lib.mbnb_mlora_last_error(), lib.mbnb_mlora_last_error()
        assert lib.mbnb_mlora_last_error().startswith(b"mbnb_mlora_gemm4: ")
        assert lib.mbnb_mlora_last_launch() == b""

    _in_a_fresh_thread(body)


def test_an_empty_group_is_a_no_op_and_check_raises_with_the_text():
    assert _call([], [], n=0) == 0 and _call([], None, n=0, ids=None) == 0
    assert _call([_plain()], [_bank()], n=0, M=0, K=-5, dt=9, bs=-1) == 0
    with pytest.raises(RuntimeError, match=r"^mps_bitsandbytes_amd\.mlora\.unit failed \(status -1\): "):
        mn.check(-1, "unit")


# (id, keywords, members, banks, text)
NOT_APPLICABLE = [
    ("M=1", dict(M=1), [_plain()], DEFAULT, b"2 <= M <= 16 is needed, got M = 1"),
    ("M=17", dict(M=17), [_plain()], DEFAULT, b"2 <= M <= 16 is needed, got M = 17"),
    ("f32", dict(dt=2), [_plain()], DEFAULT, b"16-bit"),
    ("blocksize=16", dict(bs=16), [_plain()], DEFAULT, b"power of two >= 32"),
    ("blocksize=96", dict(bs=96, K=4224), [_plain()], DEFAULT, b"power of two >= 32"),
    ("K=192", dict(K=192), [_plain()], DEFAULT, b"K % 128"),
    ("K=64", dict(K=64), [_plain()], DEFAULT, b"128 <= K"),
    ("K=256 blocksize 512", dict(K=256, bs=512), [_plain()], DEFAULT, b"K % blocksize"),
    ("K=16512", dict(K=16512), [_plain()], DEFAULT, b"K <= 16384"),
    ("x+8", dict(x=P + 8), [_plain()], DEFAULT, b"x is not 16-byte aligned"),
    ("packed+8", dict(), [_plain(), _plain(packed=P + 8)], DEFAULT, b"member 1's packed weight is not 16-byte aligned"),
    ("2^40 bytes", dict(K=16384), [_plain(N=1 << 27)], DEFAULT, b"2^40"),
    ("2^31 workgroups", dict(K=128), [_plain(N=(1 << 33) - 16)] * 4 + [_plain(N=80)], DEFAULT, b"2^31 workgroups"),
    ("nested with plain", dict(), [_nested(), _plain()], DEFAULT, b"plain and double-quantised"),
    ("plain with nested", dict(), [_plain(), _plain(), _nested()], DEFAULT, b"member 2 differs"),
    ("nested blocksize2=0", dict(), [_nested(), _nested(bs2=0)], DEFAULT, b"member 1's blocksize2 is 0"),
    ("ids+2", dict(ids=P + 2), [_plain()], DEFAULT, b"ids is not 4-byte aligned"),
    ("R=65", dict(), [_plain(), _plain()], [_bank(), _bank(R=65)], b"member 1 has R = 65, 1 <= R <= 64"),
    ("S=0", dict(), [_plain()], [_bank(S=0)], b"member 0 has S = 0 slots"),
    ("a+8", dict(), [_plain()], [_bank(a=P + 8)], b"member 0's a is not 16-byte aligned"),
    ("b+1", dict(), [_plain()], [_bank(b=P + 1)], b"member 0's b is not 2-byte aligned"),
    ("scaling+2", dict(), [_plain()], [_bank(scaling=P + 2)], b"member 0's scaling is NULL or not 4-byte aligned"),
    ("NULL scaling", dict(), [_plain(), _plain()], [NONE, _bank(scaling=None)], b"member 1's scaling is NULL or not 4-byte aligned"),
    ("t+2", dict(), [_plain()], [_bank(t=P + 2)], b"member 0's t is NULL or not 4-byte aligned"),
    ("NULL t", dict(), [_plain()], [_bank(t=None)], b"member 0's t is NULL or not 4-byte aligned"),
    ("no bank at all", dict(), [_plain(), _plain()], [NONE, mn.Bank(P + 1, P + 1, None, None, 0, 7)], b"no member has a bank"),
]


@pytest.mark.parametrize("name, kw, members, banks, text", NOT_APPLICABLE, ids=[c[0] for c in NOT_APPLICABLE])
def test_every_condition_of_the_fused_launches_answers_not_applicable(name, kw, members, banks, text):
    """Each of these would otherwise launch; the answer comes first, and the launch report is still empty."""
    def body():
        lib = mn.lib()
        assert lib.mbnb_mlora_last_launch() == b"" and lib.mbnb_mlora_last_error() == b""
        rc = _call(members, banks, **kw)
        assert rc == mn.NOT_APPLICABLE > 0, (rc, lib.mbnb_mlora_last_error())
        assert text in lib.mbnb_mlora_last_error(), lib.mbnb_mlora_last_error()
        assert lib.mbnb_mlora_last_launch() == b"" and mn.last_launch() == "" and text.decode() in mn.last_error()

    _in_a_fresh_thread(body)


# ----------------------------------------------------------------------------- chunking into calls of at most 16
class _StubLib:
    """Stands in for libmbnb_mlora.so: records what each call receives (no device involved)."""

    def __init__(self, decline=()):
        self.calls, self.decline = [], set(decline)

    def mbnb_mlora_gemm4(self, x, M, K, qt, dt, bs, members, banks, ids, n, flags, stream):
        self.calls.append(dict(x=x, M=M, K=K, qt=qt, dt=dt, bs=bs, n=n, flags=flags, stream=stream, ids=ids,
                               members=[{f: getattr(members[i], f) for f, _ in gn.Member._fields_} for i in range(n)],
                               banks=[{f: getattr(banks[i], f) for f, _ in mn.Bank._fields_} for i in range(n)]))
        return mn.NOT_APPLICABLE if len(self.calls) - 1 in self.decline else 0

    def mbnb_mlora_last_error(self):
        return b"stub"


def _rows(count):
    return [(4096 + 16 * i, 8192 + 4 * i, 0, 0, 0 if i % 2 else 12288 + 2 * i, 16384 + 2 * i, 1 + i % 5, 0, 0) for i in range(count)]


def _banks(count):
    return [mn.NO_BANK if i % 3 == 0 else (20480 + 16 * i, 24576 + 2 * i, 32768 + 4 * i, 28672 + 4 * i, 1 + i % 5, 6) for i in range(count)]


@pytest.mark.parametrize("count, want", [(1, [1]), (16, [16]), (17, [16, 1]), (33, [16, 16, 1]), (0, [])])
def test_tables_are_cut_into_calls_of_at_most_sixteen(monkeypatch, count, want):
    stub = _StubLib()
    monkeypatch.setattr(mn, "_lib", stub)
    mn.reset_launch_log()
    rows, banks = _rows(count), _banks(count)
    assert mn.gemm4(P, 9, 2176, "nf4", torch.float16, 128, rows, banks, 4 * P, 78) == [True] * len(want)
    assert [c["n"] for c in stub.calls] == want
    assert mn.launch_log == [(n, sum(b[4] for b in banks[16 * c:16 * c + 16]), 9, 2176, torch.float16) for c, n in enumerate(want)]
    seen = [m for c in stub.calls for m in c["members"]]
    assert len(seen) == count
    for row, m in zip(rows, seen):       # every member once, in order, field for field (a 0 address reads back as None)
        assert tuple(m[f] or 0 for f, _ in gn.Member._fields_) == row
    for bank, b in zip(banks, [b for c in stub.calls for b in c["banks"]]):
        assert tuple(b[f] or 0 for f, _ in mn.Bank._fields_) == bank
    for c in stub.calls:
        assert (c["x"], c["M"], c["K"], c["qt"], c["dt"], c["bs"], c["flags"], c["stream"], c["ids"]) == \
            (P, 9, 2176, _native.NF4, _native.F16, 128, 0, 78, 4 * P)
    mn.reset_launch_log()
    assert mn.launch_log == []


def test_a_declined_chunk_is_reported_and_not_logged_and_a_failed_call_raises(monkeypatch):
    stub = _StubLib(decline=[1])
    monkeypatch.setattr(mn, "_lib", stub)
    mn.reset_launch_log()
    assert mn.gemm4(P, 2, 1024, "nf4", torch.float16, 64, _rows(17), _banks(17), P, None) == [True, False]
    assert mn.launch_log == [(16, sum(b[4] for b in _banks(16)), 2, 1024, torch.float16)]
    mn.reset_launch_log()
    with pytest.raises(ValueError, match="2 members but 1 banks"):
        mn.gemm4(P, 2, 1024, "nf4", torch.float16, 64, _rows(2), _banks(1), P, None)

    class Failing(_StubLib):
        def mbnb_mlora_gemm4(self, *a):
            return -1

    monkeypatch.setattr(mn, "_lib", Failing())
    with pytest.raises(RuntimeError, match=r"mlora\.gemm4 failed \(status -1\): stub"):
        mn.gemm4(P, 2, 1024, "nf4", torch.float16, 64, _rows(1), _banks(2)[1:], P, None)
    assert mn.launch_log == []


# ----------------------------------------------------------------------------- the function, on tensors that claim to be on the GPU
class _OnGpu(torch.Tensor):
    """A CPU tensor whose .device says cuda: functional's plan for a fused call can be followed up to the library call (a stand-in)."""
    device = property(lambda self: torch.device("cuda"))


class _TorchOnCpu:
    """``torch`` as functional.py sees it here: empty() allocates on the CPU whatever device is asked for."""

    def empty(self, *args, **kwargs):
        return torch.empty(*args, **dict(kwargs, device="cpu")).as_subclass(_OnGpu)

    def __getattr__(self, name):
        return getattr(torch, name)


class _OtherStub:
    """Stands in for the group, lora and batch libraries: none of them may be reached."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mbnb_"):
            raise AttributeError(name)

        def call(*a):
            self.calls.append(name)
            return 0
        return call


@pytest.fixture
def routed(monkeypatch):
    """(mlora stub, the other libraries' stub, the composed stand-in's calls) with functional's device plumbing neutralised."""
    mlora, other, composed = _StubLib(), _OtherStub(), []
    monkeypatch.setattr(mn, "_lib", mlora)
    for binding in (gn, ln, bn):
        monkeypatch.setattr(binding, "_lib", other)
    monkeypatch.setattr(F, "torch", _TorchOnCpu())
    monkeypatch.setattr(F, "on_device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(F, "stream_ptr", lambda device: 77)

    def multilora_composed(A, B, state, bias, bank, ids, compute_dtype):
        composed.append(int(state.shape[0]))
        return torch.full((*A.shape[:-1], int(state.shape[0])), float(len(composed)))

    monkeypatch.setattr(F, "_multilora_composed", multilora_composed)
    mn.reset_launch_log()
    yield mlora, other, composed
    mn.reset_launch_log()


def _gpu(t):
    return t.as_subclass(_OnGpu)


def _fake_group(Ns, K, T=torch.bfloat16, bs=64):
    weights = []
    for N in Ns:
        st = F.QuantState(absmax=_gpu(torch.ones(N * K // bs)), shape=torch.Size([N, K]), blocksize=bs, quant_type="nf4", dtype=T)
        weights.append((_gpu(torch.zeros(N * K // 2, dtype=torch.uint8)), st))
    return weights


def _fake_banks(Ns, K, Rs, S=3, T=torch.bfloat16):
    return [None if R is None else (_gpu(torch.zeros(S, R, K, dtype=T)), _gpu(torch.zeros(S, N, R, dtype=T)), _gpu(torch.ones(S)))
            for N, R in zip(Ns, Rs)]


@pytest.mark.parametrize("shape, M", [((2, 256), 2), ((16, 256), 16), ((2, 3, 256), 6), ((1, 256), 1), ((1, 1, 256), 1), ((17, 256), 17),
                                      ((3, 6, 256), 18)])
def test_only_two_to_sixteen_rows_reach_the_library_and_reach_nothing_else(routed, shape, M):
    mlora, other, composed = routed
    K, Ns, Rs = 256, (5, 3, 20), (4, None, 9)
    A = _gpu(torch.zeros(shape, dtype=torch.bfloat16))
    weights, banks = _fake_group(Ns, K), _fake_banks(Ns, K, Rs)
    bias = [None, _gpu(torch.zeros(3, dtype=torch.bfloat16)), None]
    ids = _gpu(torch.zeros(shape[:-1], dtype=torch.int32))
    ys = F.matmul_4bit_multilora_grouped(A, weights, banks, ids, bias)
    assert len(ys) == 3 and other.calls == []
    if 2 <= M <= 16:
        assert composed == [] and len(mlora.calls) == 1 and mn.launch_log == [(3, 13, M, K, torch.bfloat16)]
        c = mlora.calls[0]
        assert (c["M"], c["K"], c["bs"], c["n"], c["qt"], c["dt"], c["stream"], c["flags"]) == (M, K, 64, 3, _native.NF4, _native.BF16, 77, 0)
        assert c["ids"] == ids.data_ptr()      # int32 and contiguous: the caller's own tensor, so it may be overwritten in place
        # the outputs: dense [M, N_g] blocks of ONE allocation, in member order; each a view shaped like A
        outs = [m["out"] for m in c["members"]]
        assert [b - a for a, b in zip(outs, outs[1:])] == [2 * M * N for N in Ns[:-1]]
        assert [m["N"] for m in c["members"]] == list(Ns) and [bool(m["bias"]) for m in c["members"]] == [False, True, False]
        for y, N, m in zip(ys, Ns, c["members"]):
            assert y.shape == shape[:-1] + (N,) and y.dtype == torch.bfloat16 and y.is_contiguous() and y.data_ptr() == m["out"]
        # the workspaces: f32 [M, R_g] blocks of ONE allocation, none for the member without a bank
        t = [b["t"] for b in c["banks"]]
        assert [b["R"] for b in c["banks"]] == [4, 0, 9] and [b["S"] for b in c["banks"]] == [3, 0, 3] and t[1] is None and t[2] - t[0] == 4 * M * 4
        for i in (0, 2):
            assert [c["banks"][i][f] for f in ("a", "b", "scaling")] == [t_.data_ptr() for t_ in banks[i]]
    else:
        assert mlora.calls == [] and mn.launch_log == [] and composed == [5, 3, 20]


def test_other_ids_are_converted_once_and_wrong_ids_raise(routed):
    mlora, other, composed = routed
    K, Ns = 256, (5, 3)
    A = _gpu(torch.zeros(4, K, dtype=torch.bfloat16))
    weights, banks = _fake_group(Ns, K), _fake_banks(Ns, K, (4, 2))
    for ids in (_gpu(torch.zeros(4, dtype=torch.int64)), _gpu(torch.zeros(8, dtype=torch.int32))[::2]):
        F.matmul_4bit_multilora_grouped(A, weights, banks, ids)
        assert mlora.calls[-1]["ids"] not in (None, ids.data_ptr())
    assert len(mlora.calls) == 2 and composed == []
    with pytest.raises(ValueError, match="adapter_ids has shape"):
        F.matmul_4bit_multilora_grouped(A, weights, banks, _gpu(torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(TypeError, match="integer tensor"):
        F.matmul_4bit_multilora_grouped(A, weights, banks, _gpu(torch.zeros(4)))
    with pytest.raises(ValueError, match="2 weights but 1 banks"):
        F.matmul_4bit_multilora_grouped(A, weights, banks[:1], _gpu(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="2 weights but 3 biases"):
        F.matmul_4bit_multilora_grouped(A, weights, banks, _gpu(torch.zeros(4, dtype=torch.int32)), [None] * 3)
    unequal = [banks[0], _fake_banks(Ns[1:], K, (2,), S=4)[0]]
    with pytest.raises(ValueError, match=r"\[3, 4\] adapters; one S"):
        F.matmul_4bit_multilora_grouped(A, weights, unequal, _gpu(torch.zeros(4, dtype=torch.int32)))
    assert len(mlora.calls) == 2 and composed == [] and other.calls == []


@pytest.mark.parametrize("why", ["gradient", "bank gradient", "r=65", "f32 bank", "f64 scaling", "mixed formats", "other compute_dtype",
                                 "strided lora_B"])
def test_what_the_fused_launch_does_not_take_never_reaches_the_library(routed, why):
    mlora, other, composed = routed
    K, Ns, Rs = 256, (5, 3), (4, 2)
    A = _gpu(torch.zeros(4, K, dtype=torch.bfloat16))
    weights, cd = _fake_group(Ns, K), None
    if why == "r=65":
        Rs = (4, 65)
    banks = _fake_banks(Ns, K, Rs)
    if why == "gradient":
        A.requires_grad_(True)
    elif why == "bank gradient":
        banks[1][0].requires_grad_(True)
    elif why == "f32 bank":
        banks[1] = (banks[1][0].float(), banks[1][1].float(), banks[1][2])
    elif why == "f64 scaling":
        banks[0] = (banks[0][0], banks[0][1], _gpu(torch.ones(3, dtype=torch.float64)))
    elif why == "mixed formats":
        weights[1][1].quant_type = "fp4"
    elif why == "other compute_dtype":
        cd = torch.float32
    elif why == "strided lora_B":
        wide = _gpu(torch.zeros(3, 3, 4, dtype=torch.bfloat16))
        banks[1] = (banks[1][0], wide[:, :, ::2], banks[1][2])
        assert banks[1][1].shape == (3, 3, 2) and not banks[1][1].is_contiguous()
    F.matmul_4bit_multilora_grouped(A, weights, banks, _gpu(torch.zeros(4, dtype=torch.int32)), compute_dtype=cd)
    assert mlora.calls == [] and other.calls == [] and mn.launch_log == [] and composed == [5, 3]


def test_every_bank_none_is_the_grouped_call_and_a_declined_chunk_falls_back(routed, monkeypatch):
    mlora, other, composed = routed
    K, Ns = 256, (3,) * 17
    A = _gpu(torch.zeros(2, K, dtype=torch.bfloat16))
    weights = _fake_group(Ns, K)
    ids = _gpu(torch.zeros(2, dtype=torch.int32))
    seen = []
    monkeypatch.setattr(F, "matmul_4bit_grouped", lambda *a: seen.append(a) or ("grouped",))
    assert F.matmul_4bit_multilora_grouped(A, weights, [None] * 17, ids) == ("grouped",)
    assert len(seen) == 1 and seen[0][0] is A and mlora.calls == [] and composed == []
    mlora.decline = {1}
    zs = F.matmul_4bit_multilora_grouped(A, weights, _fake_banks(Ns, K, (2,) * 17), ids)
    assert [c["n"] for c in mlora.calls] == [16, 1] and mn.launch_log == [(16, 32, 2, K, torch.bfloat16)]
    assert composed == [3] and len(zs) == 17 and float(zs[16][0, 0]) == 1.0 and other.calls == []


# ----------------------------------------------------------------------------- the composed form (plain CPU tensors: it is torch ops)
def test_the_composed_form_selects_by_row_with_where(monkeypatch):
    """Rows without an adapter keep the base's bits, a negative zero included; a NaN in an unselected slot does not leak."""
    g = torch.Generator().manual_seed(3)
    M, K, N, R, S = 5, 32, 6, 4, 3
    A = torch.randn(M, K, generator=g)
    base = torch.randn(M, N, generator=g)
    base[1, 2] = -0.0
    base[3, 0] = -0.0
    monkeypatch.setattr(F, "matmul_4bit", lambda *a: base.clone())
    lora_A, lora_B = torch.randn(S, R, K, generator=g), torch.randn(S, N, R, generator=g)
    scaling = torch.tensor([0.5, 2.0, -1.25])
    lora_A[1], lora_B[1], scaling[1] = float("nan"), float("nan"), float("nan")
    ids = torch.tensor([0, -1, 2, 3, 2 ** 31 - 1])
    state = F.QuantState(absmax=torch.ones(1), shape=torch.Size([N, K]), blocksize=64, quant_type="nf4", dtype=torch.float32)
    y = F._multilora_composed(A, None, state, None, (lora_A, lora_B, scaling), ids, None)
    for m, s in enumerate(ids.tolist()):
        if 0 <= s < S:
            want = base[m] + ((A[m:m + 1] @ lora_A[s].t()) @ lora_B[s].t())[0] * scaling[s]
            torch.testing.assert_close(y[m], want)
        else:
            assert torch.equal(y[m].view(torch.int32), base[m].view(torch.int32)), m
    assert bool(torch.isfinite(y).all())


# ----------------------------------------------------------------------------- the modules
def _layer(N, K, S=3, r=4, bias=True):
    base = bnb.Linear4bit(K, N, bias=bias, compute_dtype=torch.bfloat16)
    return bnb.Linear4bitMultiLoRA(base, S, r, lora_alpha=8.0)


def test_module_keys_and_a_state_dict_round_trip():
    assert "Linear4bitMultiLoRA" in bnb.__all__ and "Linear4bitMultiLoRAGroup" in bnb.__all__ and "matmul_4bit_multilora_grouped" in bnb.__all__
    assert bnb.nn.Linear4bitMultiLoRA is bnb.Linear4bitMultiLoRA and bnb.matmul_4bit_multilora_grouped is F.matmul_4bit_multilora_grouped
    layer = _layer(6, 64)
    assert layer.lora_A.shape == (3, 4, 64) and layer.lora_B.shape == (3, 6, 4) and layer.lora_A.dtype == layer.lora_B.dtype == torch.bfloat16
    assert layer.scaling.dtype == torch.float32 and layer.scaling.tolist() == [2.0] * 3 and not bool(layer.lora_B.any())
    assert all(bool(layer.lora_A[s].any()) for s in range(3)) and not torch.equal(layer.lora_A[0], layer.lora_A[1])
    keys = set(layer.state_dict())
    assert {"lora_A", "lora_B", "scaling"} <= keys and keys - {"lora_A", "lora_B", "scaling"} == {"base." + k for k in layer.base.state_dict()}
    assert {n for n, _ in layer.named_parameters()} >= {"lora_A", "lora_B"} and "scaling" in dict(layer.named_buffers())
    group = bnb.Linear4bitMultiLoRAGroup([layer, _layer(2, 64, bias=False)])
    assert set(group.state_dict()) == {f"layers.0.{k}" for k in layer.state_dict()} | {f"layers.1.{k}" for k in group.layers[1].state_dict()}
    with torch.no_grad():
        layer.lora_B.normal_()
    layer.scaling[1] = 0.75
    other = bnb.Linear4bitMultiLoRAGroup([_layer(6, 64), _layer(2, 64, bias=False)])
    other.load_state_dict(group.state_dict())
    for k, v in group.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    with pytest.raises(TypeError):
        bnb.Linear4bitMultiLoRA(torch.nn.Linear(4, 4), 2, 2)
    with pytest.raises(ValueError):
        bnb.Linear4bitMultiLoRA(layer.base, 0, 2)
    with pytest.raises(ValueError):
        bnb.Linear4bitMultiLoRA(layer.base, 2, 0)
    with pytest.raises(ValueError, match="num_adapters"):
        bnb.Linear4bitMultiLoRAGroup([layer, _layer(2, 64, S=2)])
    with pytest.raises(ValueError, match="in_features"):
        bnb.Linear4bitMultiLoRAGroup([layer, _layer(2, 128)])
    with pytest.raises(ValueError):
        bnb.Linear4bitMultiLoRAGroup([])


def test_load_adapter_copies_in_place_and_keeps_the_addresses():
    layer = _layer(6, 64)
    before = [t.data_ptr() for t in layer.bank()]
    kept = [t.clone() for t in layer.bank()]
    a, b = torch.randn(4, 64), torch.randn(6, 4)
    layer.load_adapter(1, a, b, 0.375)
    assert [t.data_ptr() for t in layer.bank()] == before and layer.bank()[0] is layer.lora_A
    assert torch.equal(layer.lora_A[1], a.bfloat16()) and torch.equal(layer.lora_B[1], b.bfloat16()) and layer.scaling.tolist() == [2.0, 0.375, 2.0]
    for s in (0, 2):
        assert torch.equal(layer.lora_A[s], kept[0][s]) and torch.equal(layer.lora_B[s], kept[1][s])
    assert layer.lora_A.requires_grad and layer.lora_A.is_leaf
    with pytest.raises(IndexError):
        layer.load_adapter(3, a, b, 1.0)
    with pytest.raises(ValueError, match="pad a smaller rank"):
        layer.load_adapter(0, a[:2], b[:, :2], 1.0)


# ----------------------------------------------------------------------------- what the cases can tell
@pytest.mark.parametrize("Ns, K, qt, nested, bs, bias, S, Rs, dt, M, pattern", mc.ARGS, ids=mc.IDS)
def test_the_wrong_adapter_and_no_adapter_violate_the_fused_bound_in_every_row_that_has_one(Ns, K, qt, nested, bs, bias, S, Rs, dt, M, pattern):
    """What a kernel would return that picked the next slot (ids rotated by one slot; with S = 1 there is no other slot, and that half
    is void), or that dropped the epilogue, rounded to T, lies outside the bound in at least one element of EVERY row that has an
    adapter, so each fused case of tests/test_gpu_mlora.py can fail for either reason in each such row."""
    T = mc.DT[dt]
    ids = mc.ids_for(pattern, M, S)
    have = torch.tensor([0 <= i < S for i in ids])
    rotated = [(i + 1) % S if 0 <= i < S else i for i in ids]
    X = mc.x(K, dt, M)
    wrong, dropped = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
    for i, (N, R) in enumerate(zip(Ns, Rs)):
        if R is None:
            continue
        Wd = lc.member(N, K, dt, qt, nested, bs, seed=i)[3]
        b = lc.bias(N, dt, i) if i in bias else None
        bank = mc.bank(N, K, R, S, dt, i)
        r, Sm, Rrow = mc.reference(X, Wd, b, bank, ids)
        assert r.shape == (M, N) and bool(((Rrow[:, 0] == R) == have).all())
        limit = mc.bound(r, Sm, Rrow, K, T, "fused")
        wrong |= ((mc.reference(X, Wd, b, bank, rotated)[0].to(T).double() - r).abs() > limit).any(dim=1)
        dropped |= ((mc.reference(X, Wd, b, None, ids)[0].to(T).double() - r).abs() > limit).any(dim=1)
    assert bool((dropped == have).all()), f"rows {(dropped != have).nonzero().flatten().tolist()} cannot tell a dropped adapter"
    if S > 1:
        assert bool((wrong == have).all()), f"rows {(wrong != have).nonzero().flatten().tolist()} cannot tell the next slot's adapter"
