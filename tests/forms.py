"""
Shared pieces of the form tables of libmbnb_train.so and libmbnb_sparse.so (tests/switchback_cases.py, tests/int8_decomp_cases.py).

GPU side: `Run` is one run of a case -- where its operands go (an offset copy, or a guarded buffer under tests/guard.py's proxy with the
case's plan for functional.py's own allocations), the sentinel call before it, and name, variant, model and guard bands after it.
`memo` shares a CPU reference between the runs of a case (poisoned, and guarded under both fills).

Host side: the scans of a launcher source that the two host modules close their tables over.  They read the HOST part of the source, the
text from its `enum { KN_...` line on: `limit_counts` counts the literals, powers of two and named limits that sizes are compared with
there, `alignment_tests` lists the aligned(p, 8 | 16 | 256) tests by function.  Comparisons inside the kernels are not scanned: a limit a
kernel branches on is held through the named tile constants (TILE_CONSTANTS of the sparse table) and the tests written for them, and a new
in-kernel comparison with a literal passes these scans unnoticed.
"""
import collections
import re

import torch

from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F

_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def at(t, off):
    """t itself, or a copy that starts `off` bytes off the allocator's alignment."""
    if not off:
        return t
    nbytes = t.numel() * t.element_size()
    buf = torch.empty(nbytes + 32, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 256 == 0
    out = buf[off:off + nbytes].view(t.dtype).view(t.shape)
    out.copy_(t)
    return out


class Run:
    """`table`: the cases module (case_id, offset, model, PLAN_OPERANDS); `native`: the library's binding (last_kernel, last_variant);
    `sentinel(case)`: a call of another entry point of the library whose launcher sets no variant."""

    def __init__(self, table, native, sentinel, case, proxy=None, fill=None):
        self.table, self.native, self.sentinel = table, native, sentinel
        self.case, self.proxy, self.fill, self.id = case, proxy, fill, table.case_id(case)

    def off(self, operand):
        return self.table.offset(self.case, operand)

    def plan(self):
        return [(name, self.off(name)) for name in self.table.PLAN_OPERANDS.get(self.case["op"], ())]

    def begin(self):
        self.sentinel(self.case)
        if self.case["kernel"].endswith("+dense"):          # libmbnb_hip's own record: emptied by a call of its own that sets no variant
            dev = "cuda"
            F.embedding_8bit(torch.zeros(1, dtype=torch.long, device=dev), torch.ones(4, 64, dtype=torch.int8, device=dev), torch.ones(4, device=dev))
            assert _native.last_variant() == ""
        if self.proxy is not None:
            self.proxy.begin(self.fill, self.plan(), self.id)

    def put(self, name, t):
        if t is None:
            return None
        if self.proxy is not None:
            return self.proxy.place(name, t, self.off(name))
        return at(t, self.off(name))

    def end(self):
        case = self.case
        got = (self.native.last_kernel(), self.native.last_variant())
        assert got == (case["kernel"], case["variant"]), f"{self.id}: the library reports {got}"
        assert got == self.table.model(case), f"{self.id}: the restated conditions give {self.table.model(case)}"
        if case["kernel"].endswith("+dense"):
            assert _native.last_variant().startswith("dense"), f"{self.id}: the GEMM's variant is libmbnb_hip's record, got {_native.last_variant()!r}"
        torch.cuda.synchronize()
        if self.proxy is not None:
            self.proxy.check()


# ----------------------------------------------------------------------------- the scans of a launcher source
def code(src):
    return re.sub(r"//[^\n]*", "", src)


def host_part(src, marker):
    c = code(src)
    return c[c.index(marker):]


def limit_counts(src, marker):
    """How often the host side compares a size with each literal, power of two or named limit (`% n == 0` as "% n")."""
    host = host_part(src, marker)
    n = collections.Counter("% " + m for m in re.findall(r"% (\d+) (?:==|!=) 0", host))
    for t in re.findall(r"(?<![<>=!])(?:<=|>=|<|>|==)(?![<>=])\s*(\(\(int64_t\)1 << \d+\)|(?:k[A-Z]\w*|COO_\w+|CR_\w+|0x[0-9A-F]+|[1-9]\d*)\b)", host):
        n[re.sub(r"\(\(int64_t\)(1 << \d+)\)", r"\1", t)] += 1
    return dict(n)


def alignment_tests(src, marker):
    """{(function, pointer, bytes)} of every aligned(p, 8 | 16 | 256) on the host side."""
    found, fn = set(), None
    for line in host_part(src, marker).split("\n"):
        m = re.match(r"[a-z_0-9]+ \*?(\w+)\(", line)
        if m:
            fn = m.group(1).replace("mbnb_", "")
        found |= {(fn, a, int(b)) for a, b in re.findall(r"aligned\((\w+), (8|16|256)\)", line)}
    return found


def pair(cases, op, operand):
    """Cases of `op` offset in `operand` alone, each with the case that differs from it by that offset only."""
    strip = lambda c: {k: v for k, v in c.items() if k not in ("off", "kernel", "variant")}      # noqa: E731
    out = []
    for c in cases:
        if c["op"] == op and set(c.get("off", {})) == {operand}:
            out += [(c, b) for b in cases if "off" not in b and "view" not in b and strip(b) == strip(c)]
    return out
