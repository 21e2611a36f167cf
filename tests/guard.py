"""
Guarded allocations for the GPU tests that run a kernel form inside guard bands: the quantise / dequantise forms (tests/quant_cases.py)
every case of the train and sparse libraries' tables that launches no GEMM (tests/forms.py), and the input-gradient path, its dense
route included (tests/grad_cases.py).

``guarded_alloc`` replaces the name ``torch`` inside ``mps_bitsandbytes_amd.functional`` with a proxy that forwards every attribute
to torch except ``empty``: the request is carved out of a larger uint8 buffer with a guard band of GUARD bytes on each side, every
byte of which -- bands and payload -- is set to the proxy's fill; the caller gets the inner view, starting at the byte offset
modulo 16 the test asked for (``plan``; an offset of 16 and more puts a workspace off its 256-byte alignment), and the proxy remembers
the allocation.  ``check()`` then requires every guard byte to
still hold the fill: a store past either end of an output, which the caching allocator's 512-byte rounding would have swallowed,
is reported with the op, the form, the buffer and the byte offset from the buffer's end (or start).

``place`` puts a tensor of the test's own (an input, a caller's ``out=``) into such a buffer the same way.

A case runs under two fills, 0xFF and 0x5A.  An element the kernel never wrote holds the fill: it can equal the oracle's value under
one fill (0xFF is a legal int8 / uint8 / packed code) but not under both, so equality under both proves it was written.

The checker works on any device (tests/test_quant_forms_host.py exercises it on CPU tensors).
"""
import pytest
import torch

from mps_bitsandbytes_amd import functional as _functional

GUARD = 256            # bytes on each side; a multiple of 16, so the payload's offset modulo 16 is the one asked for
FILLS = (0xFF, 0x5A)


class GuardViolation(AssertionError):
    pass


class Guarded:
    """One allocation: `buf` (uint8) = [GUARD + offset bytes of band | payload | >= GUARD bytes of band]."""

    def __init__(self, name, buf, start, nbytes, fill, view):
        self.name, self.buf, self.start, self.nbytes, self.fill, self.view = name, buf, start, nbytes, fill, view

    def violation(self):
        """None, or (side, offset): the first byte of a band that no longer holds the fill; offset counts from the payload's end
        (+0 is the first byte past it) or back from its start (-1 is the byte just before it)."""
        end = self.start + self.nbytes
        after = self.buf[end:]
        bad = (after != self.fill).nonzero()
        if bad.numel():
            return "end", int(bad[0])
        before = self.buf[:self.start]
        bad = (before != self.fill).nonzero()
        if bad.numel():
            return "start", int(bad[-1]) - self.start
        return None


def _carve(name, shape, dtype, device, fill, offset):
    esize = torch.empty(0, dtype=dtype).element_size()
    assert 0 <= offset < GUARD and offset % esize == 0, f"{name}: offset {offset} is not a multiple of the element size {esize}"
    numel = 1
    for s in shape:
        numel *= int(s)
    nbytes = numel * esize
    start = GUARD + offset
    tail = GUARD + (-(start + nbytes)) % 16
    buf = torch.empty(start + nbytes + tail, dtype=torch.uint8, device=device)
    buf.fill_(fill)
    assert buf.data_ptr() % 16 == 0
    view = buf[start:start + nbytes].view(dtype).view(tuple(shape))
    assert view.data_ptr() % 16 == offset % 16 and view.is_contiguous()      # (an offset of 16 and more: off a 256-byte alignment)
    return Guarded(name, buf, start, nbytes, fill, view)


class GuardedTorch:
    """``torch`` as functional.py sees it under the fixture."""

    def __init__(self):
        self.fill = FILLS[0]
        self.plan = []          # (name, offset) of the next allocations, in order; once used up, "extra<i>" at offset 0
        self.allocs = []
        self.where = ""         # "op form", for the messages

    def begin(self, fill, plan=(), where=""):
        self.fill, self.plan, self.allocs, self.where = fill, list(plan), [], where

    def empty(self, *args, **kwargs):
        meta = torch.empty(*args, **dict(kwargs, device="meta"))
        name, offset = self.plan.pop(0) if self.plan else (f"extra{len(self.allocs)}", 0)
        g = _carve(name, meta.shape, meta.dtype, kwargs.get("device", "cpu"), self.fill, offset)
        self.allocs.append(g)
        return g.view

    def place(self, name, t, offset=0):
        """A copy of `t` inside a guarded buffer at `offset` modulo 16 (on t's device)."""
        g = _carve(name, t.shape, t.dtype, t.device, self.fill, offset)
        g.view.copy_(t)
        self.allocs.append(g)
        return g.view

    def place_empty(self, name, shape, dtype, device, offset=0):
        g = _carve(name, shape, dtype, device, self.fill, offset)
        self.allocs.append(g)
        return g.view

    def check(self):
        for g in self.allocs:
            v = g.violation()
            if v is not None:
                side, off = v
                at = f"{off} bytes past its end" if side == "end" else f"{-off} bytes before its start"
                raise GuardViolation(f"{self.where}: a write outside buffer {g.name!r} ({g.nbytes} bytes, fill 0x{g.fill:02X}): "
                                     f"first changed guard byte {at} (offset {off:+d})")

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.fixture
def guarded_alloc(monkeypatch):
    proxy = GuardedTorch()
    monkeypatch.setattr(_functional, "torch", proxy)
    yield proxy
