"""
Poisoned allocations for the GPU suite.

``poisoned_alloc`` replaces the name ``torch`` inside ``mps_bitsandbytes_amd.functional`` with a proxy that forwards every
attribute to torch except ``empty``, whose result comes back with every byte set to 0xFF.  Every output, f32 split-K
partial and 16-bit decode-once scratch the Python API hands the library comes from there, so:

- in an f16 / bf16 / f32 view each element starts as a NaN: an output element that no kernel writes, a workspace slot read
  before anything wrote it, or an epilogue that folds the old contents of its output in (``0 * old``) shows up as a NaN
  instead of passing on whatever plausible value the caching allocator returned;
- in an int8 / uint8 view each element starts as -1 / 255.

The proxy is an attribute of the module, so the backward passes (autograd's device thread) see it too; in a graph-captured
call the fill is one more node of the graph.  The fixture counts what it poisons: a test that looked anything up in
functional's ``torch`` and had nothing poisoned fails at teardown, so a refactor away from ``torch.empty`` cannot switch the
poisoning off unnoticed.  With MBNB_POISON_REPORT set, the count per test module is printed when the process exits.
"""
import atexit
import os
import sys

import pytest
import torch

from mps_bitsandbytes_amd import functional as _functional

COUNTS: dict = {}     # test module -> allocations poisoned for its tests


class PoisonedTorch:
    """``torch`` as functional.py sees it under the fixture."""

    def __init__(self):
        self.poisoned = 0
        self.lookups = 0

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.numel() > 0:
            t.reshape(-1).view(torch.uint8).fill_(0xFF)
        self.poisoned += 1
        return t

    def __getattr__(self, name):
        self.lookups += 1
        return getattr(torch, name)


@pytest.fixture
def poisoned_alloc(monkeypatch, request):
    proxy = PoisonedTorch()
    monkeypatch.setattr(_functional, "torch", proxy)
    yield proxy
    mod = request.module.__name__
    COUNTS[mod] = COUNTS.get(mod, 0) + proxy.poisoned
    assert proxy.poisoned > 0 or proxy.lookups == 0, \
        "functional.py ran under poisoned_alloc but allocated nothing through torch.empty: the poisoning is not reaching it"


def _report():
    if COUNTS and os.environ.get("MBNB_POISON_REPORT"):
        print("poisoned allocations per module: " + ", ".join(f"{k} {v}" for k, v in sorted(COUNTS.items())), file=sys.stderr)


atexit.register(_report)
