"""
Every form and limit of csrc/nn_kernels.hip on guarded buffers: the quantized embedding lookups and the outlier-aware INT8 linear.

Each case of tests/nn_cases.py runs under tests/guard.py's proxy with each of its two fills, after a sentinel call of another entry
point.  Operands are placed inside guard bands at the case's offsets; functional.py's own `out` and `ws` are carved by the proxy's plan,
the C ABI cases bring their own.  Per run:

- embeddings: the library names embedding4 / embedding8, the output is bit-equal to the oracle's rows (zeros for a padding row and for an
  index out of range) under both fills, so every element was written;
- the linear's workspace, read back and split by the layout above outlier_linear_workspace_bytes: the int8 rows and the row scales are
  bit-equal to oracle.quantize_rowwise of x with the outlier columns zeroed (1e-8 and zero codes for a row that is zero outside them), the
  compact outlier activations bit-equal to x[:, outlier_indices] zero padded to a multiple of 16 where tests.nn_cases.model says they
  exist, the fill in their place where it says they do not, and the fill in every pad byte;
- the linear's output: every element within tests.test_gpu_elementwise.outlier_masked_bound of oracle.outlier_linear (a row sample on the
  two MFMA-sized cases), the library's name and variant the ones the model gives;
- a refused call answers MBNB_ERR_ARG with its text and writes nothing: `out` and `ws` still hold the fill;
- every band is intact.

x carries activations 64 times larger in the outlier columns and the int8 weight is nonzero there: a quantiser that lets one such column
into the row maximum, or a contraction that reads one, is far outside either check.  The worst err / bound is printed at the end (-s).

Measured on an MI355X: the module's 263 tests take 4 s, the slowest 0.5 s (the first call); worst err / bound 0.29 (the register form
with the compact activations under k_outlier_add), 0.26 on the fused epilogue, 0.12 and less elsewhere.  Before k_outlier_add looked at
its indices the two cases with the entries -1 and K failed: the gather read the fill next to x (NaN under 0xFF, 9.08 for -0.002 under 0x5A).
"""
import pytest
import torch

from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F
from tests import guard, nn_cases, nn_expect
from tests.elementwise import assert_bound_elementwise
from tests.forms import memo as _memo
from tests.guard import guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.nn_expect import DT

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERR_ARG = -1
WORST = {}
_SENTINEL = {}


def _sentinel(op):
    """A one-row lookup of the other width (an 8-bit one before everything but an 8-bit lookup): its launcher sets a known name and no variant."""
    if not _SENTINEL:
        _SENTINEL["q8"] = torch.ones(4, 64, dtype=torch.int8, device=DEV)
        _SENTINEL["s8"] = torch.ones(4, dtype=torch.float32, device=DEV)
        _SENTINEL["p4"] = torch.zeros(4, 32, dtype=torch.uint8, device=DEV)
        _SENTINEL["a4"] = torch.ones(4, 1, dtype=torch.float32, device=DEV)
        _SENTINEL["idx"] = torch.zeros(1, dtype=torch.int64, device=DEV)
    if op == "embedding_8bit":
        F.embedding_4bit(_SENTINEL["idx"], _SENTINEL["p4"], _SENTINEL["a4"], 64)
        want = "embedding4"
    else:
        F.embedding_8bit(_SENTINEL["idx"], _SENTINEL["q8"], _SENTINEL["s8"])
        want = "embedding8"
    assert (_native.last_kernel(), _native.last_variant()) == (want, "")


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _key(c):
    return tuple(sorted((k, repr(v)) for k, v in c.items() if k not in ("off", "err", "op") or (k == "op" and nn_cases.is_emb(c))))


def _alloc(proxy, name):
    got = [g for g in proxy.allocs if g.name == name]
    assert len(got) == 1, f"{name}: {[g.name for g in proxy.allocs]}"
    return got[0]


# ----------------------------------------------------------------------------------------------- embeddings
def _run_embedding(c, proxy, fill):
    cid = nn_cases.case_id(c)
    a, b = _memo(("emb", c["op"], c["dim"], c.get("bs")), lambda: nn_expect.embedding_operands(c))
    want = _memo(("emb_want", _key(c)), lambda: nn_expect.embedding_expected(c, a, b))
    idx, pad = nn_expect.indices(c)
    _sentinel(c["op"])
    proxy.begin(fill, [("out", nn_cases.offset(c, "out"))], cid)
    dt = DT[c["dt"]]
    idx_d = proxy.place("idx", idx.to(DEV))
    if c["op"] == "embedding_4bit":
        pa = proxy.place("packed", a.to(DEV), nn_cases.offset(c, "packed"))
        assert pa.data_ptr() % 16 == nn_cases.offset(c, "packed")
        y = F.embedding_4bit(idx_d, pa, proxy.place("absmax", b.to(DEV)), c["dim"], c["bs"], c["qt"], pad, dt)
        name = "embedding4"
    else:
        w = proxy.place("w", a.to(DEV), nn_cases.offset(c, "w"))
        assert w.data_ptr() % 16 == nn_cases.offset(c, "w")
        y = F.embedding_8bit(idx_d, w, proxy.place("scales", b.to(DEV)), pad, dt)
        name = "embedding8"
    assert (_native.last_kernel(), _native.last_variant()) == (name, ""), cid
    out = _alloc(proxy, "out")
    assert y.data_ptr() == out.view.data_ptr() and y.data_ptr() % 16 == nn_cases.offset(c, "out")
    torch.cuda.synchronize()
    assert y.dtype == dt and tuple(y.shape) == tuple(idx.shape) + (c["dim"],)
    bad = (_bits(y) != _bits(want)).nonzero()
    assert bad.numel() == 0, f"{cid} (fill 0x{fill:02X}, {nn_cases.model(c)}): {bad.shape[0]} elements differ from the oracle, the first at {bad[0].tolist()}"
    proxy.check()


# ----------------------------------------------------------------------------------------------- the outlier-aware linear
def _expected(c):
    def make():
        ops = nn_expect.linear_operands(c)
        xq, scales, xo = nn_expect.workspace_expected(c, ops)
        rows = nn_expect.row_sample(c["M"])
        err = nn_cases.model(c)[0] == "error"
        ref = None if err else nn_expect.reference_output(c, ops, rows)
        return ops, xq, scales, xo, rows, ref
    return _memo(("lin", _key(c)), make)


def _bound(c, ops, rows, ref):
    def make():
        import oracle
        from tests.test_gpu_elementwise import outlier_masked_bound
        dt = DT[c["dt"]]
        Wd = oracle.dequantize_rowwise(ops["q"], ops["s"], dt).to(DEV)
        return outlier_masked_bound(ops["x"][rows].to(DEV), Wd, ops["pos"], ops["ow"].to(DEV), None if ops["b"] is None else ops["b"].to(DEV), ref.to(DEV), dt)
    return _memo(("lin_bound", _key(c)), make)


def _check_workspace(c, ws, fill, xq_e, scales_e, xo_e, cid):
    n = nn_cases.n_entries(c)
    M, K = c["M"], c["K"]
    xq, scales, xo, pads_ok = nn_expect.split_workspace(ws.cpu(), M, K, n, fill)
    bad = (xq != xq_e).nonzero()
    assert bad.numel() == 0, (f"{cid} (fill 0x{fill:02X}): {bad.shape[0]} int8 codes differ from quantize_rowwise of the masked x, the first at "
                              f"{bad[0].tolist()}: {int(xq[tuple(bad[0])])} for {int(xq_e[tuple(bad[0])])}")
    bad = (_bits(scales) != _bits(scales_e)).nonzero()
    assert bad.numel() == 0, f"{cid} (fill 0x{fill:02X}): the scale of row {int(bad[0])} is {float(scales[bad[0]])!r}, the masked row's is {float(scales_e[bad[0]])!r}"
    if xo_e is not None:
        got = xo.view(torch.int16).reshape(M, -1)
        bad = (got != _bits(xo_e)).nonzero()
        assert bad.numel() == 0, f"{cid} (fill 0x{fill:02X}): {bad.shape[0]} compact outlier activations differ from x[:, outlier_indices] zero padded, the first at {bad[0].tolist()}"
    else:
        assert bool((xo == fill).all()), f"{cid} (fill 0x{fill:02X}): the region of the compact outlier activations was written though they do not exist"
    assert pads_ok, f"{cid} (fill 0x{fill:02X}): a pad byte of the workspace was written"
    # the floor rows
    floor = float(torch.tensor(1e-8, dtype=torch.float32))
    for r in ([M - 1] if M >= 2 else []) + ([M - 2] if M >= 3 and c["n_out"] else []):      # all zeros; zero outside the outlier columns
        assert float(scales[r]) == floor and not bool(xq[r].any()), f"{cid}: row {r} takes the 1e-8 floor and all-zero codes"


def _run_linear(c, proxy, fill):
    cid = nn_cases.case_id(c)
    M, N, K, dt = c["M"], c["N"], c["K"], DT[c["dt"]]
    ops, xq_e, scales_e, xo_e, rows, ref = _expected(c)
    m = nn_cases.model(c)
    abi = c["op"] == "outlier_abi"
    _sentinel(c["op"])
    proxy.begin(fill, [] if abi else [("out", nn_cases.offset(c, "out")), ("ws", nn_cases.offset(c, "ws"))], cid)
    oi, ow = nn_expect.given_indices(c, ops)
    n = oi.numel()
    assert n == nn_cases.n_entries(c)
    x = proxy.place("x", ops["x"].to(DEV), nn_cases.offset(c, "x"))
    q = proxy.place("q", ops["q"].to(DEV))
    s = proxy.place("s", ops["s"].to(DEV))
    oi_d = proxy.place("oidx", oi.to(DEV)) if n else torch.empty(0, dtype=torch.int64, device=DEV)
    ow_d = proxy.place("ow", ow.to(DEV), nn_cases.offset(c, "ow")) if n else torch.empty(N, 0, dtype=dt, device=DEV)
    b = None if ops["b"] is None else proxy.place("b", ops["b"].to(DEV))
    assert x.data_ptr() % 16 == nn_cases.offset(c, "x")
    if abi:
        nbytes = nn_cases.ws_bytes(c)
        if c.get("ws") == "exact":
            assert nbytes == _native.lib().mbnb_outlier_linear_workspace_bytes(M, K, n)
        y = proxy.place_empty("out", (M, N), dt, DEV, nn_cases.offset(c, "out"))
        ws = proxy.place_empty("ws", (nbytes,), torch.uint8, DEV, nn_cases.offset(c, "ws"))
        rc = _native.lib().mbnb_outlier_linear(_native.ptr(x), _native.DTYPE_CODE[dt], M, K, _native.ptr(q), _native.ptr(s), N, _native.ptr(oi_d if n else None), n,
                                               _native.ptr(ow_d if n else None), _native.ptr(b), _native.ptr(y), _native.ptr(ws), nbytes, _native.stream_ptr(DEV))
        if "err" in c:
            assert m == ("error", c["err"])
            assert rc == ERR_ARG, (cid, rc, _native.lib().mbnb_last_error())
            assert c["err"].encode() in _native.lib().mbnb_last_error(), _native.lib().mbnb_last_error()
            torch.cuda.synchronize()
            assert bool((_alloc(proxy, "out").buf == fill).all()) and bool((_alloc(proxy, "ws").buf == fill).all()), f"{cid}: a refused call wrote something"
            proxy.check()
            return
        assert rc == 0, (cid, rc, _native.lib().mbnb_last_error())
    else:
        assert "err" not in c
        y = F.outlier_linear(x, q, s, oi_d, ow_d, b, dt)
        ws = _alloc(proxy, "ws").view
        assert y.data_ptr() == _alloc(proxy, "out").view.data_ptr() and ws.numel() == nn_cases.ws_bytes(c)
    got = (_native.last_kernel(), _native.last_variant())
    assert got == (m[3], m[4]), f"{cid}: the library reports {got}, the restated conditions give {m}"
    assert y.data_ptr() % 16 == nn_cases.offset(c, "out") and ws.data_ptr() % 256 == nn_cases.offset(c, "ws")
    torch.cuda.synchronize()
    _check_workspace(c, ws, fill, xq_e, scales_e, xo_e, cid)
    bound = _bound(c, ops, rows, ref)
    name = f"{m[0]} {'xo' if m[1] else 'no xo'} {m[2] if isinstance(m[2], str) else 'add'}"
    ratio = assert_bound_elementwise(y[rows.to(DEV)], ref.to(DEV).double(), bound, got[0], f"outlier_linear ({cid})")
    print(f"\nnn forms {cid}: max err / bound {ratio:.3g}")
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    first = _memo(("lin_y", cid), lambda: _bits(y))
    assert torch.equal(first, _bits(y)), f"{cid} (fill 0x{fill:02X}): the output differs from the first fill's: an element was not written"
    proxy.check()


@pytest.mark.parametrize("fill", guard.FILLS, ids=lambda f: f"fill{f:02X}")
@pytest.mark.parametrize("case", nn_cases.CASES, ids=nn_cases.case_id)
def test_case_guarded(case, fill, guarded_alloc):
    (_run_embedding if nn_cases.is_emb(case) else _run_linear)(case, guarded_alloc, fill)
    assert guarded_alloc.allocs, "nothing went through the guarded proxy"


def test_zz_report_the_worst_ratio_per_form():
    for name, ratio in sorted(WORST.items()):
        print(f"\nnn forms: {name}: worst err / bound {ratio:.3g}")
    assert all(ratio <= 1.0 for ratio in WORST.values())
