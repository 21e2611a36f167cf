"""
Every form of every quantiser on the boundary data of tests/rounding_cases.py, bit for bit against the CPU oracle.

The data puts values within a few steps of every decision boundary of a quantiser -- the midpoints between 4-bit codes, the half-integers
of the int8 rounding, the mantissa midpoints and the powers of two of the FP8 encoder -- at 512 mantissas of the scale and several exponents,
at the edges of the kernels' fast paths and of the clamps (tests/test_rounding_host.py proves on the CPU that a last-bit error in a quotient,
a product or a threshold changes hundreds of expected outputs).  Each test reshapes the flat list of blocks or rows so that
quant_cases.model_form yields the form, runs the public API once, asserts the form the library reports and compares every output with the
oracle at zero tolerance (NaN by position).  f32 carries the sweep; f16 and bf16 run the same builders in their own steps.

A mismatch is reported with the count, the first differing element's input bits, its scale's bits, the bits of the quotient (or product) of
the restatement, and both outputs: that line names the threshold or tie at fault.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from mps_bitsandbytes_amd import _native, _sparse_native
from mps_bitsandbytes_amd import functional as F
from tests import int8_decomp_emul as emul
from tests import nn_cases, quant_cases
from tests import rounding_cases as rc
from tests.test_gpu_quant_forms import _first_diff, _same

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = rc.DT
DTS = ("f32", "f16", "bf16")
F32 = np.float32


def _cpu(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt])


def _dev(t, off=0):
    """t on the device; off: that many elements past a 16-byte boundary (the _s / scalar forms)."""
    if not off:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size() and v.is_contiguous()
    return v


def _rows_of(x, per_row):
    """Blocks [nblk, bs] -> a matrix with per_row blocks a row, blocks of zeros after the last."""
    nblk, bs = x.shape
    rows = -(-nblk // per_row)
    m = np.zeros((rows * per_row, bs), dtype=F32)
    m[:nblk] = x
    return m.reshape(rows, per_row * bs)


def _form(op, shape, dt, off, **kw):
    c = dict(op=op, shape=tuple(shape), dt=dt, **kw)
    if off:
        c["align"] = {"in": off * quant_cases.ESIZE[dt]}
    return quant_cases.model_form(c)


def _hex(v):
    return f"0x{rc.bits(v):08x}"


def _check(name, got, want, detail=None):
    if not _same(got, want):
        msg = f"{name} differs from the oracle: {_first_diff(got, want)}"
        if detail is not None:
            msg += "; " + detail(got.detach().cpu().reshape(-1), want.reshape(-1))
        raise AssertionError(msg)


# ----------------------------------------------------------------------------------------------- 4-bit
# (form, blocksize, blocks per row): spans of max(bs, 512) values per row decide between wave, rows and rows2 / big and big_rows
Q4_FORMS = [("q4_tiny", 4, 64), ("q4_wave", 128, 8), ("q4_rows", 128, 16), ("q4_rows2", 128, 32), ("q4_big", 1024, 2), ("q4_big_rows", 1024, 4),
            ("q4_dq", 128, 8)]


@functools.lru_cache(maxsize=4)
def _q4_own(qt, dt, bs):
    return rc.q4_own(qt, dt, bs)


@functools.lru_cache(maxsize=4)
def _q4_given(qt, dt, bs):
    return rc.q4_given(qt, dt, bs) if bs <= 8 else rc.q4_given(qt, dt, bs, exps=(0,), n=16)


def _q4_detail(d, m, per_row, qt):
    x_flat, bs = m.reshape(-1), d["bs"]
    am = np.concatenate([d["am"], np.full(m.size // bs - len(d["am"]), rc.CLAMP, dtype=F32)])

    def detail(got, want):
        byte = int((got != want).nonzero()[0])
        g, w = int(got[byte]), int(want[byte])
        i = 2 * byte + (0 if (g ^ w) & 0xF else 1)
        q = rc.quotient(x_flat[i], am[i // bs])
        return (f"element {i}: x {_hex(x_flat[i])} ({x_flat[i]!r}), absmax {_hex(am[i // bs])} ({am[i // bs]!r}), x / absmax {_hex(q)} ({q!r}), "
                f"code {(g >> (4 * (i & 1))) & 0xF} for {(w >> (4 * (i & 1))) & 0xF} ({qt})")
    return detail


def _run_q4(d, form, per_row, qt, dt, off, cs=False, given=False, last=None):
    """last: the form the library reports when it is not the 4-bit launch's (the two-launch route of nested statistics ends with the int8
    quantiser of the absmax)."""
    bs = d["bs"]
    m = _rows_of(d["x"], per_row)
    x = _cpu(m, dt)
    nblk = m.size // bs
    am = None
    if given:
        am = torch.from_numpy(np.concatenate([d["am"], np.ones(nblk - len(d["am"]), dtype=F32)]))
    want_form = _form("quantize_4bit", m.shape, dt, off, bs=bs, qt=qt, cs=cs, given=given)
    assert want_form == form + ("_s" if off else ""), f"the shape {m.shape} is for {want_form}, not {form}"
    p, a, st2 = oracle.quantize_4bit(x, bs, qt, cs, am)
    packed, st = F.quantize_4bit(_dev(x, off), absmax=None if am is None else am.to(DEV), blocksize=bs, compress_statistics=cs, quant_type=qt)
    got_form = _native.last_kernel()
    torch.cuda.synchronize()
    assert got_form == (last or want_form), f"dispatched {got_form!r}, the data is shaped for {last or want_form!r}"
    dd = dict(d, am=d["am"] if am is None else am.numpy()[:len(d["am"])])
    _check(f"{want_form} {qt} {dt}: packed", packed.reshape(-1), p, _q4_detail(dd, m, per_row, qt))
    if cs:
        ab, a2 = (a if am is None else am).numpy(), st2[0].numpy()         # what the nested quantisation reads: the blocks' absmax
        if am is None:
            ab = oracle.quantize_4bit(x, bs, qt, False)[1].numpy()
        _check(f"{want_form} {qt} {dt}: absmax codes", st.absmax, a, _int8_detail(ab, lambda i: a2[i // 256]))
        _check(f"{want_form} {qt} {dt}: absmax2", st.state2.absmax, st2[0])
    else:
        _check(f"{want_form} {qt} {dt}: absmax", st.absmax, a)


# the _s twins: the input one element past a 16-byte boundary (q4_tiny has one form for every alignment)
Q4_F32 = [(f, bs, n, qt, off) for f, bs, n in Q4_FORMS for qt in ("nf4", "fp4") for off in (0, 1) if not (f == "q4_tiny" and off)]


@pytest.mark.parametrize("form,bs,per_row,qt,off", Q4_F32, ids=[f"{f[0]}{'_s' if f[4] else ''}-{f[3]}" for f in Q4_F32])
def test_q4_own_absmax_f32(form, bs, per_row, qt, off):
    _run_q4(_q4_own(qt, "f32", bs), form, per_row, qt, "f32", off, cs=form == "q4_dq")


@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("qt", ("nf4", "fp4"))
@pytest.mark.parametrize("form,bs,per_row", Q4_FORMS, ids=[f[0] for f in Q4_FORMS])
def test_q4_own_absmax_16bit(form, bs, per_row, qt, dt):
    _run_q4(_q4_own(qt, dt, bs), form, per_row, qt, dt, 0, cs=form == "q4_dq")


Q4_GIVEN = [("q4_tiny", 4, 64), ("q4_wave", 8, 64), ("q4_rows", 8, 256), ("q4_rows2", 8, 512), ("q4_big", 1024, 2), ("q4_big_rows", 1024, 4)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qt", ("nf4", "fp4"))
@pytest.mark.parametrize("form,bs,per_row", Q4_GIVEN, ids=[f[0] for f in Q4_GIVEN])
def test_q4_supplied_absmax(form, bs, per_row, qt, dt):
    """The f32 absmax sweeps around x / t: how 16-bit inputs reach boundary quotients.  The odd dtype / form pairs run one element off."""
    off = 1 if (dt == "f16" and form in ("q4_wave", "q4_rows2", "q4_big")) else 0
    _run_q4(_q4_given(qt, dt, bs), form, per_row, qt, dt, off, given=True)


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_fp4_exact_ties_16bit(dt):
    d = rc.fp4_ties_16bit(dt)
    _run_q4(d, "q4_wave", 4, "fp4", dt, 0)
    _run_q4(d, "q4_dq", 4, "fp4", dt, 1, cs=True)


@pytest.mark.parametrize("dt", DTS)
def test_q4_nested_statistics_meet_int8_ties(dt):
    """The absmax values of quantize_4bit(compress_statistics=True) sit on the ties of their own int8 quantisation: the fused q4_dq form
    and the two-launch route (a supplied absmax) both."""
    d = rc.int8_absmax_blocks(dt)
    dd = dict(x=d["x"], am=d["absmax"], bs=d["bs"])
    _run_q4(dd, "q4_dq", 64, "nf4", dt, 0, cs=True)
    _run_q4(dd, "q4_dq", 64, "fp4", dt, 1, cs=True)
    nested = _form("quantize_blockwise", (len(d["absmax"]),), "f32", 0, bs=256)
    assert nested == "q8_row_loop"
    _run_q4(dd, "q4_wave", 64, "nf4", dt, 0, cs=True, given=True, last=nested)


# ----------------------------------------------------------------------------------------------- int8
def _int8_detail(x, am_of):
    xf = x.reshape(-1)

    def detail(got, want):
        i = int((got != want).nonzero()[0])
        am = am_of(i)
        p = rc.int8_product(xf[i], am)
        return (f"element {i}: x {_hex(xf[i])} ({xf[i]!r}), absmax {_hex(am)} ({am!r}), (1 / absmax) * 127 {_hex(rc.rscale127(am))}, product {_hex(p)} ({p!r}), "
                f"code {int(got[i])} for {int(want[i])}")
    return detail


@functools.lru_cache(maxsize=2)
def _int8_rows(dt, width, n=rc.N_MANT):
    return rc.int8_rows(dt, width=width, n=n)


ROW_FORMS = [("f32", 1272, 0, "q8_row_loop"), ("f32", 1271, 0, "q8_row_scalar"), ("f32", 1272, 1, "q8_row_scalar"),
             ("f16", 1272, 0, "q8_row_regs"), ("bf16", 1272, 0, "q8_row_regs"), ("f16", 1271, 0, "q8_row_scalar"), ("bf16", 1272, 1, "q8_row_scalar"),
             ("f16", 8200, 0, "q8_row_loop"), ("bf16", 8200, 0, "q8_row_loop")]


@pytest.mark.parametrize("dt,width,off,form", ROW_FORMS, ids=[f"{f[3]}-{f[0]}-{f[1]}+{f[2]}" for f in ROW_FORMS])
def test_int8_rowwise(dt, width, off, form):
    d = _int8_rows(dt, width, rc.N_MANT if width < 8000 else 64)
    x = _cpu(d["x"], dt)
    assert _form("quantize_rowwise", d["x"].shape, dt, off) == form
    wq, ws = oracle.quantize_rowwise(x)
    q, s = F.quantize_rowwise(_dev(x, off))
    got = _native.last_kernel()
    torch.cuda.synchronize()
    assert got == form, f"dispatched {got!r}"
    _check(f"{form} {dt}: scales", s, ws)
    _check(f"{form} {dt}: codes", q, wq, _int8_detail(d["x"], lambda i: d["am"][i // width]))


@pytest.mark.parametrize("dt", DTS)
def test_int8_blockwise(dt):
    """q8_block with the block's own and with a supplied absmax (the clamp's values included), and the row forms through quantize_blockwise."""
    for given in (False, True):
        b = rc.int8_blocks(dt, 32, given=given)
        x = _cpu(b["x"], dt).reshape(-1)
        am = torch.from_numpy(b["am"]) if given else None
        wq, wa = oracle.quantize_blockwise(x, 32, am)
        q, st = F.quantize_blockwise(_dev(x, 1 if given else 0), absmax=None if am is None else am.to(DEV), blocksize=32)
        got = _native.last_kernel()
        torch.cuda.synchronize()
        assert got == "q8_block", got
        _check(f"q8_block {dt} given={given}: absmax", st.absmax, wa)
        _check(f"q8_block {dt} given={given}: codes", q, wq, _int8_detail(b["x"], lambda i: b["am"][i // 32]))
    d = _int8_rows(dt, 1272)
    x = _cpu(d["x"], dt).reshape(-1)
    form = "q8_row_loop" if dt == "f32" else "q8_row_regs"
    assert _form("quantize_blockwise", x.shape, dt, 0, bs=1272) == form
    wq, wa = oracle.quantize_blockwise(x, 1272)
    q, st = F.quantize_blockwise(_dev(x), blocksize=1272)
    got = _native.last_kernel()
    torch.cuda.synchronize()
    assert got == form, got
    _check(f"blockwise {form} {dt}: absmax", st.absmax, wa)
    _check(f"blockwise {form} {dt}: codes", q, wq, _int8_detail(d["x"], lambda i: d["am"][i // 1272]))


DQ_FORMS = [("", 0, "dquant8_rc"), ("", 1, "dquant1_rc"), ("r", 0, "dquant8_c"), ("r", 1, "dquant1_c"), ("c", 0, "dquant8_r"), ("c", 1, "dquant1_r"),
            ("rc", 0, "dquant8_given"), ("rc", 1, "dquant1_given")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("given,off,form", DQ_FORMS, ids=[f[2] for f in DQ_FORMS])
def test_double_quant(given, off, form, dt):
    """The rows' boundaries in one matrix, the columns' in its transpose; a supplied statistic is the matrix's own on the boundary side and
    another scale set on the other side, so row and column scales differ."""
    d = _int8_rows(dt, 1272)
    rows = d["x"][::4]
    t = np.zeros((1272, (rows.shape[0] + 7) // 8 * 8), dtype=F32)
    t[:, :rows.shape[0]] = rows.T
    other = rc.scales("f32", (0, -3, 5), 1024)[0]
    for m, axis in ((rows, 1), (t, 0)):
        x = _cpu(m, dt)
        own = np.maximum(np.abs(x.float().numpy()).max(axis=axis), rc.CLAMP)
        rs = cs = None
        if "r" in given:
            rs = torch.from_numpy(own if axis == 1 else other[:m.shape[0]].copy())
        if "c" in given:
            cs = torch.from_numpy(own if axis == 0 else other[:m.shape[1]].copy())
        assert _form("double_quant", m.shape, dt, off, given=given) == form
        woc, wor, wcs, wrs, _ = oracle.double_quant(x, cs, rs)
        oc, orow, gcs, grs, _ = F.double_quant(_dev(x, off), None if cs is None else cs.to(DEV), None if rs is None else rs.to(DEV))
        got = _native.last_kernel()
        torch.cuda.synchronize()
        assert got == form, f"dispatched {got!r}"
        rsn, csn, cols = wrs.numpy(), wcs.numpy(), m.shape[1]
        _check(f"{form} {dt}: row statistics", grs, wrs)
        _check(f"{form} {dt}: column statistics", gcs, wcs)
        _check(f"{form} {dt}: codes by row", orow, wor, _int8_detail(x.float().numpy(), lambda i: rsn[i // cols]))
        _check(f"{form} {dt}: codes by column", oc, woc, _int8_detail(x.float().numpy(), lambda i: csn[i % cols]))


@pytest.mark.parametrize("dt", DTS)
def test_colrow_and_sparse_coo(dt):
    """quantize_colrow's vector and scalar forms (s = sqrt(rm cm)) and quantize_sparse_coo (v / (max / 127)) against the chains of
    tests/int8_decomp_emul.py, exactly."""
    m = rc.colrow_matrix(dt)
    wide = np.zeros((m.shape[0], (m.shape[1] + 7) // 8 * 8), dtype=F32)
    wide[:, :m.shape[1]] = m
    for mat, off, form in ((wide, 0, "colrow_quantize8"), (m, 0, "colrow_quantize1"), (wide, 1, "colrow_quantize1")):
        x = _cpu(mat, dt)
        rm, cm = emul.colrow_stats(x)
        s = emul.colrow_scale(rm, cm)
        want = torch.from_numpy(emul.colrow_codes(x, s))
        q, grm, gcm = F.quantize_colrow(_dev(x, off))
        got = _sparse_native.last_kernel()
        torch.cuda.synchronize()
        assert got == form, f"dispatched {got!r}"
        _check(f"{form} {dt}: row statistics", grm, torch.from_numpy(rm))
        _check(f"{form} {dt}: column statistics", gcm, torch.from_numpy(cm))
        sf = s.reshape(-1)
        _check(f"{form} {dt}: codes", q, want, _int8_detail(x.float().numpy(), lambda i: sf[i]))
    vals = rc.coo_values(dt)
    for row in vals[::64]:
        v = _cpu(row, dt)
        wq, wscale = emul.coo_quantize(v)
        _, _, q, scale = F.quantize_sparse_coo(None, None, _dev(v))
        got = _sparse_native.last_kernel()
        torch.cuda.synchronize()
        assert got == "coo_quantize", got
        _check(f"coo_quantize {dt}: scale", scale, wscale)
        _check(f"coo_quantize {dt}: codes", q, wq)


OUTLIER = [("f16", 0, "regs"), ("bf16", 0, "regs"), ("f32", 0, "two_pass_vec"), ("f32", 1, "two_pass_scalar"), ("f16", 1, "two_pass_scalar")]


@pytest.mark.parametrize("dt,off,quant", OUTLIER, ids=[f"{q}-{d}" for d, _, q in OUTLIER])
def test_outlier_linear_activation_quantiser(dt, off, quant):
    """The row quantiser of outlier_linear, read back from the workspace of the C entry point: the int8 rows and scales of x with the outlier
    columns masked (they hold twice the row's maximum) equal the oracle's quantize_rowwise of the masked x."""
    d = _int8_rows(dt, 1272)
    x = d["x"][::2].copy()
    M, K, N = x.shape[0], x.shape[1], 8
    pos = [K - 1, K - 3]
    x[:, pos] = 2 * x[:, :1]
    c = dict(op="outlier_abi", M=M, N=N, K=K, dt=dt, n_out=len(pos), bias=False, off={"x": off * quant_cases.ESIZE[dt]} if off else {})
    model = nn_cases.model(c)
    assert model[0] == quant, model
    xt = _cpu(x, dt)
    masked = xt.clone()
    masked[:, pos] = 0
    wq, wscales = oracle.quantize_rowwise(masked)
    w = torch.ones(N, K, dtype=torch.int8, device=DEV)
    s = torch.ones(N, dtype=torch.float32, device=DEV)
    oi = torch.tensor(pos, dtype=torch.int64, device=DEV)
    ow = torch.zeros(N, len(pos), dtype=DT[dt], device=DEV)
    y = torch.empty(M, N, dtype=DT[dt], device=DEV)
    nbytes = nn_cases.ws_bytes(c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    xd = _dev(xt, off)
    rcode = _native.lib().mbnb_outlier_linear(_native.ptr(xd), _native.DTYPE_CODE[DT[dt]], M, K, _native.ptr(w), _native.ptr(s), N, _native.ptr(oi), len(pos),
                                             _native.ptr(ow), _native.ptr(None), _native.ptr(y), _native.ptr(ws), nbytes, _native.stream_ptr(torch.device(DEV)))
    assert rcode == 0, _native.lib().mbnb_last_error()
    assert (_native.last_kernel(), _native.last_variant()) == (model[3], model[4])
    torch.cuda.synchronize()
    off_s, _, _ = nn_cases.regions(M, K, len(pos))
    host = ws.cpu()
    _check(f"outlier_linear {quant} {dt}: scales", host[off_s:off_s + 4 * M].view(torch.float32), wscales)
    am = wscales.numpy()
    _check(f"outlier_linear {quant} {dt}: codes", host[:M * K].view(torch.int8), wq, _int8_detail(masked.float().numpy(), lambda i: am[i // K]))


# ----------------------------------------------------------------------------------------------- FP8
FP8_FORMS = [("f32", 2168, 0, "qfp8_row_loop"), ("f32", 2167, 0, "qfp8_row_scalar"), ("f32", 2168, 1, "qfp8_row_scalar"),
             ("f16", 2168, 0, "qfp8_row_loop"), ("bf16", 2168, 0, "qfp8_row_loop"), ("f16", 2168, 1, "qfp8_row_scalar"), ("bf16", 2167, 0, "qfp8_row_scalar")]


@pytest.mark.parametrize("dt,width,off,form", FP8_FORMS, ids=[f"{f[3]}-{f[0]}-{f[1]}+{f[2]}" for f in FP8_FORMS])
def test_fp8_rowwise(dt, width, off, form):
    d = rc.fp8_rows(dt, width=width)
    x = _cpu(d["x"], dt)
    assert _form("quantize_fp8", d["x"].shape, dt, off) == form
    wq, ws = oracle.quantize_fp8_e4m3(x)
    q, s = F.quantize_fp8_e4m3(_dev(x, off))
    got = _native.last_kernel()
    torch.cuda.synchronize()
    assert got == form, f"dispatched {got!r}"
    _check(f"{form} {dt}: scales", s, ws)
    xf = d["x"].reshape(-1)

    def detail(g, w):
        i = int((g != w).nonzero()[0])
        sc = d["s"][i // width]
        n = rc.fp8_quotient(xf[i], sc)
        return f"element {i}: x {_hex(xf[i])} ({xf[i]!r}), scale {_hex(sc)} ({sc!r}), x / scale {_hex(n)} ({n!r}), byte 0x{int(g[i]):02x} for 0x{int(w[i]):02x}"
    _check(f"{form} {dt}: codes", q, wq, detail)
