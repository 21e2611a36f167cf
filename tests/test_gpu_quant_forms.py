"""
Every form of the quantise / dequantise launchers (csrc/quant_kernels.hip), bit for bit against the CPU oracle, on guarded buffers.

The cases are the table of tests/quant_cases.py.  Each runs through the public Python API right after a one-row embedding lookup
whose kernel name is known (a launch that sets no name shows up as that name); it must report the case's form, every output --
packed bytes, absmax or its int8 codes and absmax2, int8 / FP8 codes, scales, both int8 copies and both statistics of
double_quant, the dequantised values -- must equal the oracle's at zero tolerance (NaN by position), and no byte of the guard
bands around the input and the outputs may change (tests/guard.py).  Each case runs under two fills, 0xFF and 0x5A: equality
under both proves that every element of an int8 / uint8 / packed output was written.  Inputs, and a caller's out=, are placed by
hand at the byte offset modulo 16 the case gives.

Past 2^31 elements the oracle checks slabs of rows (the first, the last, those straddling element 2^31 -- byte 2^32 of a 16-bit
buffer); every row is compared on the device with the library's own output on chunks of 16384 rows, whose form the table checks
against the oracle at small shapes.
"""
import pytest
import torch

import oracle
from mps_bitsandbytes_amd import _native
from mps_bitsandbytes_amd import functional as F
from tests import quant_cases
from tests.guard import FILLS, guarded_alloc  # noqa: F401  (the fixture, by name)
from tests.quant_cases import buffers, case_id, derived

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
_SENTINEL = {}


def _sentinel():
    """Run a one-row embedding lookup (no case's own kernel) and check its name is the one on record."""
    if not _SENTINEL:
        _SENTINEL["q8"] = torch.ones(4, 64, dtype=torch.int8, device=DEV)
        _SENTINEL["s8"] = torch.ones(4, dtype=torch.float32, device=DEV)
    F.embedding_8bit(torch.zeros(1, dtype=torch.int64, device=DEV), _SENTINEL["q8"], _SENTINEL["s8"])
    assert _native.last_kernel() == "embedding8"


def _same(a, b):
    """Bit-equal, NaN in the same places (payloads and signs of NaN may differ)."""
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(torch.where(nan, 0, a).view(iv), torch.where(nan, 0, b).view(iv))


def _same_on_device(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    nan = torch.isnan(a)
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(nan, torch.isnan(b)) and torch.equal(torch.where(nan, 0, a).contiguous().view(iv), torch.where(nan, 0, b).contiguous().view(iv))


def _first_diff(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    ne = ~((a == b) | (torch.isnan(a) & torch.isnan(b)) if a.dtype.is_floating_point else (a == b))
    idx = ne.nonzero().reshape(-1)
    i = int(idx[0])
    return f"{idx.numel()} of {a.numel()} elements differ, the first at flat index {i}: got {a[i].item()!r}, the oracle has {b[i].item()!r}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _floats(shape, dt, seed, c=None):
    x = torch.randn(*shape, generator=_gen(seed))
    if len(shape) == 2 and shape[0] >= 3 and not (c and "bad" in c):
        x[1] = 0.0                                     # a row / block of zeros: the clamp of the absmax
    x = x.to(dt)
    for kind, i in (c or {}).get("bad", ()):
        x.view(-1)[i] = BAD[kind]
    return x


def _positive(n, seed):
    return torch.rand(n, generator=_gen(seed)) + 0.25


def _inputs(c):
    """The case's operands as CPU tensors."""
    op, shape, dt, d, bs = c["op"], c["shape"], DT[c["dt"]], derived(c), c.get("bs", 0)
    rows, cols = d["rows"], d["cols"]
    ins = {}
    if op == "quantize_4bit":
        ins["x"] = _floats(shape, dt, 101, c)
        if c.get("given"):
            ins["absmax"] = _positive(rows * d["cols_padded"] // bs, 102)
    elif op == "dequantize_4bit":
        nblk = rows * d["cols_padded"] // bs
        ins["packed"] = torch.randint(0, 256, (rows * d["cols_padded"] // 2,), generator=_gen(103), dtype=torch.uint8)
        if c.get("cs"):
            ins["codes"] = torch.randint(-127, 128, (nblk,), generator=_gen(104), dtype=torch.int8)
            ins["absmax2"] = _positive((nblk + 255) // 256, 105)
        else:
            ins["absmax"] = _positive(nblk, 104)
            if nblk >= 3:
                ins["absmax"][nblk // 3] = float("nan")
    elif op == "quantize_blockwise":
        ins["x"] = _floats(shape, dt, 111)
        if c.get("given"):
            ins["absmax"] = _positive(d["nblk"], 112)
    elif op == "dequantize_blockwise":
        ins["q"] = torch.randint(-128, 128, shape, generator=_gen(113), dtype=torch.int8)
        ins["absmax"] = _positive(d["nblk"], 114)
    elif op in ("quantize_rowwise", "quantize_fp8"):
        ins["x"] = _floats(shape, dt, 121)
    elif op == "dequantize_rowwise":
        ins["q"] = torch.randint(-128, 128, shape, generator=_gen(123), dtype=torch.int8)
        ins["scales"] = _positive(rows, 124)
    elif op == "dequantize_fp8":
        ins["q"] = torch.randint(0, 256, shape, generator=_gen(125), dtype=torch.uint8)     # 0x7F / 0xFF, the NaN bytes, included
        ins["scales"] = _positive(rows, 126)
    elif op == "double_quant":
        ins["x"] = _floats(shape, dt, 131)
        g = c.get("given", "")
        if "c" in g:
            ins["col_stats"] = _positive(cols, 132)
        if "r" in g:
            ins["row_stats"] = _positive(rows, 133)
    elif op == "dequant_absmax":
        kind = c["kind"]
        if kind == "i8":
            ins["q"] = torch.randint(-128, 128, shape, generator=_gen(141), dtype=torch.int8)
        elif kind == "u8":
            ins["q"] = torch.randint(0, 256, shape, generator=_gen(141), dtype=torch.uint8)
        else:
            ins["q"] = torch.randn(*shape, generator=_gen(141))
        ins["scales"] = _positive(rows * max(1, cols // bs), 142)      # cols // bs scale blocks: the codes beyond them decode to 0
    return ins


def _expected(c, ins):
    """{output name: the oracle's tensor}."""
    op, shape, dt, bs = c["op"], c["shape"], DT[c["dt"]], c.get("bs", 0)
    if op == "quantize_4bit":
        p, a, st2 = oracle.quantize_4bit(ins["x"], bs, c["qt"], bool(c.get("cs")), ins.get("absmax"))
        return {"packed": p, "codes": a, "absmax2": st2[0]} if c.get("cs") else {"packed": p, "absmax": a}
    if op == "dequantize_4bit":
        st2 = (ins["absmax2"], 256) if c.get("cs") else None
        return {"out": oracle.dequantize_4bit(ins["packed"], ins["codes"] if c.get("cs") else ins["absmax"], shape, bs, c["qt"], dt, st2)}
    if op == "quantize_blockwise":
        q, a = oracle.quantize_blockwise(ins["x"], bs, ins.get("absmax"))
        return {"q": q, "absmax": a}
    if op == "dequantize_blockwise":
        return {"out": oracle.dequantize_blockwise(ins["q"], ins["absmax"], bs, dt)}
    if op == "quantize_rowwise":
        q, s = oracle.quantize_rowwise(ins["x"])
        return {"q": q, "scales": s}
    if op == "quantize_fp8":
        q, s = oracle.quantize_fp8_e4m3(ins["x"])
        return {"q": q, "scales": s}
    if op == "dequantize_rowwise":
        return {"out": oracle.dequantize_rowwise(ins["q"], ins["scales"], dt)}
    if op == "dequantize_fp8":
        return {"out": oracle.dequantize_fp8_e4m3(ins["q"], ins["scales"], dt)}
    if op == "double_quant":
        oc, orow, cs, rs, _ = oracle.double_quant(ins["x"], ins.get("col_stats"), ins.get("row_stats"))
        return {"out_col": oc, "out_row": orow, "col_stats": cs, "row_stats": rs}
    return {"out": oracle.dequant_absmax(ins["q"], ins["scales"], bs)}


def _call(c, g, dev_ins):
    """Run the op on the device through the public API: {output name: tensor}.  `dev_ins`: the operands on the device, the main input
    already placed."""
    op, shape, dt, bs, d = c["op"], c["shape"], DT[c["dt"]], c.get("bs", 0), derived(c)
    al = c.get("align", {})
    if op == "quantize_4bit":
        out = None
        if c.get("out"):
            out = g.place_empty("packed", (d["rows"] * d["cols_padded"] // 2,), torch.uint8, DEV, al.get("packed", 0))
        packed, st = F.quantize_4bit(dev_ins["x"], absmax=dev_ins.get("absmax"), out=out, blocksize=bs, compress_statistics=bool(c.get("cs")),
                                     quant_type=c["qt"])
        if out is not None:
            assert packed.data_ptr() == out.data_ptr(), "out= was not the tensor returned"
            packed = out
        if c.get("cs"):
            assert st.state2 is not None and st.state2.blocksize == 256
            return {"packed": packed, "codes": st.absmax, "absmax2": st.state2.absmax}
        return {"packed": packed, "absmax": st.absmax}
    if op == "dequantize_4bit":
        st2 = None
        if c.get("cs"):
            st2 = F.QuantState(absmax=dev_ins["absmax2"], shape=torch.Size([dev_ins["codes"].numel()]), blocksize=256, quant_type="int8",
                               dtype=torch.float32)
        st = F.QuantState(absmax=dev_ins["codes"] if c.get("cs") else dev_ins["absmax"], shape=torch.Size(shape), blocksize=bs,
                          quant_type=c["qt"], dtype=dt, state2=st2)
        out = g.place_empty("out", shape, dt, DEV, al.get("out", 0)) if c.get("out") else None
        y = F.dequantize_4bit(dev_ins["packed"], st, out=out)
        if out is not None:
            assert y.data_ptr() == out.data_ptr()
        return {"out": y}
    if op == "quantize_blockwise":
        q, st = F.quantize_blockwise(dev_ins["x"], absmax=dev_ins.get("absmax"), blocksize=bs)
        return {"q": q, "absmax": st.absmax}
    if op == "dequantize_blockwise":
        st = F.QuantState(absmax=dev_ins["absmax"], shape=torch.Size(shape), blocksize=bs, quant_type="int8", dtype=dt)
        return {"out": F.dequantize_blockwise(dev_ins["q"], st)}
    if op == "quantize_rowwise":
        q, s = F.quantize_rowwise(dev_ins["x"])
        return {"q": q, "scales": s}
    if op == "quantize_fp8":
        q, s = F.quantize_fp8_e4m3(dev_ins["x"])
        return {"q": q, "scales": s}
    if op == "dequantize_rowwise":
        return {"out": F.dequantize_rowwise(dev_ins["q"], dev_ins["scales"], dt)}
    if op == "dequantize_fp8":
        return {"out": F.dequantize_fp8_e4m3(dev_ins["q"], dev_ins["scales"], dt)}
    if op == "double_quant":
        oc, orow, cs, rs, _ = F.double_quant(dev_ins["x"], dev_ins.get("col_stats"), dev_ins.get("row_stats"))
        return {"out_col": oc, "out_row": orow, "col_stats": cs, "row_stats": rs}
    return {"out": F.dequant_absmax(dev_ins["q"], dev_ins["scales"], bs)}


MAIN = {"quantize_4bit": "x", "dequantize_4bit": "packed", "quantize_blockwise": "x", "dequantize_blockwise": "q", "quantize_rowwise": "x",
        "quantize_fp8": "x", "dequantize_rowwise": "q", "dequantize_fp8": "q", "double_quant": "x", "dequant_absmax": "q"}


def _run_guarded(c, g, fill, dev_src):
    """One guarded run of the case under `fill`: (form, {name: output})."""
    al = c.get("align", {})
    g.begin(fill, (), f"{c['op']} {c['form']} ({case_id(c)})")
    dev_ins = dict(dev_src)
    dev_ins[MAIN[c["op"]]] = g.place("in", dev_src[MAIN[c["op"]]], al.get("in", 0))
    _sentinel()
    # out=: the offset of "packed" / "out" is the caller's buffer's; one functional.py allocates in its place sits on a boundary
    g.plan = [(n, 0 if c.get("out") and n in ("packed", "out") else al.get(n, 0)) for n in buffers(c)]
    outs = _call(c, g, dev_ins)
    assert not g.plan, f"{case_id(c)}: functional.py did not allocate {[n for n, _ in g.plan]} through torch.empty"
    form = _native.last_kernel()
    torch.cuda.synchronize()
    assert form == c["form"], f"{case_id(c)}: dispatched {form!r}, the case is for {c['form']!r}"
    g.check()
    return form, outs


def _need(c):
    if "large" in c:
        free, _ = torch.cuda.mem_get_info()
        if free < c["large"]:
            pytest.skip(f"{case_id(c)} needs {c['large'] >> 20} MiB of device memory, {free >> 20} MiB are free")


def _params(cases):
    return [pytest.param(c, marks=pytest.mark.xfail(strict=True, reason=c["xfail"])) if "xfail" in c else c for c in cases]


SMALL = [c for c in quant_cases.CASES if not c.get("slabs")]
SLABS = [c for c in quant_cases.CASES if c.get("slabs")]


@pytest.mark.parametrize("case", _params(SMALL), ids=[case_id(c) for c in SMALL])
def test_quant_form_bit_for_bit_on_guarded_buffers(case, guarded_alloc):
    c, g = case, guarded_alloc
    _need(c)
    ins = _inputs(c)
    want = _expected(c, ins)
    dev_src = {k: v.to(DEV) for k, v in ins.items()}
    for fill in FILLS:
        _, outs = _run_guarded(c, g, fill, dev_src)
        assert set(outs) == set(want)
        for name, t in outs.items():
            assert _same(t, want[name]), f"{case_id(c)}, fill 0x{fill:02X}: {name} differs from the oracle: {_first_diff(t, want[name])}"
        g.begin(fill)                   # drop the buffers before the next fill's are made
        del outs


# ----------------------------------------------------------------------------------------------------- past 2^31 elements
CHUNK_ROWS = 16384
ORACLE_CHECKED = {c["form"] for c in SMALL if "large" not in c}


def _device_operands(c, rows, cols):
    """The operands of a slab case, generated on the device, as [rows, cols] (+ per-row scales)."""
    dt = DT[c["dt"]]
    gen = torch.Generator(device=DEV).manual_seed(20261017)
    if c["op"].startswith("quantize"):
        x = torch.empty(rows, cols, dtype=dt, device=DEV)
        for r0 in range(0, rows, CHUNK_ROWS):
            r1 = min(rows, r0 + CHUNK_ROWS)
            x[r0:r1] = torch.randn(r1 - r0, cols, generator=gen, device=DEV, dtype=torch.float32).to(dt)
        return x, None
    if c["op"] == "dequantize_fp8":
        q = torch.randint(0, 256, (rows, cols), generator=gen, device=DEV, dtype=torch.uint8)
    else:
        q = torch.randint(-128, 128, (rows, cols), generator=gen, device=DEV, dtype=torch.int8)
    return q, torch.rand(rows, generator=gen, device=DEV) + 0.25


def _rows_call(c, x, s):
    """The case's op on rows [x, s] through the public API: a tuple of outputs shaped [rows, ...]."""
    op, dt = c["op"], DT[c["dt"]]
    rows, cols = x.shape
    if op == "quantize_rowwise":
        return F.quantize_rowwise(x)
    if op == "quantize_fp8":
        return F.quantize_fp8_e4m3(x)
    if op == "quantize_blockwise":
        q, st = F.quantize_blockwise(x.view(-1), blocksize=cols)
        return q.view(rows, cols), st.absmax
    if op == "dequantize_blockwise":
        st = F.QuantState(absmax=s, shape=torch.Size([rows * cols]), blocksize=cols, quant_type="int8", dtype=dt)
        return (F.dequantize_blockwise(x.view(-1), st).view(rows, cols),)
    if op == "dequantize_rowwise":
        return (F.dequantize_rowwise(x, s, dt),)
    return (F.dequantize_fp8_e4m3(x, s, dt),)


def _rows_oracle(c, x, s):
    op, dt = c["op"], DT[c["dt"]]
    rows, cols = x.shape
    if op == "quantize_rowwise":
        return oracle.quantize_rowwise(x)
    if op == "quantize_fp8":
        return oracle.quantize_fp8_e4m3(x)
    if op == "quantize_blockwise":
        q, a = oracle.quantize_blockwise(x.reshape(-1), cols)
        return q.view(rows, cols), a
    if op == "dequantize_blockwise":
        return (oracle.dequantize_blockwise(x.reshape(-1), s, cols, dt).view(rows, cols),)
    if op == "dequantize_rowwise":
        return (oracle.dequantize_rowwise(x, s, dt),)
    return (oracle.dequantize_fp8_e4m3(x, s, dt),)


@pytest.mark.parametrize("case", _params(SLABS), ids=[case_id(c) for c in SLABS])
def test_quant_form_past_two_to_the_31_elements(case, guarded_alloc):
    c, g = case, guarded_alloc
    _need(c)
    numel = derived(c)["numel"]
    cols = c.get("bs") or c["shape"][1]              # blockwise: a row is a block
    rows = numel // cols
    assert numel > 1 << 31 and rows * cols == numel
    x, s = _device_operands(c, rows, cols)
    mid = (1 << 31) // cols
    slabs = [(0, 8), (mid - 4, mid + 4), (rows - 8, rows)]      # element 2^31 is byte 2^32 of the 16-bit buffer; the 8-bit one ends before it
    assert DT[c["dt"]].itemsize == 2
    al = c.get("align", {})
    for fill in FILLS:
        g.begin(fill, (), f"{c['op']} {c['form']} ({case_id(c)})")
        _sentinel()
        g.plan = [(n, al.get(n, 0)) for n in buffers(c)]
        outs = _rows_call(c, x, s)
        form = _native.last_kernel()
        torch.cuda.synchronize()
        assert form == c["form"], f"{case_id(c)}: dispatched {form!r}, the case is for {c['form']!r}"
        g.check()
        for r0, r1 in slabs:
            want = _rows_oracle(c, x[r0:r1].cpu(), None if s is None else s[r0:r1].cpu())
            for k, (a, b) in enumerate(zip(outs, want)):
                assert _same(a[r0:r1], b), f"{case_id(c)}, fill 0x{fill:02X}: output {k}, rows {r0}..{r1}: {_first_diff(a[r0:r1], b)}"
        for r0 in range(0, rows, CHUNK_ROWS):
            r1 = min(rows, r0 + CHUNK_ROWS)
            g.begin(fill)               # the chunk's buffers are guarded too, and dropped chunk by chunk
            part = _rows_call(c, x[r0:r1], None if s is None else s[r0:r1])
            assert _native.last_kernel() in ORACLE_CHECKED, _native.last_kernel()
            g.check()
            for k, (a, b) in enumerate(zip(outs, part)):
                assert _same_on_device(a[r0:r1], b), f"{case_id(c)}, fill 0x{fill:02X}: output {k} differs from the chunked call in rows {r0}..{r1}"
        del outs, part
        g.begin(fill)
