"""
One table of the quantise / dequantise launchers of csrc/quant_kernels.hip.  Each case names an op of the public Python API, a
shape, a dtype and format options, and the FORM (mbnb_last_kernel) its launcher must take.  Data only, importable without a
GPU: tests/test_gpu_quant_forms.py runs every case on guarded allocations (tests/guard.py) under two fills and compares every
output bit for bit with the CPU oracle; tests/test_quant_forms_host.py checks the table against the library's source (every
reported name has a case), against `model_form` below (the launchers' conditions restated over the table's data) and against
THRESHOLDS (a case on each side of every limit a launcher tests).

Keys
  op       quantize_4bit, dequantize_4bit, quantize_blockwise, dequantize_blockwise, quantize_rowwise, dequantize_rowwise,
           quantize_fp8, dequantize_fp8, double_quant, dequant_absmax
  form     the name the launcher reports
  shape    the input's shape: 2-D [rows, cols], or 1-D (quantize_4bit / blockwise: the flat layout, one row)
  dt       the floating dtype of the call "f16" | "bf16" | "f32": the input's for a quantiser, the output's for a dequantiser
  bs qt    blocksize, 4-bit code table ("nf4" | "fp4")
  cs       nested statistics: quantize_4bit(compress_statistics=True), dequantize_4bit with int8 absmax + state2
  given    supplied instead of computed: True (quantize_4bit / quantize_blockwise: absmax), "r" | "c" | "rc" (double_quant: the row /
           column statistics)
  kind     dequant_absmax's code dtype "i8" | "u8" | "f32"
  out      True: the caller passes out= (quantize_4bit: packed, dequantize_4bit: the result), placed by hand at align[...]
  align    {buffer: byte offset modulo 16}; "in" is the op's main input, the others are the op's outputs by the names of BUFFERS
           (the order functional.py allocates them in); a buffer not named sits on a 16-byte boundary
  bad      ((kind, flat index), ...): "nan" | "+inf" | "-inf" planted in the input (quantize_4bit without cs only: a NaN through
           the int8 and FP8 quantisers is platform-defined, DESIGN.md, and a NaN or Inf absmax through compress_statistics'
           int8 quantisation of the absmax -- Inf * (127 / Inf) -- is one)
  large    bytes of device memory the case needs (skipped with that reason when less is free);  slabs: a case past 2^31 elements
           (the oracle checks slabs, the rest is compared on the device with the library's output on row chunks)
  xfail    a known library departure the case exposes (run as a strict xfail)
"""

BUFFERS = {
    "quantize_4bit": ("packed", "absmax"),              # cs: ("packed", "codes", "absmax2")
    "dequantize_4bit": ("out",),
    "quantize_blockwise": ("q", "absmax"),
    "dequantize_blockwise": ("out",),
    "quantize_rowwise": ("q", "scales"),
    "dequantize_rowwise": ("out",),
    "quantize_fp8": ("q", "scales"),
    "dequantize_fp8": ("out",),
    "double_quant": ("col_stats", "row_stats", "out_col", "out_row"),   # minus the supplied statistics
    "dequant_absmax": ("out",),
}
ESIZE = {"f16": 2, "bf16": 2, "f32": 4}
DTS = ("f16", "bf16", "f32")


def buffers(c):
    """The buffers functional.py allocates through torch.empty for the case, in order."""
    op = c["op"]
    if op == "quantize_4bit":
        names = ("packed", "codes", "absmax2") if c.get("cs") else ("packed", "absmax")
        direct = c.get("out") and c.get("align", {}).get("packed", 0) % 4 == 0     # else functional.py quantises into a buffer of its own
        return names[1:] if direct else names
    if op == "dequantize_4bit" and c.get("out"):
        return ()
    if op == "double_quant":
        g = c.get("given", "")
        return tuple(n for n in BUFFERS[op] if not ((n == "col_stats" and "c" in g) or (n == "row_stats" and "r" in g)))
    return BUFFERS[op]


def _c(op, form, shape, dt="f16", **kw):
    kw.update(op=op, form=form, shape=tuple(shape), dt=dt)
    return kw


def case_id(c):
    parts = [c["op"], c["form"], "x".join(str(s) for s in c["shape"]), c["dt"]]
    if "bs" in c:
        parts.append(f"bs{c['bs']}")
    if "qt" in c:
        parts.append(c["qt"])
    if c.get("cs"):
        parts.append("cs")
    if c.get("given"):
        parts.append("given" if c["given"] is True else "given_" + c["given"])
    if "kind" in c:
        parts.append(c["kind"])
    if c.get("out"):
        parts.append("out=")
    for k, v in sorted(c.get("align", {}).items()):
        parts.append(f"{k}+{v}")
    if "bad" in c:
        parts.append("bad_" + "_".join(k.strip("+-") + ("p" if k[0] == "+" else "m" if k[0] == "-" else "") for k, _ in c["bad"]))
    return "-".join(parts)


# ----------------------------------------------------------------------------------------------- what a launcher derives
def padded(cols, bs):
    p = (cols + bs - 1) // bs * bs
    return p + bs if p % 2 else p


def derived(c):
    """rows, cols, numel and the quantities the launchers branch on."""
    shape = c["shape"]
    op, bs = c["op"], c.get("bs", 0)
    numel = 1
    for s in shape:
        numel *= s
    d = {"numel": numel}
    if op in ("quantize_blockwise", "dequantize_blockwise"):
        d.update(rows=1, cols=numel, rem=numel % bs, nblk=(numel + bs - 1) // bs)
    elif len(shape) == 2:
        d.update(rows=shape[0], cols=shape[1])
    else:
        d.update(rows=1, cols=numel)
    if op in ("quantize_4bit", "dequantize_4bit"):
        cp = padded(d["cols"], bs)
        span = max(bs, 512)
        d.update(cols_padded=cp, spans_per_row=(cp + span - 1) // span, ndw=d["rows"] * d["cols"] // 8, rem=d["cols"] % bs,
                 gpr=(d["cols"] + 7) // 8)
    return d


def _al(c, name, mask):
    return c.get("align", {}).get(name, 0) & mask == 0


def _rowwise_q(c, rows, cols, fp8, in_name="in", out_name="q"):
    if fp8:
        return "qfp8_row_loop" if cols % 8 == 0 and _al(c, in_name, 15) and _al(c, out_name, 7) else "qfp8_row_scalar"
    vec = cols % 8 == 0 and _al(c, in_name, 15) and _al(c, out_name, 15)
    if vec and cols <= 8192 and c["dt"] != "f32":
        return "q8_row_regs"
    return "q8_row_loop" if vec else "q8_row_scalar"


def _rowwise_dq(c, rows, cols, fp8):
    p = "dqfp8_" if fp8 else "dq8_"
    return p + ("rows16" if cols % 16 == 0 and _al(c, "in", 15) and _al(c, "out", 15) and 0 < rows < 65536 else "scalar")


def model_form(c):
    """The launchers' conditions (csrc/quant_kernels.hip, host launchers) over the table's data: the form a case must take if the
    table and the source agree.  The host test holds every case's `form` against it; the GPU test holds `form` against the library."""
    op, d, bs = c["op"], derived(c), c.get("bs", 0)
    rows, cols = d["rows"], d["cols"]
    if op == "quantize_4bit":
        if bs < 8:
            return "q4_tiny"
        s = "" if _al(c, "in", 15) and cols % 8 == 0 else "_s"
        if c.get("cs") and not c.get("given") and bs <= 512:
            return "q4_dq" + s
        spr = d["spans_per_row"]
        row_grid = spr >= 4 and (spr + 3) // 4 <= 65535
        if bs > 512:
            return ("q4_big_rows" if row_grid else "q4_big") + s
        if row_grid and spr >= 8:
            return "q4_rows2" + s
        return ("q4_rows" if row_grid else "q4_wave") + s
    if op == "dequantize_4bit":
        if (c["dt"] != "f32" and cols == d["cols_padded"] and cols % 8 == 0 and bs >= 8 and cols % bs == 0 and _al(c, "out", 15)
                and d["ndw"] >= 65536):
            return "dq4_flat"
        s = "" if _al(c, "out", 15) and cols % 8 == 0 else "_s"
        return ("dq4_rows" if d["gpr"] >= 256 and (d["gpr"] + 255) // 256 <= 65535 else "dq4_plain") + s
    if op == "quantize_blockwise":
        if not c.get("given") and d["numel"] > 0 and d["rem"] == 0 and bs >= 64:
            return _rowwise_q(c, d["numel"] // bs, bs, False)
        return "q8_block"
    if op == "dequantize_blockwise":
        if d["numel"] > 0 and d["rem"] == 0 and bs >= 1024 and bs % 16 == 0 and d["numel"] // bs < 65536:
            return _rowwise_dq(c, d["numel"] // bs, bs, False)
        return "dq8_block"
    if op in ("quantize_rowwise", "quantize_fp8"):
        return _rowwise_q(c, rows, cols, op == "quantize_fp8")
    if op in ("dequantize_rowwise", "dequantize_fp8"):
        return _rowwise_dq(c, rows, cols, op == "dequantize_fp8")
    if op == "double_quant":
        g = c.get("given", "")
        stats = {"": "rc", "r": "c", "c": "r", "rc": "given"}[g]      # the statistics the call computes
        vec = cols % 8 == 0 and _al(c, "in", 15) and _al(c, "out_col", 7) and _al(c, "out_row", 7) and (rows + 7) // 8 <= 65535
        return ("dquant8_" if vec else "dquant1_") + stats
    if op == "dequant_absmax":
        return "dequant_absmax_" + c["kind"]
    raise KeyError(op)


# the alignment tests of the launchers: form -> ((the buffer tested, the form taken when it fails), ...).  The test of packed's 4-byte
# alignment in dequantize_4bit's flat form is not listed: the C ABI refuses such a pointer before any launcher sees it, and
# functional.py copies the tensor (cases with align {"in": 1} run that route).
ALIGNMENT_TESTED = {
    "q4_wave": (("in", "q4_wave_s"),), "q4_rows": (("in", "q4_rows_s"),), "q4_rows2": (("in", "q4_rows2_s"),),
    "q4_big": (("in", "q4_big_s"),), "q4_big_rows": (("in", "q4_big_rows_s"),), "q4_dq": (("in", "q4_dq_s"),),
    "dq4_flat": (("out", "dq4_rows_s"),), "dq4_rows": (("out", "dq4_rows_s"),), "dq4_plain": (("out", "dq4_plain_s"),),
    "q8_row_regs": (("in", "q8_row_scalar"), ("q", "q8_row_scalar")),
    "q8_row_loop": (("in", "q8_row_scalar"), ("q", "q8_row_scalar")),
    "qfp8_row_loop": (("in", "qfp8_row_scalar"), ("q", "qfp8_row_scalar")),
    "dq8_rows16": (("in", "dq8_scalar"), ("out", "dq8_scalar")),
    "dqfp8_rows16": (("in", "dqfp8_scalar"), ("out", "dqfp8_scalar")),
    "dquant8_rc": (("in", "dquant1_rc"), ("out_col", "dquant1_rc"), ("out_row", "dquant1_rc")),
}

# the dtypes a form's kernels are instantiated for, where not all three
INSTANTIATED = {"q8_row_regs": ("f16", "bf16"), "dq4_flat": ("f16", "bf16"),
                "dequant_absmax_i8": ("f32",), "dequant_absmax_u8": ("f32",), "dequant_absmax_f32": ("f32",)}

# every limit a launcher tests: (what, ops, predicate of (case, derived) for one side, for the other side); each op needs both sides
THRESHOLDS = [
    ("quantize_rowwise cols <= 8192", ("quantize_rowwise",), lambda c, d: d["cols"] == 8192 and c["dt"] != "f32", lambda c, d: d["cols"] == 8200 and c["dt"] != "f32"),
    ("dequantize_rowwise rows < 65536", ("dequantize_rowwise",), lambda c, d: d["rows"] == 65535, lambda c, d: d["rows"] == 65536),
    ("dequantize_fp8 rows < 65536", ("dequantize_fp8",), lambda c, d: d["rows"] == 65535, lambda c, d: d["rows"] == 65536),
    ("dequantize_blockwise blocks < 65536", ("dequantize_blockwise",), lambda c, d: c["bs"] >= 1024 and d["nblk"] == 65535 and d["rem"] == 0,
     lambda c, d: c["bs"] >= 1024 and d["nblk"] == 65536 and d["rem"] == 0),
    ("dequantize_4bit ndw >= 65536", ("dequantize_4bit",), lambda c, d: d["ndw"] == 65535, lambda c, d: d["ndw"] == 65536),
    ("dequantize_4bit groups per row >= 256", ("dequantize_4bit",), lambda c, d: d["gpr"] == 255, lambda c, d: d["gpr"] == 256),
    ("quantize_4bit blocksize <= 512", ("quantize_4bit",), lambda c, d: c["bs"] == 512, lambda c, d: c["bs"] == 1024),
    ("quantize_4bit blocksize < 8", ("quantize_4bit",), lambda c, d: c["bs"] == 4, lambda c, d: c["bs"] == 8),
    ("quantize_4bit spans_per_row >= 4", ("quantize_4bit",), lambda c, d: d["spans_per_row"] == 3 and c["bs"] <= 512, lambda c, d: d["spans_per_row"] == 4 and c["bs"] <= 512),
    ("quantize_4bit spans_per_row >= 4, big blocks", ("quantize_4bit",), lambda c, d: d["spans_per_row"] == 3 and c["bs"] > 512, lambda c, d: d["spans_per_row"] == 4 and c["bs"] > 512),
    ("quantize_4bit spans_per_row >= 8", ("quantize_4bit",), lambda c, d: d["spans_per_row"] == 7 and c["bs"] <= 512, lambda c, d: d["spans_per_row"] == 8 and c["bs"] <= 512),
    ("quantize_4bit row-grid limit of 65535 * 4 spans", ("quantize_4bit",), lambda c, d: 8 <= d["spans_per_row"] <= 262140, lambda c, d: d["spans_per_row"] > 262140),
    ("quantize_blockwise blocksize >= 64", ("quantize_blockwise",), lambda c, d: c["bs"] == 32 and d["rem"] == 0 and not c.get("given"),
     lambda c, d: c["bs"] == 64 and d["rem"] == 0 and not c.get("given")),
    ("dequantize_blockwise blocksize >= 1024", ("dequantize_blockwise",), lambda c, d: c["bs"] == 1008 and d["rem"] == 0, lambda c, d: c["bs"] == 1024 and d["rem"] == 0),
    ("double_quant rows <= 524280", ("double_quant",), lambda c, d: d["rows"] == 524280, lambda c, d: d["rows"] == 524288),
    ("cols % 8", ("quantize_4bit", "dequantize_4bit", "quantize_rowwise", "quantize_fp8", "double_quant"), lambda c, d: d["cols"] % 8 == 0, lambda c, d: d["cols"] % 8 != 0),
    ("cols % 16", ("dequantize_rowwise", "dequantize_fp8"), lambda c, d: d["cols"] % 16 == 0, lambda c, d: d["cols"] % 16 != 0),
    ("numel % blocksize", ("quantize_blockwise", "dequantize_blockwise"), lambda c, d: d["rem"] == 0, lambda c, d: d["rem"] != 0),
    ("cols % blocksize", ("quantize_4bit", "dequantize_4bit"), lambda c, d: d["rem"] == 0, lambda c, d: d["rem"] != 0),
    ("cols < blocksize", ("quantize_4bit", "dequantize_4bit"), lambda c, d: d["cols"] < c["bs"], lambda c, d: d["cols"] >= c["bs"]),
    ("one row", ("quantize_4bit", "dequantize_4bit", "quantize_rowwise", "quantize_fp8", "dequantize_rowwise", "dequantize_fp8", "double_quant",
                 "dequant_absmax"), lambda c, d: d["rows"] == 1 and d["numel"] > 1, lambda c, d: d["rows"] > 1),
    ("one element", ("quantize_4bit", "dequantize_4bit", "quantize_blockwise", "quantize_rowwise", "quantize_fp8", "dequantize_rowwise", "dequantize_fp8",
                     "dequantize_blockwise", "double_quant", "dequant_absmax"), lambda c, d: d["numel"] == 1, lambda c, d: d["numel"] > 1),
]

NAN_INF = (("nan", 3), ("+inf", 1030), ("-inf", 2077))     # three different blocks at every blocksize <= 1024 of a >= 3072-wide row

CASES = []

# ----------------------------------------------------------------------------------------------- quantize_4bit
for dt in DTS:
    CASES += [
        # tiny: one thread per output byte; odd cols (blocksize 1: the padded row has cols + 1 values)
        _c("quantize_4bit", "q4_tiny", (3, 37), dt, bs=1, qt="nf4"),
        _c("quantize_4bit", "q4_tiny", (5, 33), dt, bs=2, qt="fp4"),
        _c("quantize_4bit", "q4_tiny", (7, 45), dt, bs=4, qt="nf4"),
        # flat wave index: fewer than 4 spans of 512 per row
        _c("quantize_4bit", "q4_wave", (9, 1536), dt, bs=64, qt="nf4"),            # 3 spans
        _c("quantize_4bit", "q4_wave_s", (9, 1100), dt, bs=64, qt="fp4"),          # cols % 8, cols % blocksize
        _c("quantize_4bit", "q4_rows", (5, 2048), dt, bs=64, qt="nf4"),            # 4 spans
        _c("quantize_4bit", "q4_rows_s", (5, 3581), dt, bs=128, qt="nf4"),         # 7 spans, odd cols
        _c("quantize_4bit", "q4_rows2", (3, 4096), dt, bs=512, qt="fp4"),          # 8 spans
        _c("quantize_4bit", "q4_rows2_s", (3, 4611), dt, bs=32, qt="nf4"),
        _c("quantize_4bit", "q4_big", (6, 3072), dt, bs=1024, qt="nf4"),           # 3 spans of 1024
        _c("quantize_4bit", "q4_big_s", (2, 5001), dt, bs=4096, qt="fp4"),
        _c("quantize_4bit", "q4_big_rows", (3, 4096), dt, bs=1024, qt="nf4"),      # 4 spans of 1024
        _c("quantize_4bit", "q4_big_rows_s", (2, 9001), dt, bs=2048, qt="nf4"),
        _c("quantize_4bit", "q4_dq", (40, 1024), dt, bs=64, qt="nf4", cs=True),    # 640 blocks: 2.5 groups of 256
        _c("quantize_4bit", "q4_dq_s", (7, 333), dt, bs=32, qt="fp4", cs=True),
    ]
CASES += [
    _c("quantize_4bit", "q4_wave", (1, 512), "f16", bs=8, qt="nf4"),               # one row; blocksize 8: a team of one lane
    _c("quantize_4bit", "q4_wave_s", (1,), "bf16", bs=64, qt="nf4"),               # one element
    _c("quantize_4bit", "q4_wave", (4, 40), "f16", bs=64, qt="fp4"),               # cols < blocksize: 16-byte loads up to cols, zeros beyond
    _c("quantize_4bit", "q4_rows", (3000,), "f16", bs=64, qt="nf4"),               # flat layout: one row of 6 spans, 3000 % 64 != 0
    _c("quantize_4bit", "q4_rows", (2, 3584), "bf16", bs=256, qt="fp4"),           # 7 spans
    _c("quantize_4bit", "q4_dq", (1, 1 << 16), "bf16", bs=512, qt="nf4", cs=True),
    _c("quantize_4bit", "q4_tiny", (2, 8), "f16", bs=4, qt="fp4", given=True),
    # supplied absmax, every form
    _c("quantize_4bit", "q4_wave", (9, 1536), "f16", bs=64, qt="nf4", given=True),
    _c("quantize_4bit", "q4_rows", (5, 2048), "bf16", bs=128, qt="fp4", given=True),
    _c("quantize_4bit", "q4_rows2", (3, 4096), "f32", bs=64, qt="nf4", given=True),
    _c("quantize_4bit", "q4_big", (6, 3072), "f16", bs=1024, qt="nf4", given=True),
    _c("quantize_4bit", "q4_big_rows", (3, 4096), "bf16", bs=1024, qt="fp4", given=True),
    # a caller's out= for packed (the direct path), aligned and one byte off (functional.py then quantises into a buffer of its own)
    _c("quantize_4bit", "q4_rows", (5, 2048), "f16", bs=64, qt="nf4", out=True),
    _c("quantize_4bit", "q4_rows", (5, 2048), "f16", bs=64, qt="nf4", out=True, align={"packed": 1}),
    _c("quantize_4bit", "q4_wave", (9, 1536), "f16", bs=64, qt="nf4", out=True, align={"packed": 4, "absmax": 4}),
    _c("quantize_4bit", "q4_dq", (40, 1024), "bf16", bs=64, qt="nf4", cs=True, align={"packed": 4, "codes": 1, "absmax2": 12}),
    _c("quantize_4bit", "q4_tiny", (3, 37), "f16", bs=1, qt="nf4", align={"in": 2, "packed": 4, "absmax": 8}),
    # misaligned input: the 2- / 4-byte loads
    _c("quantize_4bit", "q4_wave_s", (9, 1536), "f16", bs=64, qt="nf4", align={"in": 2}),
    _c("quantize_4bit", "q4_rows_s", (5, 2048), "bf16", bs=64, qt="nf4", align={"in": 2}),
    _c("quantize_4bit", "q4_rows2_s", (3, 4096), "f32", bs=512, qt="fp4", align={"in": 4}),
    _c("quantize_4bit", "q4_rows2_s", (3, 4096), "f16", bs=512, qt="fp4", align={"in": 8}),
    _c("quantize_4bit", "q4_big_s", (6, 3072), "f16", bs=1024, qt="nf4", align={"in": 2}),
    _c("quantize_4bit", "q4_big_rows_s", (3, 4096), "bf16", bs=1024, qt="nf4", align={"in": 14}),
    _c("quantize_4bit", "q4_dq_s", (40, 1024), "f16", bs=64, qt="nf4", cs=True, align={"in": 2}),
    # NaN, +Inf and -Inf inside a block, every form
    _c("quantize_4bit", "q4_tiny", (2, 4001), "f16", bs=1, qt="nf4", bad=NAN_INF),
    _c("quantize_4bit", "q4_tiny", (2, 4001), "bf16", bs=2, qt="fp4", bad=NAN_INF),
    _c("quantize_4bit", "q4_tiny", (2, 4000), "f32", bs=4, qt="nf4", bad=NAN_INF),
    _c("quantize_4bit", "q4_wave", (2, 1536), "f16", bs=64, qt="nf4", bad=(("nan", 3), ("+inf", 530), ("-inf", 1077))),
    _c("quantize_4bit", "q4_wave_s", (2, 1533), "bf16", bs=8, qt="fp4", bad=(("nan", 3), ("+inf", 530), ("-inf", 1077))),
    _c("quantize_4bit", "q4_rows", (2, 3072), "f16", bs=512, qt="nf4", bad=NAN_INF),
    _c("quantize_4bit", "q4_rows2", (2, 4096), "bf16", bs=64, qt="fp4", bad=NAN_INF),
    _c("quantize_4bit", "q4_big", (2, 3072), "f16", bs=1024, qt="nf4", bad=NAN_INF),
    _c("quantize_4bit", "q4_big_rows", (2, 8192), "f32", bs=2048, qt="fp4", bad=(("nan", 3), ("+inf", 2100), ("-inf", 5000))),
    _c("quantize_4bit", "q4_rows", (2, 3072), "f16", bs=64, qt="nf4", given=True, bad=NAN_INF),
    _c("quantize_4bit", "q4_big", (2, 3072), "bf16", bs=1024, qt="fp4", given=True, bad=NAN_INF),
    _c("quantize_4bit", "q4_tiny", (2, 4000), "f16", bs=4, qt="nf4", given=True, bad=NAN_INF),
    # 2^28 values in one row: 524288 spans, past the row-grid's 65535 * 4
    _c("quantize_4bit", "q4_wave", (1 << 28,), "bf16", bs=64, qt="nf4", large=3 << 30),
]

# ----------------------------------------------------------------------------------------------- dequantize_4bit
for dt in DTS:
    CASES += [
        _c("dequantize_4bit", "dq4_plain", (9, 1536), dt, bs=64, qt="nf4"),
        _c("dequantize_4bit", "dq4_plain_s", (9, 1100), dt, bs=64, qt="fp4"),           # the byte-wise reads of a padded row
        _c("dequantize_4bit", "dq4_plain", (6, 2040), dt, bs=8, qt="nf4", cs=True),     # 255 groups of 8 per row
        _c("dequantize_4bit", "dq4_rows", (6, 2048), dt, bs=64, qt="nf4"),              # 256 groups
        _c("dequantize_4bit", "dq4_rows_s", (5, 3581), dt, bs=128, qt="fp4", cs=True),
        _c("dequantize_4bit", "dq4_plain", (3, 40), dt, bs=4, qt="nf4"),                # blocksize < 8: an absmax per value
    ]
for dt in ("f16", "bf16"):
    CASES += [
        _c("dequantize_4bit", "dq4_flat", (65536, 8), dt, bs=8, qt="nf4"),              # ndw = 65536
        _c("dequantize_4bit", "dq4_plain", (65535, 8), dt, bs=8, qt="nf4"),             # ndw = 65535
        _c("dequantize_4bit", "dq4_flat", (300, 2048), dt, bs=128, qt="fp4", cs=True),
        _c("dequantize_4bit", "dq4_rows_s", (300, 2048), dt, bs=128, qt="fp4", out=True, align={"out": 2}),   # flat but for the alignment
    ]
CASES += [
    _c("dequantize_4bit", "dq4_rows", (300, 2048), "f32", bs=128, qt="fp4"),            # flat but for the dtype
    _c("dequantize_4bit", "dq4_rows", (300, 2080), "f16", bs=64, qt="nf4"),             # flat but for cols % blocksize
    _c("dequantize_4bit", "dq4_flat", (300, 2048), "f16", bs=64, qt="nf4", out=True),   # the direct path, aligned
    _c("dequantize_4bit", "dq4_flat", (300, 2048), "bf16", bs=64, qt="nf4", align={"in": 1}),   # packed one byte off: copied, functional.py
    _c("dequantize_4bit", "dq4_plain", (9, 1536), "f16", bs=64, qt="nf4", align={"in": 1}),
    _c("dequantize_4bit", "dq4_flat", (300, 2048), "bf16", bs=64, qt="nf4", align={"in": 4}),
    _c("dequantize_4bit", "dq4_rows_s", (6, 2048), "f16", bs=64, qt="nf4", out=True, align={"out": 2}),
    _c("dequantize_4bit", "dq4_rows_s", (6, 2048), "f32", bs=64, qt="nf4", out=True, align={"out": 4}),
    _c("dequantize_4bit", "dq4_plain_s", (9, 1536), "bf16", bs=64, qt="nf4", out=True, align={"out": 2}),
    _c("dequantize_4bit", "dq4_plain_s", (9, 1536), "f32", bs=64, qt="nf4", out=True, align={"out": 8}),
    _c("dequantize_4bit", "dq4_plain", (1, 64), "f16", bs=64, qt="nf4"),                # one row
    _c("dequantize_4bit", "dq4_plain_s", (2, 20), "f16", bs=64, qt="nf4"),              # cols < blocksize
    _c("dequantize_4bit", "dq4_plain_s", (1, 1), "bf16", bs=64, qt="fp4"),              # one element
]

# ----------------------------------------------------------------------------------------------- blockwise int8
for dt in DTS:
    r = "q8_row_loop" if dt == "f32" else "q8_row_regs"
    CASES += [
        _c("quantize_blockwise", "q8_block", (64, 100), dt, bs=32),
        _c("quantize_blockwise", r, (64, 100), dt, bs=64),
        _c("quantize_blockwise", "q8_block", (5000,), dt, bs=4096),                     # a partial last block
        _c("quantize_blockwise", "q8_block", (4, 4096), dt, bs=4096, given=True),
        _c("quantize_blockwise", "q8_row_loop", (3, 16384), dt, bs=16384),
        _c("quantize_blockwise", "q8_row_scalar", (3, 4100), dt, bs=4100),              # blocksize % 8
        _c("dequantize_blockwise", "dq8_block", (16, 1008), dt, bs=1008),
        _c("dequantize_blockwise", "dq8_rows16", (16, 1024), dt, bs=1024),
        _c("dequantize_blockwise", "dq8_block", (5000,), dt, bs=4096),
        _c("dequantize_blockwise", "dq8_block", (640,), dt, bs=64),
        _c("dequantize_blockwise", "dq8_block", (3, 1032), dt, bs=1032),                # blocksize % 16
    ]
CASES += [
    _c("quantize_blockwise", "q8_block", (1,), "f16", bs=64),
    _c("quantize_blockwise", "q8_row_scalar", (64, 100), "f16", bs=64, align={"in": 2}),
    _c("quantize_blockwise", "q8_row_scalar", (64, 100), "bf16", bs=64, align={"q": 8}),
    _c("quantize_blockwise", "q8_block", (64, 100), "f16", bs=32, align={"in": 2, "q": 1, "absmax": 4}),
    _c("dequantize_blockwise", "dq8_block", (1,), "f16", bs=4096),
    _c("dequantize_blockwise", "dq8_scalar", (16, 1024), "f16", bs=1024, align={"in": 8}),
    _c("dequantize_blockwise", "dq8_scalar", (16, 1024), "bf16", bs=1024, align={"out": 8}),
    _c("dequantize_blockwise", "dq8_block", (16, 1008), "f16", bs=1008, align={"in": 1, "out": 2}),
    _c("dequantize_blockwise", "dq8_rows16", (65535, 1024), "f16", bs=1024, large=1 << 30),
    _c("dequantize_blockwise", "dq8_block", (65536, 1024), "f16", bs=1024, large=1 << 30),
]

# ----------------------------------------------------------------------------------------------- rowwise int8 / FP8
for dt in DTS:
    r = "q8_row_loop" if dt == "f32" else "q8_row_regs"
    CASES += [
        _c("quantize_rowwise", r, (5, 8192), dt),
        _c("quantize_rowwise", "q8_row_loop", (5, 8200), dt),
        _c("quantize_rowwise", r, (33, 264), dt),                                        # 33 pieces of 16 bytes: a partial wave
        _c("quantize_rowwise", "q8_row_scalar", (7, 1001), dt),
        _c("quantize_fp8", "qfp8_row_loop", (5, 8200), dt),
        _c("quantize_fp8", "qfp8_row_loop", (33, 264), dt),
        _c("quantize_fp8", "qfp8_row_scalar", (7, 1001), dt),
        _c("dequantize_rowwise", "dq8_rows16", (33, 4112), dt),                          # 257 groups of 16: two grid columns
        _c("dequantize_rowwise", "dq8_scalar", (7, 1001), dt),
        _c("dequantize_rowwise", "dq8_scalar", (7, 1016), dt),                           # cols % 8 == 0, % 16 != 0
        _c("dequantize_fp8", "dqfp8_rows16", (33, 4112), dt),
        _c("dequantize_fp8", "dqfp8_scalar", (7, 1001), dt),
    ]
CASES += [
    _c("quantize_rowwise", "q8_row_regs", (1, 64), "f16"), _c("quantize_rowwise", "q8_row_scalar", (1, 1), "f16"),
    _c("quantize_fp8", "qfp8_row_loop", (1, 64), "f16"), _c("quantize_fp8", "qfp8_row_scalar", (1, 1), "bf16"),
    _c("dequantize_rowwise", "dq8_rows16", (1, 64), "f16"), _c("dequantize_rowwise", "dq8_scalar", (1, 1), "f16"),
    _c("dequantize_fp8", "dqfp8_rows16", (1, 64), "f16"), _c("dequantize_fp8", "dqfp8_scalar", (1, 1), "f16"),
    _c("dequantize_rowwise", "dq8_rows16", (65535, 16), "f16"), _c("dequantize_rowwise", "dq8_scalar", (65536, 16), "f16"),
    _c("dequantize_fp8", "dqfp8_rows16", (65535, 16), "bf16"), _c("dequantize_fp8", "dqfp8_scalar", (65536, 16), "bf16"),
    _c("quantize_rowwise", "q8_row_regs", (70000, 8), "bf16"),                          # more rows than a grid's y would hold
    # misaligned
    _c("quantize_rowwise", "q8_row_scalar", (5, 8192), "f16", align={"in": 2}),
    _c("quantize_rowwise", "q8_row_scalar", (5, 8192), "bf16", align={"q": 8}),
    _c("quantize_rowwise", "q8_row_scalar", (5, 8200), "f32", align={"in": 8}),
    _c("quantize_rowwise", "q8_row_scalar", (5, 8200), "f16", align={"q": 8, "scales": 4}),
    _c("quantize_fp8", "qfp8_row_scalar", (5, 8200), "f16", align={"in": 2}),
    _c("quantize_fp8", "qfp8_row_scalar", (5, 8200), "bf16", align={"q": 4}),
    _c("quantize_fp8", "qfp8_row_loop", (5, 8200), "f32", align={"q": 8, "scales": 12}),   # 8-byte stores: 8 passes the test
    _c("dequantize_rowwise", "dq8_scalar", (33, 4112), "f16", align={"in": 8}),
    _c("dequantize_rowwise", "dq8_scalar", (33, 4112), "bf16", align={"out": 8}),
    _c("dequantize_rowwise", "dq8_scalar", (33, 4112), "f32", align={"in": 1, "out": 4}),
    _c("dequantize_fp8", "dqfp8_scalar", (33, 4112), "f16", align={"in": 8}),
    _c("dequantize_fp8", "dqfp8_scalar", (33, 4112), "f32", align={"out": 8}),
    # an embedding / LM-head table: past rows16's 65535 grid rows
    _c("dequantize_rowwise", "dq8_scalar", (128256, 4096), "bf16", large=3 << 30),
    _c("dequantize_fp8", "dqfp8_scalar", (128256, 4096), "f16", large=3 << 30),
    _c("dequantize_rowwise", "dq8_scalar", (262144, 64), "f16"),
    _c("dequantize_fp8", "dqfp8_scalar", (262144, 64), "f32"),
]

# ----------------------------------------------------------------------------------------------- double_quant, dequant_absmax
for dt in DTS:
    CASES += [
        _c("double_quant", "dquant8_rc", (300, 520), dt),                                # partial 128 x 128 and 8 x 8 groups
        _c("double_quant", "dquant1_rc", (77, 101), dt),
        _c("double_quant", "dquant8_given", (300, 520), dt, given="rc"),
        _c("double_quant", "dquant1_given", (77, 101), dt, given="rc"),
        _c("double_quant", "dquant8_c", (130, 264), dt, given="r"), _c("double_quant", "dquant8_r", (130, 264), dt, given="c"),
        _c("double_quant", "dquant1_c", (77, 101), dt, given="r"), _c("double_quant", "dquant1_r", (77, 101), dt, given="c"),
    ]
CASES += [
    _c("double_quant", "dquant8_rc", (1, 8), "f16"), _c("double_quant", "dquant1_rc", (1, 1), "f16"),
    _c("double_quant", "dquant8_rc", (524280, 8), "f16"), _c("double_quant", "dquant1_rc", (524288, 8), "f16"),
    _c("double_quant", "dquant1_rc", (300, 520), "f16", align={"in": 2}),
    _c("double_quant", "dquant1_rc", (300, 520), "bf16", align={"out_col": 4}),
    _c("double_quant", "dquant1_rc", (300, 520), "f32", align={"out_row": 4}),
    _c("double_quant", "dquant1_given", (300, 520), "f32", given="rc", align={"in": 8}),
    _c("double_quant", "dquant8_rc", (300, 520), "f16", align={"out_row": 8, "out_col": 8, "row_stats": 4, "col_stats": 12}),
    _c("dequant_absmax", "dequant_absmax_i8", (5, 700), "f32", kind="i8", bs=256),      # 3 scale blocks a row, the last partial
    _c("dequant_absmax", "dequant_absmax_u8", (5, 700), "f32", kind="u8", bs=256, align={"in": 1, "out": 4}),
    _c("dequant_absmax", "dequant_absmax_f32", (700,), "f32", kind="f32", bs=64),
    _c("dequant_absmax", "dequant_absmax_i8", (1,), "f32", kind="i8", bs=256),
]

# ----------------------------------------------------------------------------------------------- past 2^31 elements
# 2^31 + 2^20 elements each; slabs: the oracle checks the first and last rows and those straddling element 2^31 and byte 2^32
_BIG = (1 << 31) + (1 << 20)
CASES += [
    _c("quantize_rowwise", "q8_row_regs", (_BIG // 4096, 4096), "bf16", large=8 << 30, slabs=True),
    _c("quantize_fp8", "qfp8_row_loop", (_BIG // 4096, 4096), "f16", large=8 << 30, slabs=True),
    _c("quantize_blockwise", "q8_row_regs", (_BIG,), "f16", bs=4096, large=8 << 30, slabs=True),
    _c("dequantize_blockwise", "dq8_block", (_BIG,), "bf16", bs=4096, large=8 << 30, slabs=True),
    _c("dequantize_rowwise", "dq8_scalar", (_BIG // 4096, 4096), "f16", large=8 << 30, slabs=True),
    _c("dequantize_fp8", "dqfp8_scalar", (_BIG // 4096, 4096), "bf16", large=8 << 30, slabs=True),
]
