"""
The kernel routes of libmbnb_train.so (include/mbnb_train.h), one table.  Each case names an op, a shape, a dtype and the name
mbnb_train_last_kernel() must report for it.  Data only, importable without a GPU: tests/test_gpu_switchback.py runs every case and
checks every output element against float64 (tests/elementwise.py); tests/test_switchback_host.py checks that every name the library
can report (its kTrainKernelNames table) is the kernel of some case.

A name hides several pieces of compiled code.  `variant` is the second string the library reports (include/mbnb_train.h: words joined by
blanks, "dq8x4 bias8", "dy1 x8"; "" where the launcher sets none), `model(case)` restates every launcher's conditions in Python and gives
(kernel, variant) -- the GPU runner holds the library's report against it, the host test every case's keys.  THRESHOLDS lists every limit
a launcher compares a size with, each with a predicate per side; LIMIT_CLAIMS maps every literal of the sources' host part to its row or
to ("no case", why); INSTANTIATED the dtypes every form is compiled for; OPERAND_ALIGNMENT_TESTED every pointer a launcher tests.

Keys
  op       forward (functional._switchback_forward), dequant (its Wd pass alone), grad_w (functional._linear_grad_weight),
           transpose (its transposing pass alone)
  M N K    rows (tokens), output columns, input columns; lead: the leading dims of a 3-D input instead of M
  dt       "f16" | "bf16" | "f32";  bias: with a bias;  generic: MBNB_TRAIN_FORCE_GENERIC
  view     "misaligned": the activation (and dY) 2 bytes off 16-byte alignment
  off      {operand: bytes}: that operand starts so many bytes off 256-byte alignment.  Operands the test makes (forward x w bias; dequant w;
           grad_w dy x; transpose x) are copied there; those functional.py allocates (forward out ws; dequant out; grad_w dW ws) are placed
           by the plan of tests/guard.py, so such a case runs under guarded_alloc only
  special  "nonfinite": a NaN, a +Inf and a -Inf in weight_scales and in X
"""


def _c(op, kernel, variant="", **kw):
    kw.update(op=op, kernel=kernel, variant=variant)
    return kw


FORWARD = [
    _c("forward", "switchback_dq+dense", "dq8x4 bias8", M=512, N=3072, K=512, dt="bf16", bias=True),      # 16-byte bias epilogue
    _c("forward", "switchback_dq+dense", "dq8x4 bias1", M=300, N=5003, K=192, dt="f16", bias=True),       # ragged N: scalar bias epilogue
    _c("forward", "switchback_dq+dense", "dq8x4 nobias", M=1024, N=2048, K=1024, dt="f16"),
    _c("forward", "switchback_dq+dense", "dq8x4 bias8", lead=(4, 128), N=4096, K=256, dt="bf16", bias=True),   # 3-D input
    _c("forward", "switchback_dq+dense", "dq8x4 bias8", M=16, N=4096, K=4096, dt="f16", bias=True),
    _c("forward", "switchback_dq+dense", "dq8x1 bias8", M=1, N=16384, K=8192, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=1, N=4096, K=4096, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=1, N=257, K=100, dt="f16"),
    _c("forward", "switchback_generic", M=17, N=100, K=100, dt="f16", bias=True),
    _c("forward", "switchback_generic", M=64, N=256, K=512, dt="f32", bias=True),
    _c("forward", "switchback_generic", M=600, N=3072, K=512, dt="f32"),
    _c("forward", "switchback_generic", lead=(2, 5), N=72, K=136, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=512, N=3072, K=512, dt="f16", bias=True, generic=True),
    _c("forward", "switchback_generic", M=512, N=3072, K=512, dt="bf16", view="misaligned"),
    _c("forward", "switchback_generic", M=512, N=3000, K=500, dt="bf16", bias=True),       # K % 64 != 0
]
DEQUANT = [
    _c("dequant", "switchback_dq", "dq8x4", N=4096, K=4096, dt="f16"),
    _c("dequant", "switchback_dq", "dq8x1", N=11008, K=4096, dt="bf16"),      # more than 2^25 elements: one row per thread
    _c("dequant", "switchback_dq", "dq8x4", N=1000, K=1000, dt="bf16"),
    _c("dequant", "switchback_dq", "dq1", N=77, K=100, dt="f16"),           # K % 8 != 0: the scalar pass
    _c("dequant", "switchback_dq", "dq1", N=33, K=64, dt="f32"),
]
GRAD_W = [
    _c("grad_w", "grad_w_t+dense", "dy8 x8", M=1, N=8192, K=8256, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", "dy8 x8", M=17, N=4096, K=4096, dt="f16"),
    _c("grad_w", "grad_w_t+dense", "dy8 x8", M=100, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", "dy8 x8", M=4095, N=1024, K=2048, dt="f16"),
    _c("grad_w", "grad_w_t+dense", "dy8 x8", M=4096, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", "dy1 x1", M=333, N=1001, K=1537, dt="f16"),                 # ragged N and K: 2-byte loads
    _c("grad_w", "grad_w_t+dense", "dy1 x1", lead=(3, 70), N=2048, K=1024, dt="bf16", view="misaligned"),
    _c("grad_w", "grad_w_generic", M=1, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_generic", M=17, N=1024, K=2048, dt="f16"),
    _c("grad_w", "grad_w_generic", M=100, N=256, K=512, dt="f32"),
    _c("grad_w", "grad_w_generic", M=7, N=40, K=100, dt="f16"),
    _c("grad_w", "grad_w_generic", M=1, N=96, K=64, dt="bf16"),
    _c("grad_w", "grad_w_generic", M=333, N=512, K=4096, dt="bf16", generic=True),
]
TRANSPOSE = [
    _c("transpose", "grad_w_t", "x8", M=4096, K=4096, dt="bf16"),
    _c("transpose", "grad_w_t", "x8", M=1, K=1024, dt="f16"),
    _c("transpose", "grad_w_t", "x1", M=100, K=1537, dt="f16"),            # ragged: 2-byte loads, 36 zero columns
    _c("transpose", "grad_w_t", "x8", M=4095, K=72, dt="bf16"),
]

# ----------------------------------------------------------------------------- forms and limits behind the names
_DENSE, _GEN, _DQ, _GWD, _GWG, _GWT = "switchback_dq+dense", "switchback_generic", "switchback_dq", "grad_w_t+dense", "grad_w_generic", "grad_w_t"
DEQUANT_FORMS = [
    # N K <= 2^25: four rows per thread | one
    _c("dequant", _DQ, "dq8x4", N=8192, K=4096, dt="bf16"), _c("dequant", _DQ, "dq8x1", N=8196, K=4096, dt="bf16"),
    _c("dequant", _DQ, "dq8x4", N=8192, K=4096, dt="f16"), _c("dequant", _DQ, "dq8x1", N=8196, K=4096, dt="f16"),
    # (N + 3) / 4 <= 65535 grid rows: past it N > 65535 too, and a 16-bit aligned weight takes the scalar kernel
    _c("dequant", _DQ, "dq8x4", N=262140, K=64, dt="bf16"), _c("dequant", _DQ, "dq1", N=262144, K=64, dt="bf16"),
    _c("dequant", _DQ, "dq8x4", N=262140, K=64, dt="f16"), _c("dequant", _DQ, "dq1", N=262144, K=64, dt="f16"),
    # N <= 65535 grid rows of the one-row form
    _c("dequant", _DQ, "dq8x1", N=65535, K=520, dt="bf16"), _c("dequant", _DQ, "dq1", N=65536, K=520, dt="bf16"),
    _c("dequant", _DQ, "dq8x1", N=65535, K=520, dt="f16"), _c("dequant", _DQ, "dq1", N=65536, K=520, dt="f16"),
    # the scalar form past its first workgroup: f32, and K % 8 != 0 in both 16-bit dtypes
    _c("dequant", _DQ, "dq1", N=300, K=72, dt="f32"), _c("dequant", _DQ, "dq1", N=300, K=100, dt="bf16"), _c("dequant", _DQ, "dq1", N=300, K=100, dt="f16"),
    # each pointer the pass tests, against the aligned call
    _c("dequant", _DQ, "dq8x4", N=300, K=72, dt="bf16"),
    _c("dequant", _DQ, "dq1", N=300, K=72, dt="bf16", off={"w": 1}), _c("dequant", _DQ, "dq1", N=300, K=72, dt="bf16", off={"out": 2}),
    _c("dequant", _DQ, "dq8x4", N=300, K=72, dt="f16", special="nonfinite"), _c("dequant", _DQ, "dq1", N=300, K=100, dt="f32", special="nonfinite"),
]
FORWARD_FORMS = [
    _c("forward", _DENSE, "dq8x4 bias8", M=32, N=2048, K=2048, dt="bf16", bias=True),             # M N K = 2^27
    _c("forward", _GEN, M=31, N=2048, K=2048, dt="bf16", bias=True),
    _c("forward", _GEN, M=15, N=4096, K=4096, dt="f16", bias=True),                                # against M = 16 above
    _c("forward", _DENSE, "dq8x4 nobias", M=4, N=8192, K=4096, dt="bf16"),                          # N K = 2^25 below M = 16
    _c("forward", _GEN, M=4, N=8192, K=4032, dt="bf16"),                                            # 2^25 - 64 N (and a product below 2^27)
    _c("forward", _DENSE, "dq8x4 bias8", M=8, N=8192, K=4096, dt="f16", bias=True),
    _c("forward", _GEN, M=8, N=8192, K=4032, dt="f16", bias=True),                                  # the weight's size alone decides
    _c("forward", _GEN, M=512, N=4096, K=64, dt="f16", bias=True),
    _c("forward", _DENSE, "dq8x4 bias8", M=512, N=4096, K=128, dt="f16", bias=True),
    _c("forward", _DENSE, "dq8x4 bias8", M=512, N=4096, K=192, dt="f16", bias=True),
    # each pointer the launcher tests, against M=512 N=3072 K=512 bf16 bias above
    _c("forward", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"x": 2}),
    _c("forward", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"w": 4}),
    _c("forward", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"out": 2}),
    _c("forward", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"ws": 8}),
    _c("forward", _DENSE, "dq8x4 bias1", M=512, N=3072, K=512, dt="bf16", bias=True, off={"bias": 2}),      # the scalar bias pass through a misaligned bias
    _c("forward", _GEN, M=17, N=100, K=100, dt="f16", bias=True, special="nonfinite"),
    _c("forward", _GEN, M=10, N=72, K=136, dt="f32", bias=True, special="nonfinite"),
]
GRAD_W_FORMS = [
    _c("grad_w", _GWG, M=64, N=1024, K=1024, dt="bf16"),                    # M N K = 2^26 exactly: not above it
    _c("grad_w", _GWD, "dy8 x8", M=65, N=1024, K=1024, dt="bf16"),
    # padded_rows: 64 | 65 and 127 | 128 | 129 tokens
    _c("grad_w", _GWD, "dy8 x8", M=64, N=1024, K=2048, dt="f16"), _c("grad_w", _GWD, "dy8 x8", M=65, N=1024, K=2048, dt="f16"),
    _c("grad_w", _GWD, "dy8 x8", M=127, N=1024, K=2048, dt="bf16"), _c("grad_w", _GWD, "dy8 x8", M=128, N=1024, K=2048, dt="bf16"),
    _c("grad_w", _GWD, "dy8 x8", M=129, N=1024, K=2048, dt="bf16"),
    # each operand alone
    _c("grad_w", _GWD, "dy1 x8", M=129, N=1024, K=2048, dt="bf16", off={"dy": 2}), _c("grad_w", _GWD, "dy8 x1", M=129, N=1024, K=2048, dt="bf16", off={"x": 2}),
    _c("grad_w", _GWG, M=129, N=1024, K=2048, dt="bf16", off={"dW": 2}), _c("grad_w", _GWG, M=129, N=1024, K=2048, dt="bf16", off={"ws": 8}),
    _c("grad_w", _GWD, "dy1 x8", M=100, N=1004, K=2048, dt="f16"), _c("grad_w", _GWD, "dy8 x1", M=100, N=1024, K=2044, dt="f16"),
]
TRANSPOSE_FORMS = [
    _c("transpose", _GWT, "x8", M=100, K=8, dt="bf16"), _c("transpose", _GWT, "x1", M=100, K=9, dt="bf16"),
    _c("transpose", _GWT, "x8", M=100, K=64, dt="f16"), _c("transpose", _GWT, "x1", M=100, K=65, dt="f16"),         # one | two column blocks of a lane group
    _c("transpose", _GWT, "x8", M=100, K=256, dt="bf16"), _c("transpose", _GWT, "x8", M=100, K=264, dt="bf16"),     # one | two workgroups along c
    _c("transpose", _GWT, "x1", M=100, K=264, dt="bf16", off={"x": 2}),
    _c("transpose", _GWT, "x8", M=64, K=72, dt="f16"), _c("transpose", _GWT, "x8", M=65, K=72, dt="f16"),
    _c("transpose", _GWT, "x8", M=127, K=72, dt="f16"), _c("transpose", _GWT, "x8", M=128, K=72, dt="f16"), _c("transpose", _GWT, "x8", M=129, K=72, dt="f16"),
]
FORMS = DEQUANT_FORMS + FORWARD_FORMS + GRAD_W_FORMS + TRANSPOSE_FORMS
CASES = FORWARD + DEQUANT + GRAD_W + TRANSPOSE + FORMS
PLAN_OPERANDS = {"forward": ("out", "ws"), "dequant": ("out",), "grad_w": ("dW", "ws"), "transpose": ("out",)}     # functional.py's allocations, in order


def needs_plan(c):
    """An offset on a buffer functional.py allocates itself: reachable through the plan of tests/guard.py only."""
    return any(k in PLAN_OPERANDS[c["op"]] for k in c.get("off", {}))


def launches_gemm(c):
    return c["kernel"].endswith("+dense")


def _off(c, operand):
    """Bytes off alignment of `operand`; the old key view="misaligned" moves the activation and dY by one element."""
    if c.get("view") == "misaligned" and operand in ("x", "dy"):
        return 2
    return c.get("off", {}).get(operand, 0)


offset = _off


def rows_of(c):
    if "lead" in c:
        m = 1
        for v in c["lead"]:
            m *= v
        return m
    return c.get("M", 0)


def padded_rows(M):
    return max(128, -(-M // 64) * 64)


def _wd_form(c, out_off):
    N, K = c["N"], c["K"]
    if c["dt"] != "f32" and K % 8 == 0 and _off(c, "w") % 8 == 0 and out_off % 16 == 0:
        if N * K <= 1 << 25 and (N + 3) // 4 <= 65535:
            return "dq8x4"
        if N <= 65535:
            return "dq8x1"
    return "dq1"


def model(c):
    """(kernel, variant) by the launchers' conditions (train_kernels.hip's host side), restated."""
    op, is16, M = c["op"], c["dt"] != "f32", rows_of(c)
    if op == "dequant":
        return _DQ, _wd_form(c, _off(c, "out"))
    if op == "transpose":
        return _GWT, ("x8" if c["K"] % 8 == 0 and _off(c, "x") % 16 == 0 else "x1")
    N, K = c["N"], c["K"]
    if op == "forward":
        shape = is16 and M > 0 and N > 0 and K % 64 == 0 and K >= 128 and 256 * K * 2 < 1 << 31 and M * N * 4 < 1 << 40 and M * N * K >= 1 << 27 and \
            (M >= 16 or N * K >= 1 << 25)
        ptrs = _off(c, "ws") % 256 == 0 and _off(c, "x") % 16 == 0 and _off(c, "w") % 8 == 0 and _off(c, "out") % 16 == 0
        if not (shape and ptrs) or c.get("generic"):
            return _GEN, ""
        bias = "nobias" if not c.get("bias") else "bias8" if N % 8 == 0 and _off(c, "bias") % 16 == 0 else "bias1"
        return _DENSE, f"{_wd_form(c, 0)} {bias}"
    assert op == "grad_w"
    Mp = padded_rows(M)
    shape = is16 and 256 * Mp * 2 < 1 << 31 and (K + 255) // 256 <= 65535 and (N + 255) // 256 <= 65535 and N * K * 4 < 1 << 40 and M * N * K > 1 << 26
    if not (shape and _off(c, "ws") % 256 == 0 and _off(c, "dW") % 16 == 0) or c.get("generic"):
        return _GWG, ""
    return _GWD, ("dy8" if N % 8 == 0 and _off(c, "dy") % 16 == 0 else "dy1") + " " + ("x8" if K % 8 == 0 and _off(c, "x") % 16 == 0 else "x1")


def derived(c):
    M = rows_of(c)
    return dict(M=M, Mp=padded_rows(M), macs=M * c.get("N", 0) * c["K"], weight=c.get("N", 0) * c["K"])


def _v16(c):
    """A Wd pass that no dtype, shape or pointer keeps from the vector forms: the grid limits alone decide."""
    return c["dt"] != "f32" and c["K"] % 8 == 0 and "off" not in c


THRESHOLDS = [
    ("Wd pass K % 8", ("dequant",), lambda c, d: c["K"] % 8 == 0 and c["dt"] != "f32", lambda c, d: c["K"] % 8 != 0 and c["dt"] != "f32"),
    ("Wd pass N K <= 2^25", ("dequant",), lambda c, d: _v16(c) and d["weight"] == 1 << 25 and c["variant"] == "dq8x4",
     lambda c, d: _v16(c) and (1 << 25) < d["weight"] <= (1 << 25) + 4 * c["K"] and c["variant"] == "dq8x1"),
    ("Wd pass (N + 3) / 4 <= 65535", ("dequant",), lambda c, d: _v16(c) and c["N"] == 4 * 65535 and c["variant"] == "dq8x4",
     lambda c, d: _v16(c) and c["N"] == 4 * 65535 + 4 and d["weight"] <= 1 << 25 and c["variant"] == "dq1"),
    ("Wd pass N <= 65535", ("dequant",), lambda c, d: _v16(c) and c["N"] == 65535 and c["variant"] == "dq8x1",
     lambda c, d: _v16(c) and c["N"] == 65536 and d["weight"] > 1 << 25 and c["variant"] == "dq1"),
    ("bias N % 8", ("forward",), lambda c, d: c["variant"].endswith("bias8"), lambda c, d: c["variant"].endswith("bias1") and c["N"] % 8 != 0),
    ("K % 64", ("forward",), lambda c, d: c["K"] % 64 == 0 and c["kernel"] == _DENSE, lambda c, d: c["K"] % 64 != 0 and c["dt"] != "f32" and d["macs"] >= 1 << 27),
    ("K >= 128", ("forward",), lambda c, d: c["K"] == 64 and d["macs"] >= 1 << 27, lambda c, d: c["K"] == 128 and c["kernel"] == _DENSE),
    ("M N K >= 2^27", ("forward",), lambda c, d: d["macs"] == 1 << 27 and c["kernel"] == _DENSE,
     lambda c, d: (1 << 27) - (1 << 22) <= d["macs"] < 1 << 27 and d["M"] >= 16 and c["K"] % 64 == 0 and c["dt"] != "f32"),
    ("M >= 16", ("forward",), lambda c, d: d["M"] == 16 and d["weight"] < 1 << 25 and c["kernel"] == _DENSE,
     lambda c, d: d["M"] == 15 and d["weight"] < 1 << 25 and d["macs"] >= 1 << 27 and c["kernel"] == _GEN),
    ("N K >= 2^25", ("forward",), lambda c, d: d["M"] < 16 and d["weight"] == 1 << 25 and c["kernel"] == _DENSE,
     lambda c, d: d["M"] < 16 and d["weight"] == (1 << 25) - 64 * c["N"] and d["macs"] >= 1 << 27 and c["kernel"] == _GEN),
    ("dW M N K > 2^26", ("grad_w",), lambda c, d: d["macs"] == 1 << 26 and c["dt"] != "f32" and not c.get("generic") and c["kernel"] == _GWG,
     lambda c, d: (1 << 26) < d["macs"] <= (1 << 26) + c["N"] * c["K"] and c["kernel"] == _GWD),
    ("transpose C % 8", ("transpose",), lambda c, d: c["K"] == 8, lambda c, d: c["K"] == 9),
    ("transpose lane groups C 64|65", ("transpose",), lambda c, d: c["K"] == 64, lambda c, d: c["K"] == 65),
    ("transpose workgroups C 256|264", ("transpose",), lambda c, d: c["K"] == 256, lambda c, d: c["K"] == 264 and "off" not in c),
] + [
    (f"padded_rows M {a}|{b}", ops, lambda c, d, a=a: d["M"] == a and "off" not in c, lambda c, d, b=b: d["M"] == b and "off" not in c)
    for ops in (("grad_w",), ("transpose",)) for a, b in ((64, 65), (127, 128), (128, 129))
]

# Every literal the host side of train_kernels.hip compares with (the scan of tests/test_switchback_host.py): a THRESHOLDS row, a list of
# rows, or ("no case", why).
LIMIT_CLAIMS = {
    "% 8": ["Wd pass K % 8", "bias N % 8", "transpose C % 8"], "% 64": "K % 64", "128": ["K >= 128", "padded_rows M 127|128", "padded_rows M 128|129"],
    "16": "M >= 16", "kSbDenseMacs": "M N K >= 2^27", "kSbBigWeight": "N K >= 2^25", "kGwDenseMacs": "dW M N K > 2^26",
    "1 << 25": "Wd pass N K <= 2^25",
    "65535": ["Wd pass (N + 3) / 4 <= 65535", "Wd pass N <= 65535",
              ("no case", "(K + 255) / 256 <= 65535 and (N + 255) / 256 <= 65535 of the weight gradient: a dimension of 16 M elements")],
    "1 << 31": ("no case", "256 K 2 < 2^31 (256 Mp 2 for dW) needs K or M of 2^22 and more: an operand row of 4 M elements, no shape of the suite's budget"),
    "1 << 40": ("no case", "M N 4 < 2^40 (N K 4 for dW) needs an output of 2^38 elements"),
    "0x7FFFFFFF": ("no case", "2^31 - 1 workgroups: the smallest such launch writes 2^33 elements"),
    "kMaxElems": ("no case", "the argument check of every entry point; held without a GPU by test_argument_errors_return_a_status_before_any_device_access"),
    "2": ("no case", "sizeof(T) == 2: a dtype test, held by INSTANTIATED"),
}
# how often the host side compares with each literal; a new comparison changes a count until its THRESHOLDS row and cases follow
LIMIT_COUNTS = {"% 64": 1, "% 8": 3, "128": 2, "1 << 31": 3, "1 << 40": 2, "kSbDenseMacs": 1, "16": 1, "kSbBigWeight": 1, "2": 3, "1 << 25": 1, "65535": 5,
                "0x7FFFFFFF": 2, "kGwDenseMacs": 1, "kMaxElems": 11}

_ALL, _16 = ("f16", "bf16", "f32"), ("f16", "bf16")
INSTANTIATED = {
    (_DQ, "dq8x4"): _16, (_DQ, "dq8x1"): _16, (_DQ, "dq1"): _ALL, (_DENSE, "dq8x4 bias8"): _16, (_DENSE, "dq8x4 bias1"): _16, (_GEN, ""): _ALL,
    (_GWT, "x8"): _16, (_GWT, "x1"): _16, (_GWD, "dy8 x8"): _16, (_GWD, "dy1 x1"): _16, (_GWG, ""): _ALL,
}

# (function, pointer, bytes) of every aligned() test that picks a form -> (op, the operand of `off`); the host test requires for each a pair
# of cases that differ in that offset alone and take different (kernel, variant).
OPERAND_ALIGNMENT_TESTED = {
    ("sb_pass", "W", 8): ("dequant", "w"), ("sb_pass", "out", 16): ("dequant", "out"),
    ("sb_forward", "ws", 256): ("forward", "ws"), ("sb_forward", "X", 16): ("forward", "x"), ("sb_forward", "W", 8): ("forward", "w"),
    ("sb_forward", "out", 16): ("forward", "out"), ("sb_forward", "bias", 16): ("forward", "bias"),
    ("transpose_pad", "A", 16): ("transpose", "x"), ("gw_dispatch", "ws", 256): ("grad_w", "ws"), ("gw_dispatch", "dW", 16): ("grad_w", "dW"),
}
# operands of the dense weight gradient that reach transpose_pad's test one by one
OPERAND_ALIGNMENT_ALSO = {("grad_w", "dy"), ("grad_w", "x")}


def case_id(c):
    rows = "x".join(map(str, c["lead"])) if "lead" in c else str(c.get("M", ""))
    parts = [c["op"], c["kernel"], rows, str(c.get("N", "")), str(c["K"]), c["dt"]]
    parts += [k for k in ("bias", "generic") if c.get(k)] + ([c["view"]] if "view" in c else [])
    parts += [f"{k}+{v}" for k, v in sorted(c.get("off", {}).items())] + ([c["special"]] if "special" in c else [])
    return "-".join(p for p in parts if p)
