"""
The kernel routes of libmbnb_sparse.so (include/mbnb_sparse.h), one table.  Each case names an op, a shape, a dtype and the name
mbnb_sparse_last_kernel() must report for it.  Data only, importable without a GPU: tests/test_gpu_int8_decomp.py runs every case and
checks every output element (bit for bit against the emulation of tests/int8_decomp_emul.py, or against float64 with the bound of
tests/elementwise.py); tests/test_int8_decomp_host.py checks that every name the library can report (its kSparseKernelNames table) is
the kernel of some case.

A name hides several pieces of compiled code.  `variant` is the second string the library reports (include/mbnb_sparse.h: "wt",
"parts<n>", "G<g> x<t>"; "" where the launcher sets none), `model(case)` restates every launcher's conditions in Python and gives
(kernel, variant) -- the GPU runner holds the library's report against it, the host test every case's keys -- and `derived(case)` the
sizes the kernels branch on (column chunks, row blocks, G, tiles, the scan's share).  THRESHOLDS lists every limit a launcher or a kernel
compares a size with, each with a predicate per side; LIMIT_CLAIMS maps every literal of the sources' host part to its row or to
("no case", why); INSTANTIATED the dtypes every form is compiled for; OPERAND_ALIGNMENT_TESTED every pointer a launcher tests.

Keys
  op       quantize (quantize_colrow), dequant (dequantize_colrow; route "pass": functional._colrow_dequant_pass), matmul (functional._matmul_colrow), count (sparse_coo_from_dense's
           first launch pair, functional._coo_row_ptr), from_dense (sparse_coo_from_dense), quantize_coo (quantize_sparse_coo),
           spmm (functional._spmm_coo)
  R C      rows and columns of the matrix;  M N K: tokens, output columns, input columns of matmul (lead: the leading dims of the
           input instead of M; () is a 1-D input);  rows cols N density: the sparse shape, the dense matrix's width, the share of nonzeros
  dt       "f16" | "bf16" | "f32";  bias: with a bias;  generic: MBNB_SPARSE_FORCE_GENERIC;  view "misaligned": the main operand 2 bytes
           (4 for f32) off 16-byte alignment;  threshold: of from_dense
  index    "sorted" | "permuted" | "int32" | "duplicates";  values: "T" | "int8" | "int8_entry"
  off      {operand: bytes}: that operand starts so many bytes off 256-byte alignment.  Operands the test makes (quantize x; dequant q rm cm;
           matmul x w rm cm bias; spmm row col values dense) are copied there; those functional.py allocates (quantize q rs cs; dequant
           out; matmul out ws; spmm out) are placed by the plan of tests/guard.py, so such a case runs under guarded_alloc only
  special  from_dense "edges": values equal to the rounded threshold, -0.0, NaN, +-Inf;  quantize / dequant / quantize_coo "nonfinite":
           a NaN, a +Inf and a -Inf across chunk and row-block boundaries
"""


def _c(op, kernel, variant="", **kw):
    kw.update(op=op, kernel=kernel, variant=variant)
    return kw


ESIZE = {"f16": 2, "bf16": 2, "f32": 4}
CR_CB, CR_RB, CR_UN, COO_QP, COO_SORT_LDS, SCAN_THREADS = 2048, 16, 4, 1024, 4096, 1024      # sparse_kernels.hip's constants


QUANTIZE = [
    _c("quantize", "colrow_quantize8", R=4096, C=4096, dt="bf16"),
    _c("quantize", "colrow_quantize8", R=4096, C=11008, dt="f16"),
    _c("quantize", "colrow_quantize8", R=1000, C=1000, dt="f32"),
    _c("quantize", "colrow_quantize8", R=33, C=2056, dt="f16"),            # two column chunks, a ragged last row block
    _c("quantize", "colrow_quantize8", R=1, C=4096, dt="bf16"),
    _c("quantize", "colrow_quantize1", R=1001, C=1537, dt="bf16"),         # C % 8 != 0
    _c("quantize", "colrow_quantize1", R=77, C=100, dt="f32"),
    _c("quantize", "colrow_quantize1", R=2500, C=1, dt="f16"),
    _c("quantize", "colrow_quantize1", R=64, C=4096, dt="f16", view="misaligned"),
]
DEQUANT = [
    _c("dequant", "colrow_dequant8", R=4096, C=4096, dt="f16"),
    _c("dequant", "colrow_dequant8", R=11008, C=4096, dt="bf16"),
    _c("dequant", "colrow_dequant8", R=1000, C=1000, dt="f32"),
    _c("dequant", "colrow_dequant1", R=77, C=100, dt="f16"),
    _c("dequant", "colrow_dequant1", R=1001, C=1537, dt="bf16"),
    _c("dequant", "colrow_dequant1", R=33, C=65, dt="f32"),
    # matmul_colrow's pass alone, as its dense route runs it (write-through stores in the 16-bit vector form)
    _c("dequant", "colrow_dequant8", "wt", R=4096, C=4096, dt="bf16", route="pass"),
    _c("dequant", "colrow_dequant8", "wt", R=5003, C=192, dt="f16", route="pass"),
    _c("dequant", "colrow_dequant8", R=1000, C=1000, dt="f32", route="pass"),
    _c("dequant", "colrow_dequant1", R=77, C=100, dt="bf16", route="pass"),
]
MATMUL = [
    _c("matmul", "colrow_dq+dense", "wt", M=512, N=3072, K=512, dt="bf16", bias=True),
    _c("matmul", "colrow_dq+dense", "wt", M=300, N=5003, K=192, dt="f16", bias=True),        # ragged N
    _c("matmul", "colrow_dq+dense", "wt", M=1024, N=2048, K=1024, dt="f16"),
    _c("matmul", "colrow_dq+dense", "wt", lead=(4, 128), N=4096, K=256, dt="bf16", bias=True),
    _c("matmul", "colrow_dq+dense", "wt", M=16, N=4096, K=4096, dt="f16", bias=True),
    _c("matmul", "colrow_generic", M=1, N=4096, K=4096, dt="bf16", bias=True),
    _c("matmul", "colrow_generic", lead=(), N=257, K=100, dt="f16"),                   # 1-D input
    _c("matmul", "colrow_generic", M=17, N=100, K=100, dt="f16", bias=True),
    _c("matmul", "colrow_generic", M=64, N=256, K=512, dt="f32", bias=True),
    _c("matmul", "colrow_generic", M=600, N=3072, K=512, dt="f32"),
    _c("matmul", "colrow_generic", lead=(2, 5), N=72, K=136, dt="bf16", bias=True),
    _c("matmul", "colrow_generic", M=512, N=3072, K=512, dt="f16", bias=True, generic=True),
    _c("matmul", "colrow_generic", M=512, N=3072, K=512, dt="bf16", view="misaligned"),
    _c("matmul", "colrow_generic", M=512, N=3000, K=500, dt="bf16", bias=True),        # K % 64 != 0
]
FROM_DENSE = [
    _c("count", "coo_count", R=1000, C=2000, dt="f32", density=0.05),
    _c("count", "coo_count", R=3, C=70000, dt="f16", density=0.5, threshold=0.3),
    _c("from_dense", "coo_fill", R=1000, C=2000, dt="f32", density=0.05),
    _c("from_dense", "coo_fill", R=4096, C=4096, dt="f16", density=0.05),
    _c("from_dense", "coo_fill", R=4097, C=1001, dt="bf16", density=1.0, threshold=0.5),   # a threshold on a full matrix; more rows than scan threads
    _c("from_dense", "coo_fill", R=3, C=70000, dt="f16", density=0.5, threshold=0.3),
    _c("from_dense", "coo_fill", R=1, C=1, dt="f32", density=1.0),
]
QUANTIZE_COO = [
    _c("quantize_coo", "coo_quantize", "parts49", n=100000, dt="f32"),
    _c("quantize_coo", "coo_quantize", "parts1024", n=5000001, dt="f16"),               # more than the 1024 partial maxima cover in one pass
    _c("quantize_coo", "coo_quantize", "parts1", n=1, dt="bf16"),
    _c("quantize_coo", "coo_quantize", "parts1", n=777, dt="bf16"),
]
SPMM = [
    _c("spmm", "spmm_coo8", "G32 x1", rows=1000, cols=2000, N=256, dt="f16", density=0.05, index="sorted", values="T"),
    _c("spmm", "spmm_coo8", "G64 x1", rows=1000, cols=2000, N=256, dt="f32", density=0.05, index="permuted", values="T"),
    _c("spmm", "spmm_coo8", "G32 x1", rows=1000, cols=2000, N=256, dt="bf16", density=0.05, index="duplicates", values="T"),
    _c("spmm", "spmm_coo8", "G64 x8", rows=512, cols=1024, N=4096, dt="bf16", density=0.02, index="int32", values="T"),     # a whole wave per row, 8 tiles
    _c("spmm", "spmm_coo8", "G16 x1", rows=300, cols=500, N=64, dt="f16", density=0.1, index="permuted", values="int8"),     # 16 lanes per row
    _c("spmm", "spmm_coo8", "G16 x1", rows=300, cols=500, N=72, dt="bf16", density=0.1, index="sorted", values="int8_entry"),
    _c("spmm", "spmm_coo8", "G32 x1", rows=40, cols=9000, N=128, dt="f32", density=0.7, index="permuted", values="T"),       # 6300 entries per row: sorted in global memory
    _c("spmm", "spmm_coo8", "G16 x1", rows=64, cols=64, N=8, dt="f16", density=0.0, index="sorted", values="T"),             # nnz = 0: zeros
    _c("spmm", "spmm_coo1", "G64 x1", rows=1000, cols=2000, N=250, dt="f16", density=0.05, index="permuted", values="T"),    # N * 2 % 16 != 0
    _c("spmm", "spmm_coo1", "G16 x1", rows=77, cols=100, N=3, dt="f32", density=0.2, index="sorted", values="int8"),
    _c("spmm", "spmm_coo1", "G64 x1", rows=200, cols=300, N=256, dt="bf16", density=0.1, index="int32", values="T", view="misaligned"),
    _c("spmm", "spmm_coo8_general", "G32 x1", rows=1000, cols=2000, N=256, dt="f16", density=0.05, index="sorted", values="T", generic=True),
    _c("spmm", "spmm_coo1_general", "G16 x1", rows=77, cols=100, N=3, dt="f32", density=0.2, index="sorted", values="T", generic=True),
]

# ----------------------------------------------------------------------------- forms and limits behind the names
_Q8, _Q1, _DQ8, _DQ1 = "colrow_quantize8", "colrow_quantize1", "colrow_dequant8", "colrow_dequant1"
_DENSE, _GEN = "colrow_dq+dense", "colrow_generic"
QUANTIZE_FORMS = [
    # the scalar forms across column chunks (CR_CB = 2048: three chunks, the partial-merge path), every dtype
    _c("quantize", _Q1, R=37, C=4099, dt="f16"),
    _c("quantize", _Q1, R=37, C=4099, dt="bf16"),
    _c("quantize", _Q1, R=37, C=4099, dt="f32"),
    # each pointer the launcher tests, against the aligned call
    _c("quantize", _Q8, R=37, C=4096, dt="f16"),
    _c("quantize", _Q1, R=37, C=4096, dt="f16", off={"x": 2}),
    _c("quantize", _Q1, R=37, C=4096, dt="f16", off={"cs": 4}),
    _c("quantize", _Q1, R=37, C=4096, dt="f16", off={"q": 4}),
    # k_colrow_merge: nrb = 3 | 4 | 5 partial rows for four waves (a wave without one, waves with one, a wave with two)
    _c("quantize", _Q8, R=48, C=2056, dt="f16"),
    _c("quantize", _Q8, R=49, C=2056, dt="bf16"),
    _c("quantize", _Q8, R=64, C=2056, dt="f32"),
    _c("quantize", _Q8, R=65, C=2056, dt="f16"),
    _c("quantize", _Q8, R=80, C=2056, dt="bf16"),
    # one | two merge workgroups for the columns, one | two for the rows
    _c("quantize", _Q8, R=20, C=64, dt="bf16"),
    _c("quantize", _Q8, R=20, C=72, dt="bf16"),
    _c("quantize", _Q8, R=256, C=72, dt="f16"),
    _c("quantize", _Q8, R=257, C=72, dt="f16"),
    _c("quantize", _Q1, R=256, C=65, dt="f32"),
    _c("quantize", _Q1, R=257, C=65, dt="f32"),
    # a NaN, a +Inf and a -Inf across a chunk and a row-block boundary, scalar and vector
    _c("quantize", _Q1, R=37, C=4099, dt="f16", special="nonfinite"),
    _c("quantize", _Q1, R=37, C=4099, dt="f32", special="nonfinite"),
    _c("quantize", _Q8, R=80, C=2056, dt="bf16", special="nonfinite"),
]
DEQUANT_FORMS = [
    _c("dequant", _DQ1, R=37, C=4099, dt="f16"),
    _c("dequant", _DQ1, R=37, C=4099, dt="bf16"),
    _c("dequant", _DQ1, R=37, C=4099, dt="f32"),
    _c("dequant", _DQ8, R=37, C=4096, dt="bf16"),
    _c("dequant", _DQ1, R=37, C=4096, dt="bf16", off={"q": 4}),
    _c("dequant", _DQ1, R=37, C=4096, dt="bf16", off={"cm": 4}),
    _c("dequant", _DQ1, R=37, C=4096, dt="bf16", off={"out": 2}),
    _c("dequant", _DQ8, R=80, C=2056, dt="f16"),
    _c("dequant", _DQ8, "wt", R=37, C=4096, dt="f16", route="pass"),
    _c("dequant", _DQ1, R=37, C=4096, dt="f16", route="pass", off={"out": 2}),
    _c("dequant", _DQ1, R=37, C=4099, dt="f16", special="nonfinite"),
    _c("dequant", _DQ8, R=80, C=2056, dt="f32", special="nonfinite"),
]
MATMUL_FORMS = [
    # M N K >= 2^27
    _c("matmul", _DENSE, "wt", M=32, N=2048, K=2048, dt="bf16", bias=True),
    _c("matmul", _GEN, M=31, N=2048, K=2048, dt="bf16", bias=True),
    # M >= 16 below N K = 2^25
    _c("matmul", _GEN, M=15, N=4096, K=4096, dt="f16", bias=True),
    # N K >= 2^25 below M = 16: M = 4 (the product falls below 2^27 with it), M = 8 (the weight's size alone decides)
    _c("matmul", _DENSE, "wt", M=4, N=8192, K=4096, dt="bf16"),
    _c("matmul", _GEN, M=4, N=8192, K=4032, dt="bf16"),
    _c("matmul", _DENSE, "wt", M=8, N=8192, K=4096, dt="f16", bias=True),
    _c("matmul", _GEN, M=8, N=8192, K=4032, dt="f16", bias=True),
    # K >= 128
    _c("matmul", _GEN, M=512, N=4096, K=64, dt="f16", bias=True),
    _c("matmul", _DENSE, "wt", M=512, N=4096, K=128, dt="f16", bias=True),
    _c("matmul", _DENSE, "wt", M=512, N=4096, K=192, dt="f16", bias=True),
    # each pointer the launcher tests, against M=512 N=3072 K=512 bf16 bias (dense)
    _c("matmul", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"x": 2}),
    _c("matmul", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"w": 4}),
    _c("matmul", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"cm": 4}),
    _c("matmul", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"out": 2}),
    _c("matmul", _GEN, M=512, N=3072, K=512, dt="bf16", bias=True, off={"ws": 8}),
]
FROM_DENSE_FORMS = [
    _c("from_dense", "coo_fill", R=33, C=64, dt="f16", density=0.3),            # one | two 64-column steps of a wave
    _c("from_dense", "coo_fill", R=33, C=65, dt="f16", density=0.3),
    _c("from_dense", "coo_fill", R=1024, C=65, dt="bf16", density=0.3),         # the scan's share: 1 | 2 rows per thread
    _c("from_dense", "coo_fill", R=1025, C=65, dt="bf16", density=0.3),
    _c("count", "coo_count", R=1025, C=65, dt="f32", density=0.3),
    _c("count", "coo_count", R=1024, C=64, dt="bf16", density=0.3, threshold=0.5),
    _c("from_dense", "coo_fill", R=33, C=130, dt="f16", density=0.5, threshold=0.3, special="edges"),
    _c("from_dense", "coo_fill", R=33, C=130, dt="bf16", density=0.5, threshold=0.3, special="edges"),
    _c("from_dense", "coo_fill", R=33, C=130, dt="f32", density=0.5, threshold=0.3, special="edges"),
    _c("from_dense", "coo_fill", R=33, C=130, dt="f16", density=0.5, special="edges"),          # the same values without a threshold
    _c("from_dense", "coo_fill", R=33, C=130, dt="f32", density=0.5, special="edges"),
]
QUANTIZE_COO_FORMS = [
    _c("quantize_coo", "coo_quantize", "parts1", n=2048, dt="f16"),
    _c("quantize_coo", "coo_quantize", "parts2", n=2049, dt="f16"),
    _c("quantize_coo", "coo_quantize", "parts1024", n=2097152, dt="bf16"),
    _c("quantize_coo", "coo_quantize", "parts1024", n=2097153, dt="f32"),
    _c("quantize_coo", "coo_quantize", "parts2", n=2049, dt="f32", special="nonfinite"),       # scale NaN, every code 0
]


def _sp(kernel, variant, N, dt, **kw):
    kw.setdefault("index", "permuted")
    kw.setdefault("values", "T")
    return _c("spmm", kernel, variant, rows=37, cols=200, N=N, dt=dt, density=0.1, **kw)      # 37 rows: ragged against 4, 8 and 16 rows per workgroup


SPMM_FORMS = [
    # vector form, 16-bit (8 columns per lane): G = 16 | 32 | 64 and a second, ragged tile
    _sp("spmm_coo8", "G16 x1", 128, "bf16"), _sp("spmm_coo8", "G32 x1", 136, "bf16"),
    _sp("spmm_coo8", "G32 x1", 256, "f16"), _sp("spmm_coo8", "G64 x1", 264, "f16"),
    _sp("spmm_coo8", "G64 x1", 512, "bf16"), _sp("spmm_coo8", "G64 x2", 520, "bf16"),
    # vector form, f32 (4 columns per lane)
    _sp("spmm_coo8", "G16 x1", 64, "f32"), _sp("spmm_coo8", "G32 x1", 68, "f32"),
    _sp("spmm_coo8", "G32 x1", 128, "f32", index="sorted"), _sp("spmm_coo8", "G64 x1", 132, "f32"),
    _sp("spmm_coo8", "G64 x1", 256, "f32", index="duplicates"), _sp("spmm_coo8", "G64 x2", 260, "f32"),
    # scalar form (4 columns per lane, G apart): the multiples of 8 reach it through a `dense` 4 bytes off
    _sp("spmm_coo1", "G16 x1", 64, "f32", off={"dense": 4}), _sp("spmm_coo1", "G32 x1", 65, "f32"),
    _sp("spmm_coo1", "G32 x1", 128, "f16", off={"dense": 2}), _sp("spmm_coo1", "G64 x1", 129, "f32"),
    _sp("spmm_coo1", "G64 x1", 256, "bf16", off={"dense": 2}), _sp("spmm_coo1", "G64 x2", 257, "bf16"),
    _sp("spmm_coo1", "G64 x3", 515, "f16", index="int32"), _sp("spmm_coo1_general", "G64 x3", 515, "f32", index="sorted", generic=True),
    # a per-entry scale in the two other dtypes
    _sp("spmm_coo8", "G16 x1", 72, "f16", values="int8_entry"), _sp("spmm_coo8", "G32 x1", 72, "f32", values="int8_entry"),
    _sp("spmm_coo1", "G16 x1", 9, "f32", values="int8_entry", index="sorted"),
    # the scalar form's narrowest group in the 16-bit dtypes; one scale for all entries in bf16
    _sp("spmm_coo1", "G16 x1", 10, "f16"), _sp("spmm_coo1", "G16 x1", 10, "bf16", values="int8"),
    # each operand offset against N = 128 bf16 above: `dense` and `out` change the form, the lists must not
    _sp("spmm_coo8", "G16 x1", 128, "bf16", off={"row": 8}), _sp("spmm_coo8", "G16 x1", 128, "bf16", off={"col": 8}),
    _sp("spmm_coo8", "G16 x1", 128, "bf16", off={"values": 2}),
    _sp("spmm_coo1", "G32 x1", 128, "bf16", off={"dense": 2}), _sp("spmm_coo1", "G32 x1", 128, "bf16", off={"out": 2}),
]
FORMS = QUANTIZE_FORMS + DEQUANT_FORMS + MATMUL_FORMS + FROM_DENSE_FORMS + QUANTIZE_COO_FORMS + SPMM_FORMS
CASES = QUANTIZE + DEQUANT + MATMUL + FROM_DENSE + QUANTIZE_COO + SPMM + FORMS
PLAN_OPERANDS = {"quantize": ("q", "rs", "cs", "ws"), "dequant": ("out",), "matmul": ("out", "ws"), "spmm": ("out", "ws")}     # functional.py's allocations, in order


def needs_plan(c):
    """An offset on a buffer functional.py allocates itself: reachable through the plan of tests/guard.py only."""
    return any(k in PLAN_OPERANDS.get(c["op"], ()) for k in c.get("off", {}))


def launches_gemm(c):
    return c["kernel"].endswith("+dense")


def _off(c, operand, main):
    """Bytes off alignment of `operand`; the old key view="misaligned" moves the op's main operand by one element."""
    if c.get("view") == "misaligned" and operand == main:
        return ESIZE[c["dt"]]
    return c.get("off", {}).get(operand, 0)


MAIN_OPERAND = {"quantize": "x", "dequant": "q", "matmul": "x", "spmm": "dense"}


def offset(c, operand):
    return _off(c, operand, MAIN_OPERAND.get(c["op"]))


def rows_of(c):
    if "lead" in c:
        m = 1
        for v in c["lead"]:
            m *= v
        return m
    return c["M"]


def derived(c):
    """The sizes the launchers and kernels branch on."""
    op, d = c["op"], {}
    if op in ("quantize", "dequant"):
        R, C = c["R"], c["C"]
        d.update(nchunk=-(-C // CR_CB), nrb=-(-R // CR_RB), cblocks=-(-C // 64), rblocks=-(-R // 256), quads=-(-R // CR_UN))
    elif op == "matmul":
        M, N, K = rows_of(c), c["N"], c["K"]
        d.update(M=M, macs=M * N * K, weight=N * K)
    elif op in ("count", "from_dense"):
        d.update(per=-(-c["R"] // SCAN_THREADS), steps=-(-c["C"] // 64))
    elif op == "quantize_coo":
        d.update(want=-(-c["n"] // 2048))
    elif op == "spmm":
        N, es = c["N"], ESIZE[c["dt"]]
        vec = (N * es) % 16 == 0 and _off(c, "dense", "dense") % 16 == 0 and _off(c, "out", "dense") % 16 == 0
        cpl = 16 // es if vec else 4
        G = 64
        while G > 16 and (G // 2) * cpl >= N:
            G //= 2
        d.update(vec=vec, cpl=cpl, G=G, ntile=-(-N // (G * cpl)), rows_per_wg=4 * (64 // G), per=-(-c["rows"] // SCAN_THREADS))
    return d


def model(c):
    """(kernel, variant) by the launchers' conditions (sparse_kernels.hip's host side), restated."""
    op, d, is16 = c["op"], derived(c), c["dt"] != "f32"
    if op == "quantize":
        vec = c["C"] % 8 == 0 and _off(c, "x", "x") % 16 == 0 and _off(c, "cs", "x") % 16 == 0 and _off(c, "q", "x") % 8 == 0
        return (_Q8 if vec else _Q1), ""
    if op == "dequant":
        vec = c["C"] % 8 == 0 and _off(c, "q", "q") % 8 == 0 and _off(c, "cm", "q") % 16 == 0 and _off(c, "out", "q") % 16 == 0
        return (_DQ8 if vec else _DQ1), ("wt" if vec and is16 and c.get("route") == "pass" else "")
    if op == "matmul":
        M, N, K = d["M"], c["N"], c["K"]
        shape = is16 and M > 0 and N > 0 and K % 64 == 0 and K >= 128 and 256 * K * 2 < 1 << 31 and M * N * 4 < 1 << 40 and \
            M * N * K >= 1 << 27 and (M >= 16 or N * K >= 1 << 25)
        ptrs = _off(c, "ws", "x") % 256 == 0 and _off(c, "x", "x") % 16 == 0 and _off(c, "w", "x") % 8 == 0 and _off(c, "cm", "x") % 16 == 0 and \
            _off(c, "out", "x") % 16 == 0
        return (_DENSE, "wt") if shape and ptrs and not c.get("generic") else (_GEN, "")
    if op == "count":
        return "coo_count", ""
    if op == "from_dense":
        return "coo_fill", ""
    if op == "quantize_coo":
        return "coo_quantize", f"parts{min(d['want'], COO_QP)}"
    assert op == "spmm"
    name = ("spmm_coo8" if d["vec"] else "spmm_coo1") + ("_general" if c.get("generic") else "")
    return name, f"G{d['G']} x{d['ntile']}"


# Every limit a launcher or a kernel of sparse_kernels.hip compares a size with: (what, ops, first side, second side), predicates of
# (case, derived(case)).  tests/test_int8_decomp_host.py requires a case on each side and holds the sources' literals against LIMIT_CLAIMS.
def _vec(c):
    return c["kernel"].endswith("8")


THRESHOLDS = [
    ("C % 8", ("quantize", "dequant"), lambda c, d: c["C"] % 8 == 0, lambda c, d: c["C"] % 8 != 0),
    ("vector nchunk 1|2", ("quantize", "dequant"), lambda c, d: _vec(c) and d["nchunk"] == 1, lambda c, d: _vec(c) and d["nchunk"] > 1),
    ("scalar nchunk 1|2", ("quantize", "dequant"), lambda c, d: not _vec(c) and d["nchunk"] == 1, lambda c, d: not _vec(c) and d["nchunk"] > 1),
    ("merge nrb 3|4", ("quantize",), lambda c, d: d["nrb"] == 3, lambda c, d: d["nrb"] == 4),
    ("merge nrb 4|5", ("quantize",), lambda c, d: d["nrb"] == 4, lambda c, d: d["nrb"] == 5),
    ("row block R 48|49", ("quantize",), lambda c, d: c["R"] == 48, lambda c, d: c["R"] == 49),
    ("row block R 64|65", ("quantize",), lambda c, d: c["R"] == 64, lambda c, d: c["R"] == 65),
    ("merge cblocks 1|2", ("quantize",), lambda c, d: d["cblocks"] == 1, lambda c, d: d["cblocks"] == 2),
    ("merge rblocks 1|2", ("quantize",), lambda c, d: c["R"] == 256, lambda c, d: c["R"] == 257),
    ("rows % 4", ("quantize", "dequant"), lambda c, d: c["R"] % CR_UN == 0, lambda c, d: c["R"] % CR_UN != 0),
    ("K % 64", ("matmul",), lambda c, d: c["K"] % 64 == 0 and c["kernel"] == _DENSE, lambda c, d: c["K"] % 64 != 0 and c["dt"] != "f32" and d["macs"] >= 1 << 27),
    ("K >= 128", ("matmul",), lambda c, d: c["K"] == 64 and d["macs"] >= 1 << 27, lambda c, d: c["K"] == 128 and c["kernel"] == _DENSE),
    ("M N K >= 2^27", ("matmul",), lambda c, d: d["macs"] == 1 << 27 and c["kernel"] == _DENSE,
     lambda c, d: (1 << 27) - (1 << 22) <= d["macs"] < 1 << 27 and d["M"] >= 16 and c["K"] % 64 == 0 and c["dt"] != "f32"),
    ("M >= 16", ("matmul",), lambda c, d: d["M"] == 16 and d["weight"] < 1 << 25 and c["kernel"] == _DENSE,
     lambda c, d: d["M"] == 15 and d["weight"] < 1 << 25 and d["macs"] >= 1 << 27 and c["kernel"] == _GEN),
    ("N K >= 2^25", ("matmul",), lambda c, d: d["M"] < 16 and d["weight"] == 1 << 25 and c["kernel"] == _DENSE,
     lambda c, d: d["M"] < 16 and d["weight"] == (1 << 25) - 64 * c["N"] and d["macs"] >= 1 << 27 and c["kernel"] == _GEN),
    ("scan share (int64) 1|2", ("from_dense",), lambda c, d: c["R"] == 1024, lambda c, d: c["R"] == 1025),
    ("from_dense 64-column steps 1|2", ("from_dense",), lambda c, d: c["C"] == 64, lambda c, d: c["C"] == 65),
    ("threshold > 0", ("from_dense",), lambda c, d: c.get("threshold", 0.0) > 0, lambda c, d: c.get("threshold", 0.0) == 0),
    ("coo_quantize 2048 values per workgroup", ("quantize_coo",), lambda c, d: c["n"] == 2048, lambda c, d: c["n"] == 2049),
    ("coo_quantize COO_QP partials", ("quantize_coo",), lambda c, d: c["n"] == 2048 * COO_QP, lambda c, d: c["n"] == 2048 * COO_QP + 1),
    ("spmm vector shape", ("spmm",), lambda c, d: (c["N"] * ESIZE[c["dt"]]) % 16 == 0, lambda c, d: (c["N"] * ESIZE[c["dt"]]) % 16 != 0),
] + [
    (f"spmm {form} {dts[0]} G {lo}|{hi} at N {n}|{m}", ("spmm",),
     lambda c, d, f=form, t=dts, n=n, g=lo: d["vec"] == (f == "vector") and c["dt"] in t and c["N"] == n and d["G"] == g,
     lambda c, d, f=form, t=dts, m=m, g=hi: d["vec"] == (f == "vector") and c["dt"] in t and c["N"] == m and d["G"] == g)
    for form, dts, lo, hi, n, m in (
        ("vector", ("f16", "bf16"), 16, 32, 128, 136), ("vector", ("f16", "bf16"), 32, 64, 256, 264),
        ("vector", ("f32",), 16, 32, 64, 68), ("vector", ("f32",), 32, 64, 128, 132),
        ("scalar", ("f16", "bf16", "f32"), 16, 32, 64, 65), ("scalar", ("f16", "bf16", "f32"), 32, 64, 128, 129))
] + [
    (f"spmm {form} {dts[0]} tiles 1|2 at N {n}|{m}", ("spmm",),
     lambda c, d, f=form, t=dts, n=n: d["vec"] == (f == "vector") and c["dt"] in t and c["N"] == n and d["ntile"] == 1,
     lambda c, d, f=form, t=dts, m=m: d["vec"] == (f == "vector") and c["dt"] in t and c["N"] == m and d["ntile"] == 2)
    for form, dts, n, m in (("vector", ("f16", "bf16"), 512, 520), ("vector", ("f32",), 256, 260), ("scalar", ("f16", "bf16", "f32"), 256, 257))
] + [
    (f"spmm rows ragged against {4 * (64 // g)} per workgroup, G = {g}", ("spmm",),
     lambda c, d, g=g: d["G"] == g and c["rows"] % d["rows_per_wg"] != 0, lambda c, d, g=g: d["G"] == g and c["rows"] % d["rows_per_wg"] == 0)
    for g in (16, 32, 64)
]
# The CSR build's limits are held by tests/test_gpu_int8_decomp.py::test_csr_build_is_exact (planned row lengths and row counts), not by table cases.
CSR_ROW_LENGTHS = (0, 1, 2, 3, 5, 255, 256, 257, 4095, 4096, 4097, 9000)     # L < 2, the network's skipped comparators, one pass of 256 threads, COO_SORT_LDS
CSR_ROW_COUNTS = (1024, 1025, 5000)                                           # k_scan_counts<int>: 1 | 2 | 5 rows per thread
_CSR = "tests/test_gpu_int8_decomp.py::test_csr_build_is_exact"

# Every literal the host side of sparse_kernels.hip compares with (the scan of tests/test_int8_decomp_host.py) and the constants its kernels
# tile by: a THRESHOLDS row, or ("no case", why).
LIMIT_CLAIMS = {
    "% 8": "C % 8", "% 16": "spmm vector shape", "% 64": "K % 64", "128": "K >= 128",
    "16": ["M >= 16", "spmm scalar f16 G 16|32 at N 64|65", "spmm vector f16 G 16|32 at N 128|136", "spmm vector f32 G 16|32 at N 64|68"],      # M >= 16 and `G > 16`
    "kCrDenseMacs": "M N K >= 2^27", "kCrBigWeight": "N K >= 2^25",
    "1 << 31": ("no case", "256 K 2 < 2^31 needs K >= 2^22: a weight row of 4 M codes, no shape of the suite's budget"),
    "1 << 40": ("no case", "M N 4 < 2^40 needs an output of 2^38 elements"),
    "kMaxGrid": ("no case", "2^31 - 1 workgroups: the smallest such launch is 2^33 elements"),
    "kMaxElems": ("no case", "the argument check of every entry point; held without a GPU by test_argument_errors_return_a_status_before_any_device_access"),
    "kMaxIndex": ("no case", "nnz and rows below 2^31 - 1: an argument check, held without a GPU"),
    "2": ("no case", "sizeof(T) == 2: a dtype test, held by INSTANTIATED"),
    "COO_QP": "coo_quantize COO_QP partials",
    "CR_CB": "scalar nchunk 1|2", "CR_RB": "merge nrb 3|4", "CR_UN": "rows % 4", "CR_GM": ("no case", "the generic kernel's 8 rows per workgroup: M = 1, 10, 15, 17, 31 and multiples of 8 all run"),
    "COO_SORT_LDS": _CSR,
}

# form -> the dtypes it is compiled for; every one needs a case (scalar and vector forms of the same kernel are separate instantiations)
_ALL = ("f16", "bf16", "f32")
INSTANTIATED = {
    (_Q8, ""): _ALL, (_Q1, ""): _ALL, (_DQ8, ""): _ALL, (_DQ1, ""): _ALL, (_DQ8, "wt"): ("f16", "bf16"), (_DENSE, "wt"): ("f16", "bf16"),
    (_GEN, ""): _ALL, ("coo_count", ""): _ALL, ("coo_fill", ""): _ALL, ("coo_quantize", None): _ALL,
    # k_spmm_csr<T, VEC>: G and the value kind are run-time arguments, held by THRESHOLDS and by the two last rows
    ("spmm_coo8", None): _ALL, ("spmm_coo1", None): _ALL,
    ("spmm_coo8_general", None): ("f16",), ("spmm_coo1_general", None): ("f32",),      # the same instantiations; the CSR build has no dtype
    ("spmm int8_entry", None): _ALL, ("spmm int8", None): _ALL,
}

# (C name in the launcher, bytes) of every aligned() test that picks a form -> (op, the operand of `off`); the host test requires for each a
# pair of cases that differ in that offset alone and take different (kernel, variant).
OPERAND_ALIGNMENT_TESTED = {
    ("colrow_quantize", "x", 16): ("quantize", "x"), ("colrow_quantize", "col_absmax", 16): ("quantize", "cs"), ("colrow_quantize", "q", 8): ("quantize", "q"),
    ("cr_dequant_launch", "q", 8): ("dequant", "q"), ("cr_dequant_launch", "cm", 16): ("dequant", "cm"), ("cr_dequant_launch", "out", 16): ("dequant", "out"),
    ("cr_matmul", "ws", 256): ("matmul", "ws"), ("cr_matmul", "X", 16): ("matmul", "x"), ("cr_matmul", "W", 8): ("matmul", "w"),
    ("cr_matmul", "cm", 16): ("matmul", "cm"), ("cr_matmul", "out", 16): ("matmul", "out"),
    ("spmm_coo", "dense", 16): ("spmm", "dense"), ("spmm_coo", "out", 16): ("spmm", "out"),
}
# aligned() tests that are argument requirements (an error, no other form): held by test_argument_errors_return_a_status_before_any_device_access
ALIGNMENT_REQUIRED = {("colrow_quantize", "workspace", 256), ("coo_quantize", "workspace", 256), ("spmm_coo", "workspace", 256), ("coo_count", "row_ptr", 8),
                      ("coo_fill", "row_ptr", 8), ("coo_fill", "row", 8), ("coo_fill", "col", 8)}
# how often the host side compares with each literal; a new comparison changes a count until its THRESHOLDS row and cases follow
LIMIT_COUNTS = {"% 8": 3, "% 64": 1, "% 16": 1, "kMaxGrid": 6, "2": 3, "128": 1, "1 << 31": 1, "1 << 40": 1, "kCrDenseMacs": 1, "16": 2, "kCrBigWeight": 1,
                "kMaxElems": 15, "kMaxIndex": 6, "COO_QP": 2}
TILE_CONSTANTS = ("CR_CB", "CR_RB", "CR_UN", "CR_GM", "COO_QP", "COO_SORT_LDS")
# operands whose offset must NOT change the form (element alignment is all the kernels ask of them)
OPERAND_ALIGNMENT_FREE = {("spmm", "row"), ("spmm", "col"), ("spmm", "values")}


def case_id(c):
    if c["op"] == "matmul":
        rows = "x".join(map(str, c["lead"])) if "lead" in c else str(c["M"])
        shape = [rows or "1d", str(c["N"]), str(c["K"])]
    elif c["op"] == "spmm":
        shape = [str(c["rows"]), str(c["cols"]), str(c["N"]), str(c["density"]), c["index"], c["values"]]
    elif c["op"] == "quantize_coo":
        shape = [str(c["n"])]
    else:
        shape = [str(c["R"]), str(c["C"])] + ([str(c["density"])] if "density" in c else []) + ([f"thr{c['threshold']}"] if "threshold" in c else [])
    parts = [c["op"], c["kernel"]] + shape + [c["dt"]]
    parts += [k for k in ("bias", "generic") if c.get(k)] + ([c["view"]] if "view" in c else []) + ([c["route"]] if "route" in c else [])
    parts += [f"{k}+{v}" for k, v in sorted(c.get("off", {}).items())] + ([c["special"]] if "special" in c else [])
    return "-".join(parts)
