"""
The kernel routes of libmbnb_sparse.so (include/mbnb_sparse.h), one table.  Each case names an op, a shape, a dtype and the name
mbnb_sparse_last_kernel() must report for it.  Data only, importable without a GPU: tests/test_gpu_int8_decomp.py runs every case and
checks every output element (bit for bit against the emulation of tests/int8_decomp_emul.py, or against float64 with the bound of
tests/elementwise.py); tests/test_int8_decomp_host.py checks that every name the library can report (its kSparseKernelNames table) is
the kernel of some case.

Keys
  op       quantize (quantize_colrow), dequant (dequantize_colrow; route "pass": functional._colrow_dequant_pass), matmul (functional._matmul_colrow), count (sparse_coo_from_dense's
           first launch pair, functional._coo_row_ptr), from_dense (sparse_coo_from_dense), quantize_coo (quantize_sparse_coo),
           spmm (functional._spmm_coo)
  R C      rows and columns of the matrix;  M N K: tokens, output columns, input columns of matmul (lead: the leading dims of the
           input instead of M; () is a 1-D input);  rows cols N density: the sparse shape, the dense matrix's width, the share of nonzeros
  dt       "f16" | "bf16" | "f32";  bias: with a bias;  generic: MBNB_SPARSE_FORCE_GENERIC;  view "misaligned": the main operand 2 bytes
           (4 for f32) off 16-byte alignment;  threshold: of from_dense
  index    "sorted" | "permuted" | "int32" | "duplicates";  values: "T" | "int8" | "int8_entry"
"""


def _c(op, kernel, **kw):
    kw.update(op=op, kernel=kernel)
    return kw


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
    _c("dequant", "colrow_dequant8", R=4096, C=4096, dt="bf16", route="pass"),
    _c("dequant", "colrow_dequant8", R=5003, C=192, dt="f16", route="pass"),
    _c("dequant", "colrow_dequant8", R=1000, C=1000, dt="f32", route="pass"),
    _c("dequant", "colrow_dequant1", R=77, C=100, dt="bf16", route="pass"),
]
MATMUL = [
    _c("matmul", "colrow_dq+dense", M=512, N=3072, K=512, dt="bf16", bias=True),
    _c("matmul", "colrow_dq+dense", M=300, N=5003, K=192, dt="f16", bias=True),        # ragged N
    _c("matmul", "colrow_dq+dense", M=1024, N=2048, K=1024, dt="f16"),
    _c("matmul", "colrow_dq+dense", lead=(4, 128), N=4096, K=256, dt="bf16", bias=True),
    _c("matmul", "colrow_dq+dense", M=16, N=4096, K=4096, dt="f16", bias=True),
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
    _c("quantize_coo", "coo_quantize", n=100000, dt="f32"),
    _c("quantize_coo", "coo_quantize", n=5000001, dt="f16"),               # more than the 1024 partial maxima cover in one pass
    _c("quantize_coo", "coo_quantize", n=1, dt="bf16"),
    _c("quantize_coo", "coo_quantize", n=777, dt="bf16"),
]
SPMM = [
    _c("spmm", "spmm_coo8", rows=1000, cols=2000, N=256, dt="f16", density=0.05, index="sorted", values="T"),
    _c("spmm", "spmm_coo8", rows=1000, cols=2000, N=256, dt="f32", density=0.05, index="permuted", values="T"),
    _c("spmm", "spmm_coo8", rows=1000, cols=2000, N=256, dt="bf16", density=0.05, index="duplicates", values="T"),
    _c("spmm", "spmm_coo8", rows=512, cols=1024, N=4096, dt="bf16", density=0.02, index="int32", values="T"),     # a whole wave per row, 8 tiles
    _c("spmm", "spmm_coo8", rows=300, cols=500, N=64, dt="f16", density=0.1, index="permuted", values="int8"),     # 16 lanes per row
    _c("spmm", "spmm_coo8", rows=300, cols=500, N=72, dt="bf16", density=0.1, index="sorted", values="int8_entry"),
    _c("spmm", "spmm_coo8", rows=40, cols=9000, N=128, dt="f32", density=0.7, index="permuted", values="T"),       # 6300 entries per row: sorted in global memory
    _c("spmm", "spmm_coo8", rows=64, cols=64, N=8, dt="f16", density=0.0, index="sorted", values="T"),             # nnz = 0: zeros
    _c("spmm", "spmm_coo1", rows=1000, cols=2000, N=250, dt="f16", density=0.05, index="permuted", values="T"),    # N * 2 % 16 != 0
    _c("spmm", "spmm_coo1", rows=77, cols=100, N=3, dt="f32", density=0.2, index="sorted", values="int8"),
    _c("spmm", "spmm_coo1", rows=200, cols=300, N=256, dt="bf16", density=0.1, index="int32", values="T", view="misaligned"),
    _c("spmm", "spmm_coo8_general", rows=1000, cols=2000, N=256, dt="f16", density=0.05, index="sorted", values="T", generic=True),
    _c("spmm", "spmm_coo1_general", rows=77, cols=100, N=3, dt="f32", density=0.2, index="sorted", values="T", generic=True),
]
CASES = QUANTIZE + DEQUANT + MATMUL + FROM_DENSE + QUANTIZE_COO + SPMM


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
    return "-".join(parts)
