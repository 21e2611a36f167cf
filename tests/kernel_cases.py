"""
One table of the library's kernels.  Each case names an op, a shape, dtypes and format options, and the kernel name
(mbnb_last_kernel) the case must dispatch to.  Data only, importable without a GPU: tests/test_gpu_elementwise.py runs the
cases through the public API and checks every output element against float64 (tests/elementwise.py), and
tests/test_elementwise_host.py checks that every name the library can report is the kernel of some case.

Keys
  op       matmul_4bit, linear_int8, matmul_fp8, linear_dense, gemm_dense (mbnb_gemm_dense through the C ABI), matmul_int8,
           grad (x.grad through .backward()), grad_t (the transposed dequantise pass alone), outlier_linear, embedding_4bit,
           embedding_8bit
  kernel   the name; one ending in a space is a prefix ("dense_nb ": the plan follows)
  M N K    rows, output columns, contraction (lead: the leading dims of a 3-D input instead of M)
  dt       weight / compute dtype "f16" | "bf16" | "f32";  out: the output dtype where it differs (compute_dtype, dtype)
  qt bs cs 4-bit code table, blocksize, nested absmax;  fmt: the weight format of grad / grad_t ("4bit", "int8", "fp8")
  bias     with a bias;  fused: DECODE_ONCE = False (the fused kernels at every M)
  view     "rows": X a row slice of a taller tensor at an odd row offset;  "misaligned": X 2 bytes off 16-byte alignment
  xexp     (lo, hi): row i of X scaled by 2^e, e running from lo to hi over the rows
  bad      "x": a NaN in one X row, +Inf in another, -Inf in a third;  "w": one poisoned weight block (a NaN absmax, a NaN row
           scale, FP8 byte 0x7F, a NaN column scale of matmul_int8)
  tile slices ldw   mbnb_gemm_dense's tile code (0 the plan, 1 256 x 128, 2 256 x 256, 3 128 x 128), K slices, weight pitch
  n_out    outlier columns of outlier_linear
  xfail    a known library departure the case exposes (run as a strict xfail: it fails loudly once fixed)
"""


def _c(op, kernel, **kw):
    kw.update(op=op, kernel=kernel)
    return kw


BF16_RANGE = (-40, 40)     # bf16 rows over 80 binades (bf16 or f32 output only)
F16_RANGE = (-8, 4)        # f16: |y| stays below 2^15

MATMUL_4BIT = [
    # k_gemv4_lean: M = 1, blocksize 64, K % 64 == 0, 1024 <= K <= 16384
    _c("matmul_4bit", "gemv", M=1, N=4096, K=4096, dt="bf16", bias=True, bad="w"),
    _c("matmul_4bit", "gemv", M=1, N=777, K=11008, dt="f16", cs=True),
    _c("matmul_4bit", "gemv", M=1, N=257, K=1088, dt="f16", qt="fp4"),                # one partial chunk, N = 256 + 1
    _c("matmul_4bit", "gemv", M=1, N=256, K=1024, dt="bf16", view="rows"),          # the shortest K of the lean form
    # k_gemv4, the plain form
    _c("matmul_4bit", "gemv", M=1, N=64, K=96, dt="f16"),                            # K_weight = 128 > K
    # k_gemv4 answers the chunks past K from a clamped address (k = 0): the Inf at X[3, 5] sits in the chunk they re-read, and must
    # not reach the sum a second time as Inf * 0
    _c("matmul_4bit", "gemv", M=5, N=64, K=2080, dt="bf16", bias=True, bad="x"),
    _c("matmul_4bit", "gemv", M=2, N=64, K=4160, dt="f16", xexp=F16_RANGE),         # ragged last k-step
    # k_skinny4
    _c("matmul_4bit", "skinny_mfma16", M=7, N=1000, K=384, dt="f16", qt="fp4", cs=True),
    _c("matmul_4bit", "skinny_mfma16", M=17, N=48, K=128, dt="f16", bs=32),
    _c("matmul_4bit", "skinny_mfma16", M=28, N=4096, K=1024, dt="f16", out="f32", xexp=F16_RANGE, bad="x"),
    _c("matmul_4bit", "skinny_mfma16", M=32, N=4096, K=384, dt="bf16", bias=True, xexp=BF16_RANGE),
    _c("matmul_4bit", "skinny_mfma16", lead=(2, 5), N=128, K=256, dt="f16", bias=True),   # 3-D input
    # k_gemm_small (the fused kernels: DECODE_ONCE = False where the decode-once path would take the shape)
    _c("matmul_4bit", "mfma_small", M=100, N=4096, K=1280, dt="bf16", fused=True),
    _c("matmul_4bit", "mfma_small", M=256, N=1024, K=2048, dt="f16", fused=True),
    _c("matmul_4bit", "mfma_small", M=384, N=11008, K=4096, dt="bf16", out="f32", fused=True, xexp=BF16_RANGE),
    _c("matmul_4bit", "mfma_small_splitk", M=133, N=777, K=2304, dt="bf16", bias=True, fused=True),   # slices of 2 and 1 steps
    _c("matmul_4bit", "mfma_small_splitk", M=190, N=1000, K=2048, dt="f16", qt="fp4", cs=True, fused=True, bad="x"),
    _c("matmul_4bit", "mfma_small_splitk", M=64, N=4096, K=4096, dt="bf16", bs=128, cs=True, fused=True),
    # k_gemm_mid (N < 64 keeps k_gemm_small off the split shapes)
    _c("matmul_4bit", "mfma_mid", M=65, N=64, K=256, dt="bf16", fused=True),
    _c("matmul_4bit", "mfma_mid", M=300, N=8192, K=256, dt="f16", bias=True, fused=True),
    _c("matmul_4bit", "mfma_mid_splitk", M=100, N=48, K=2304, dt="bf16", bias=True),     # 5 slices, the last one short
    _c("matmul_4bit", "mfma_mid_splitk", M=129, N=40, K=1024, dt="f16", cs=True, out="f32"),
    # k_gemm_decode, 128 x 128 tiles
    _c("matmul_4bit", "mfma128", M=1, N=64, K=72, dt="f16", bias=True),             # K % 32 != 0: not the GEMV
    _c("matmul_4bit", "mfma128_splitk", M=1024, N=2048, K=4096, dt="f16", fused=True),
    _c("matmul_4bit", "mfma128_splitk", M=640, N=4096, K=2048, dt="bf16", out="f32", fused=True, xexp=BF16_RANGE),
    # k_gemm256p / k_gemm_fused4
    _c("matmul_4bit", "mfma256", M=2500, N=2600, K=128, dt="bf16", qt="fp4", cs=True, bs=32, fused=True),
    _c("matmul_4bit", "mfma256", M=3000, N=2304, K=384, dt="f16", cs=True, bs=128, out="f32", bias=True, fused=True),
    _c("matmul_4bit", "mfma256f", M=2560, N=2560, K=256, dt="bf16", fused=True),
    _c("matmul_4bit", "mfma256f", M=2305, N=2600, K=512, dt="f16", bias=True, fused=True, bad="x"),   # M = 9 * 256 + 1
    # decode once: dequantize_4bit into the scratch + k_gemm_dense
    _c("matmul_4bit", "dequant+dense", M=700, N=4096, K=4096, dt="f16", view="rows"),
    _c("matmul_4bit", "dequant+dense", M=2500, N=2600, K=192, dt="f16", bias=True, bad="xw"),
    _c("matmul_4bit", "dequant+dense", M=257, N=11008, K=512, dt="f16", cs=True),     # one row in the last 128-row tile
    _c("matmul_4bit", "dequant+dense", M=2049, N=2048, K=1024, dt="bf16", xexp=BF16_RANGE),
    _c("matmul_4bit", "dequant+dense_splitk", M=640, N=2048, K=8128, dt="bf16", bias=True),   # 6 slices, the last one short
    _c("matmul_4bit", "dequant+dense_f32", M=600, N=512, K=224, dt="f32"),
    _c("matmul_4bit", "dequant+dense_f32_splitk", M=300, N=1000, K=1028, dt="f32", cs=True, bias=True),   # K_weight = 1088 > K
    # k_matmul4_generic
    _c("matmul_4bit", "generic", M=32, N=63, K=127, dt="f16"),                       # K % 8 != 0
    _c("matmul_4bit", "generic", M=4, N=64, K=128, dt="f16", bs=16, bad="w"),          # blocksize 16
    _c("matmul_4bit", "generic", M=4, N=512, K=1024, dt="f32", bias=True),
    _c("matmul_4bit", "generic", M=40, N=64, K=128, dt="f32", out="bf16"),
    _c("matmul_4bit", "generic", M=64, N=256, K=512, dt="f16", view="misaligned"),   # the dispatchers' alignment fallback
]

_W8_SHAPES = [
    ("skinny", dict(M=7, N=1000, K=384, dt="f16", bias=True)),
    ("skinny", dict(M=33, N=300, K=256, dt="f16", bad="x")),
    ("small", dict(M=64, N=4096, K=1024, dt="f16", bias=True)),
    ("small", dict(M=40, N=1000, K=512, dt="bf16", xexp=BF16_RANGE)),
    ("small_splitk", dict(M=240, N=2048, K=2048, dt="bf16", bias=True)),
    ("mfma128", dict(M=200, N=520, K=448, dt="f16", bias=True)),
    ("mfma128_splitk", dict(M=300, N=1000, K=1024, dt="f16")),
    ("generic", dict(M=5, N=100, K=72, dt="f16", bias=True, bad="w")),
    ("mfma256", dict(M=2500, N=2600, K=192, dt="f16", fused=True)),
    ("dequant+dense", dict(M=2500, N=2600, K=192, dt="f16", bias=True)),
    ("dequant+dense", dict(M=1024, N=4096, K=2048, dt="bf16", view="rows")),
    ("dequant+dense_splitk", dict(M=512, N=2048, K=8192, dt="bf16")),
]
LINEAR_8BIT = ([_c("linear_int8", "w8a16_" + k, **kw) for k, kw in _W8_SHAPES] +
               [_c("matmul_fp8", "fp8a16_" + k, **kw) for k, kw in _W8_SHAPES])

DENSE = [
    # mbnb_gemm_dense through the C ABI: the tile and the K slices forced, the output and the partials poisoned by hand
    _c("gemm_dense", "dense 256x256", M=515, N=1000, K=640, ldw=704, tile=2, slices=1, dt="bf16", out="f32", bias=True),
    _c("gemm_dense", "dense 256x128", M=515, N=1000, K=640, ldw=640, tile=1, slices=1, dt="f16", bias=True),
    _c("gemm_dense", "dense 128x128", M=129, N=257, K=192, ldw=200, tile=3, slices=1, dt="f16", bias=True),
    _c("gemm_dense", "dense 128x128", M=127, N=128, K=256, ldw=256, tile=3, slices=1, dt="bf16", out="f16", bad="x"),
    _c("gemm_dense", "dense 256x256_splitk", M=515, N=1000, K=640, ldw=640, tile=2, slices=3, dt="bf16", bias=True),   # 4 + 4 + 2 steps
    _c("gemm_dense", "dense 256x128_splitk", M=257, N=255, K=1088, ldw=1088, tile=1, slices=4, dt="f16", out="bf16", bias=True),
    _c("gemm_dense", "dense_nb ", M=4096, N=6144, K=4096, ldw=4096, tile=0, slices=1, dt="bf16"),    # the plan: 32 columns of 192
    # linear_dense: the library's plan
    _c("linear_dense", "dense 128x128", M=700, N=4096, K=4096, dt="bf16", bias=True),
    _c("linear_dense", "dense 256x128", M=2500, N=2600, K=192, dt="f16", bias=True, xexp=F16_RANGE),
    _c("linear_dense", "dense 256x128_splitk", M=640, N=2048, K=8128, dt="bf16"),
]

MATMUL_INT8 = [
    _c("matmul_int8", "i8_inplace4", M=2560, N=2560, K=384, out="f32"),
    _c("matmul_int8", "i8_inplace4", M=2500, N=2608, K=256, out="bf16", bad="w"),
    _c("matmul_int8", "i8_mfma256", M=2560, N=2560, K=128, out="f16"),
    _c("matmul_int8", "i8_mfma128", M=200, N=136, K=320, out="f32"),
    _c("matmul_int8", "i8_generic", M=64, N=100, K=70, out="f16"),                    # K % 16 != 0
    _c("matmul_int8", "i8_transpose+dense", M=24576, N=192, K=256, out="bf16"),        # N < 256: not the in-place kernel
    # (the in-place kernel's 32-bit offsets at K * N = 2^31: test_matmul_int8_transpose_path_at_the_offset_limit)
]

GRAD = [
    _c("grad", "grad_t+dense", M=300, N=1024, K=1000, dt="bf16", fmt="4bit", qt="nf4"),
    _c("grad", "grad_t+dense", M=257, N=640, K=384, dt="f16", fmt="int8", bad="x"),
    _c("grad", "grad_t+dense", M=256, N=512, K=520, dt="bf16", fmt="fp8"),
    _c("grad", "grad_t+dense_splitk", M=640, N=8192, K=2048, dt="bf16", fmt="4bit", qt="fp4", cs=True),
    _c("grad", "grad_generic", M=31, N=127, K=200, dt="f16", fmt="4bit", qt="nf4"),     # N % 64 != 0
    _c("grad", "grad_generic", M=7, N=100, K=72, dt="bf16", fmt="int8"),
    _c("grad_t", "grad_t", N=4160, K=1000, dt="f16", fmt="4bit", qt="fp4", bs=128, bad="w"),
    _c("grad_t", "grad_t", N=100, K=127, dt="bf16", fmt="4bit", qt="nf4", bs=8, cs=True),
    _c("grad_t", "grad_t", N=100, K=72, dt="bf16", fmt="int8"),
    _c("grad_t", "grad_t", N=256, K=128, dt="f16", fmt="fp8", bad="w"),
]

OUTLIER = [
    _c("outlier_linear", "i8_dense+outliers", M=2560, N=2560, K=512, dt="f16", n_out=21, bias=True),
    _c("outlier_linear", "i8_mfma256", M=2560, N=2560, K=512, dt="bf16", n_out=70, bias=True),     # > 64 outlier columns
    _c("outlier_linear", "i8_mfma128", M=300, N=777, K=1024, dt="bf16", n_out=5, bias=True),      # k_outlier_add
    _c("outlier_linear", "i8_generic", M=64, N=96, K=200, dt="f16", n_out=3),                     # K % 16 != 0, k_outlier_add
]

EMBEDDING = [
    _c("embedding_4bit", "embedding4", M=50, N=256, K=1000, dt="bf16", qt="nf4", bs=64),
    _c("embedding_8bit", "embedding8", M=50, N=256, K=1000, dt="f16"),
]

CASES = MATMUL_4BIT + LINEAR_8BIT + DENSE + MATMUL_INT8 + GRAD + OUTLIER + EMBEDDING


def case_id(c):
    dims = "x".join(str(v) for v in (c.get("lead") or (c.get("M"),)) if v is not None)
    opts = "-".join(f"{k}{'' if v is True else v}" for k, v in sorted(c.items())
                    if k not in ("op", "kernel", "M", "N", "K", "lead", "xfail") and v not in (None, False))
    return f"{c['op']}[{c['kernel'].strip()}]{dims}x{c.get('N')}x{c.get('K')}-{opts}"
