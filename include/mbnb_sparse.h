/*
 * mbnb_sparse.h — C ABI of the two halves of the LLM.int8 decomposition (libmbnb_sparse.so): INT8 with column + row statistics
 * (quantize_colrow / dequantize_colrow / matmul_colrow) and the COO sparse operations (sparse_coo_from_dense, quantize_sparse_coo,
 * spmm_coo, spmm_coo_int8) of the reference's functional.py.
 *
 * A separate library from libmbnb_hip.so (whose ABI version 2 is frozen), with the same conventions:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, outputs and workspaces; the library never allocates, frees or retains device memory and
 *     keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation, no copy to the host);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch, >0 hipError_t);
 *     mbnb_sparse_last_error() returns a thread-local description of the last failure.
 *
 * The only cross-library call is libmbnb_hip.so's public mbnb_gemm_dense (with its workspace query and error text), on
 * matmul_colrow's dense route.  All tensors are dense, row-major, contiguous device tensors on the current HIP device.
 */
#ifndef MBNB_SPARSE_H
#define MBNB_SPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_SPARSE_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_SPARSE_F16 = 0, MBNB_SPARSE_BF16 = 1, MBNB_SPARSE_F32 = 2 };

/* status codes */
enum { MBNB_SPARSE_OK = 0, MBNB_SPARSE_ERR_ARG = -1, MBNB_SPARSE_ERR_SHAPE = -2, MBNB_SPARSE_ERR_UNSUPPORTED = -3 };

/* flags.
 * MBNB_SPARSE_PASS_ONLY (mbnb_colrow_matmul): run the first pass alone and write its result, Wd [N, K], into the output; for tests.
 * MBNB_SPARSE_FORCE_GENERIC: mbnb_colrow_matmul takes the generic kernel even where the dense route applies; mbnb_spmm_coo builds the
 * CSR form on the device even where the row indices are already non-decreasing. */
#define MBNB_SPARSE_PASS_ONLY 1
#define MBNB_SPARSE_FORCE_GENERIC 2

int mbnb_sparse_abi_version(void);
/* thread-local, never NULL; valid until the next failing call on this thread */
const char *mbnb_sparse_last_error(void);
/* name of the kernel route the last successful call on this thread took ("colrow_quantize8", "spmm_coo8", ...).
 * The pointer leads into a thread-local buffer that holds TWO strings: the name, its terminating NUL, then the VARIANT of the call
 * and a second NUL -- what the name does not say about the kernel forms that ran, "" where the launcher sets none:
 *   "wt"          colrow_dequant8 of a 16-bit dtype with write-through stores (matmul_colrow's dense route and its pass alone)
 *   "parts<n>"    coo_quantize: the number of partial maxima = workgroups, min(ceil(nnz / 2048), 1024)
 *   "G<g> x<t>"   spmm_coo*: g = 16 | 32 | 64 lanes per output row, t column tiles of g * (vector: 16 / sizeof(T), scalar: 4) columns
 * The variant of the "+dense" route's GEMM stays in mbnb_last_kernel()'s buffer.  A reader of the name alone sees what it always saw;
 * the variant is at `p + strlen(p) + 1`.  Valid until the next call on this thread. */
const char *mbnb_sparse_last_kernel(void);

/* ---------------------------------------------------------------------------
 * INT8 with column + row statistics (reference functional.py quantize_colrow / dequantize_colrow / matmul_colrow).  All in f32,
 * every operation correctly rounded, in the reference's order (x = float(tensor)):
 *   rm[i]    = max(max_j |x[i, j]|, 1e-8f)          cm[j] = max(max_i |x[i, j]|, 1e-8f)       (a NaN makes the statistic NaN)
 *   s[i, j]  = sqrt(rm[i] * cm[j])
 *   inv      = (1.0f / s[i, j]) * 127.0f                                   (torch's `127.0 / tensor`: reciprocal, then a product)
 *   q[i, j]  = int8(clamp(rint(x[i, j] * inv), -127, 127)),  0 where the product is NaN
 *   Wd[i, j] = round_T(float(q[i, j]) * (s[i, j] / 127.0f))                                                  (dequantize_colrow)
 *   y        = round_T(X . Wd^T + bias)                      (matmul_colrow: f32 accumulation, ONE rounding, the bias inside it)
 * sqrt is the correctly rounded one; torch's vectorised CPU sqrt is 1 ulp low on about 0.6 % of inputs.
 *
 * mbnb_colrow_quantize: x [R, C] of `dtype` -> q int8 [R, C], row_absmax f32 [R], col_absmax f32 [C].  The matrix is read twice: a
 * statistics kernel takes both maxima from one read (partial maxima per 16-row x 2048-column tile in the workspace, merged by a small
 * second kernel), the quantising kernel reads it again.  The workspace (mbnb_colrow_quantize_workspace_bytes, pure host code) is
 * required, 256-byte aligned.  Vector form (16-byte loads, 8 codes per store) where C % 8 == 0, x and col_absmax are 16-byte and q
 * 8-byte aligned; scalar form otherwise.  mbnb_sparse_last_kernel(): "colrow_quantize8" / "colrow_quantize1".
 * mbnb_colrow_dequantize: Wd [R, C] of `dtype`; vector form where C % 8 == 0, q 8-byte, col_scales and out 16-byte aligned.
 * "colrow_dequant8" / "colrow_dequant1".
 * mbnb_colrow_matmul: X [M, K], bias [N] or NULL, out [M, N] in T = `dtype`; W int8 [N, K], row_scales f32 [N], col_scales f32 [K].
 * Dispatch (SwitchBack's rule): 16-bit T, K % 64 == 0, K >= 128, M * N * K >= 2^27 and (M >= 16 or N * K >= 2^25), with X and out
 * 16-byte, W 8-byte and col_scales 16-byte aligned and a 256-byte aligned workspace of mbnb_colrow_matmul_workspace_bytes(...) bytes:
 * the dequantising pass writes Wd into the workspace, then mbnb_gemm_dense(X, Wd, bias, slices = 0) writes the output.  Everything else
 * (f32, small or ragged shapes, misalignment, no workspace, MBNB_SPARSE_FORCE_GENERIC) runs one generic kernel that decodes Wd on
 * the fly with the same rule.  A shorter workspace takes the generic kernel.  MBNB_SPARSE_PASS_ONLY:
 * the pass as the dense route runs it (write-through stores), Wd [N, K] into `out`.
 * "colrow_dq+dense" / "colrow_generic" / the pass's own name.
 * ------------------------------------------------------------------------- */
int64_t mbnb_colrow_quantize_workspace_bytes(int64_t R, int64_t C);
int mbnb_colrow_quantize(const void *x, int dtype, int64_t R, int64_t C, int8_t *q, float *row_absmax, float *col_absmax,
                         void *workspace, int64_t workspace_bytes, void *stream);
int mbnb_colrow_dequantize(const int8_t *q, const float *row_scales, const float *col_scales, int64_t R, int64_t C, int dtype,
                           void *out, void *stream);
int64_t mbnb_colrow_matmul_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype);
int mbnb_colrow_matmul(const void *X, int dtype, int64_t M, int64_t K, const int8_t *W, const float *row_scales,
                       const float *col_scales, int64_t N, const void *bias, void *out, void *workspace, int64_t workspace_bytes,
                       int flags, void *stream);

/* ---------------------------------------------------------------------------
 * sparse_coo_from_dense: the entries of x [R, C] kept by the reference's rule, in row-major order.  With v = x where threshold <= 0,
 * else v = x * (|x| >= threshold), an element is kept iff v != 0 and v is stored: -0.0 is dropped, +-Inf kept, NaN kept at any
 * threshold.  `threshold` is the caller's threshold already rounded to `dtype` (torch compares in the tensor's dtype).
 * mbnb_coo_count writes row_ptr int64 [R + 1], the exclusive scan of the per-row counts: row_ptr[R] is nnz, which the caller reads (the
 * operation's only host read) to size the outputs; mbnb_coo_fill then writes row / col int64 [nnz] and values [nnz] of `dtype`.
 * "coo_count" / "coo_fill".
 * ------------------------------------------------------------------------- */
int mbnb_coo_count(const void *x, int dtype, int64_t R, int64_t C, float threshold, int64_t *row_ptr, void *stream);
int mbnb_coo_fill(const void *x, int dtype, int64_t R, int64_t C, float threshold, const int64_t *row_ptr, int64_t *row, int64_t *col,
                  void *values, int64_t nnz, void *stream);

/* ---------------------------------------------------------------------------
 * quantize_sparse_coo: absmax = max(max |float(v)|, 1e-8f), scale[0] = absmax / 127.0f, q = int8(clamp(rint(float(v) / scale), -127,
 * 127)), 0 where the quotient is NaN.  nnz >= 1.  The maximum stays on the device: per-workgroup partial maxima in the workspace
 * (mbnb_coo_quantize_workspace_bytes(), a constant), merged by every workgroup of the quantising kernel.  "coo_quantize".
 * ------------------------------------------------------------------------- */
int64_t mbnb_coo_quantize_workspace_bytes(void);
int mbnb_coo_quantize(const void *values, int dtype, int64_t nnz, int8_t *q, float *scale, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* ---------------------------------------------------------------------------
 * spmm_coo / spmm_coo_int8:  out[i, n] = round_T( sum over entries e with row[e] == i of val(e) * float(dense[col[e], n]) ),
 * f32 accumulation in the order of the entry index e, ONE rounding; rows without entries are zeros.  dense [cols, N] and out [rows, N]
 * in T = `dtype`.  `value_kind`:
 *   MBNB_COO_VALUES       values [nnz] in T:                                       val(e) = float(values[e])
 *   MBNB_COO_INT8_SCALAR  values int8 [nnz], scale f32 [1]:                        val(e) = round_T(float(q[e]) * scale[0])
 *   MBNB_COO_INT8_ENTRY   values int8 [nnz], scale f32 [nnz]:                      val(e) = round_T(float(q[e]) * float(round_T(scale[e])))
 * row / col: int64 (`*_bits` = 64) or int32 (32), in any order, duplicates add.  An entry whose row is outside [0, rows) or whose column
 * is outside [0, cols) is skipped; nothing outside any buffer is read or written.
 * One kernel tests whether `row` is non-decreasing and leaves the answer in the first int32 of the workspace (0: it is).  If it is, row_ptr
 * comes from a binary search and the entries are used in place.  Otherwise (or with MBNB_SPARSE_FORCE_GENERIC) the CSR form is built on the
 * device: histogram of rows, exclusive scan, scatter, then each row's segment sorted by entry index, so the order of summation never depends
 * on the order atomics arrive in.  Both sets of kernels are launched and the one not wanted returns at once: the host never learns
 * the flag.  The workspace (mbnb_spmm_coo_workspace_bytes, pure host code) is required, 256-byte aligned; nnz and rows below 2^31 - 1.
 * Vector form (16-byte loads of dense rows) where N * sizeof(T) % 16 == 0 and dense and out are 16-byte aligned; scalar form otherwise.
 * "spmm_coo8" / "spmm_coo1"; with MBNB_SPARSE_FORCE_GENERIC "spmm_coo8_general" / "spmm_coo1_general".
 * ------------------------------------------------------------------------- */
enum { MBNB_COO_VALUES = 0, MBNB_COO_INT8_SCALAR = 1, MBNB_COO_INT8_ENTRY = 2 };
int64_t mbnb_spmm_coo_workspace_bytes(int64_t nnz, int64_t rows);
int mbnb_spmm_coo(const void *row, int row_bits, const void *col, int col_bits, const void *values, int value_kind, const float *scale,
                  int64_t nnz, const void *dense, int dtype, int64_t rows, int64_t cols, int64_t N, void *out, void *workspace,
                  int64_t workspace_bytes, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_SPARSE_H */
