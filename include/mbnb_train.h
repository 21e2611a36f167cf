/*
 * mbnb_train.h — C ABI of the trainable-weight linears (libmbnb_train.so): SwitchBackLinear's int8 forward and the weight
 * gradient dW = dY^T . X.
 *
 * A separate library from libmbnb_hip.so (whose ABI version 2 is frozen), with the same conventions:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, outputs and workspaces; the library never allocates, frees or retains device memory and
 *     keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch, >0 hipError_t);
 *     mbnb_train_last_error() returns a thread-local description of the last failure.
 *
 * The MFMA work is libmbnb_hip.so's public mbnb_gemm_dense with slices = 0 (that library's own plan); this library adds the passes
 * around it and the generic kernels.  All tensors are dense, row-major, contiguous device tensors on the current HIP device.
 */
#ifndef MBNB_TRAIN_H
#define MBNB_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_TRAIN_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_TRAIN_F16 = 0, MBNB_TRAIN_BF16 = 1, MBNB_TRAIN_F32 = 2 };

/* status codes */
enum { MBNB_TRAIN_OK = 0, MBNB_TRAIN_ERR_ARG = -1, MBNB_TRAIN_ERR_SHAPE = -2, MBNB_TRAIN_ERR_UNSUPPORTED = -3 };

/* flags of both operations.
 * MBNB_TRAIN_PASS_ONLY: run the first pass alone and write its result into the output (see each operation), for tests.
 * MBNB_TRAIN_FORCE_GENERIC: take the generic kernel even where the dense route applies. */
#define MBNB_TRAIN_PASS_ONLY 1
#define MBNB_TRAIN_FORCE_GENERIC 2

int mbnb_train_abi_version(void);
/* thread-local, never NULL; valid until the next failing call on this thread */
const char *mbnb_train_last_error(void);
/* name of the kernel route the last successful call on this thread took ("switchback_dq+dense", "grad_w_generic", ...).
 * The pointer leads into a thread-local buffer that holds TWO strings: the name, its terminating NUL, then the VARIANT of the call
 * and a second NUL -- the kernel forms that ran behind the name, as words joined by blanks, "" where the launcher sets none:
 *   the Wd pass          "dq8x4" (vector form, 4 rows per thread: N K <= 2^25 and (N + 3) / 4 <= 65535) | "dq8x1" (one row: N <= 65535) |
 *                        "dq1" (scalar: f32, K % 8 != 0, W off 8 or the output off 16 bytes, or N > 65535)
 *   the bias pass        "bias8" (N % 8 == 0 and a 16-byte aligned bias) | "bias1" | "nobias", behind the Wd pass's word
 *   the transposing pass "dy8" | "dy1" for dY, "x8" | "x1" for X (8: C % 8 == 0 and a 16-byte aligned operand)
 * so "dq8x4 bias8", "dy1 x8", "x1" (the pass alone).  The generic kernels set none; the variant of a "+dense" route's GEMM stays in
 * mbnb_last_kernel()'s buffer.  A reader of the name alone sees what it always saw; the variant is at `p + strlen(p) + 1`.  Valid
 * until the next call on this thread. */
const char *mbnb_train_last_kernel(void);

/* ---------------------------------------------------------------------------
 * SwitchBackLinear.forward (reference nn/switchback.py, SwitchBackFunction.forward), T = `dtype`:
 *   Wd[n, k]  = round_T( q[n, k] * round_T(scales[n] / 127.0f) )        -- the weight rounded TWICE, not dequantize_rowwise
 *   out[m, n] = round_T( round_T(X[m, :] . Wd[n, :]) + bias[n] )          -- torch.mm, then the bias as a separate add
 * X [M, K], bias [N] (or NULL), out [M, N] in T (f16 / bf16 / f32); W int8 [N, K], scales f32 [N]; f32 accumulation.
 * Dispatch.  16-bit T, K % 64 == 0, K >= 128, M * N * K >= 2^27 and (M >= 16 or N * K >= 2^25), with X 16-byte aligned, W 8-byte
 * aligned and a 256-byte aligned workspace of mbnb_switchback_forward_workspace_bytes(...) bytes: a pass writes Wd [N, K] into the workspace, then
 * mbnb_gemm_dense(X, Wd, bias = NULL, slices = 0) writes round_T(X . Wd^T) and, with a bias, an in-place pass adds it.  Everything else
 * (f32, small products, K % 64 != 0, misalignment, no workspace) runs one generic kernel that decodes Wd on the fly with the same rule.
 * The query is pure host code: Wd's bytes (rounded up to 256) plus the GEMM's split-K share where the dense route applies, else 0.
 * MBNB_TRAIN_PASS_ONLY: write Wd [N, K] of `dtype` into `out` (X, M, bias and the workspace are ignored); any K, all three dtypes.
 * mbnb_train_last_kernel(): "switchback_dq+dense" / "switchback_generic" / "switchback_dq" (the pass alone).
 * ------------------------------------------------------------------------- */
int64_t mbnb_switchback_forward_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype);
int mbnb_switchback_forward(const void *X, int dtype, int64_t M, int64_t K, const int8_t *W, const float *scales, int64_t N,
                            const void *bias, void *out, void *workspace, int64_t workspace_bytes, int flags, void *stream);

/* ---------------------------------------------------------------------------
 * Weight gradient of a linear, the contraction over the token dimension M:
 *   dW[n, k] = round_T( sum_m dY[m, n] * X[m, k] )
 * dY [M, N], X [M, K], dW [N, K] in T = `dtype` (f16 / bf16 / f32); f32 accumulation, one rounding.  M >= 0 (M = 0 gives zeros).
 * Dispatch.  16-bit T where M * N * K > 2^26, Mp = mbnb_train_padded_rows(M), with a 256-byte aligned workspace of
 * mbnb_linear_grad_weight_workspace_bytes(...) bytes: two transposing passes write dY^T [N, Mp] and X^T [K, Mp] into the workspace,
 * columns M .. Mp-1 as zeros (they add exact zeros to the sums), then mbnb_gemm_dense(dY^T, X^T, M = N, N = K, K = Mp, ldw = Mp,
 * slices = 0) writes dW.  Everything else (f32, small products, no workspace) runs a generic kernel.  Any alignment of dY and X.
 * The query is pure host code: the two transposed operands (each rounded up to 256 bytes) plus the GEMM's split-K share, else 0.
 * MBNB_TRAIN_PASS_ONLY: the transposing pass alone on X: X [M, K] goes to dW as X^T [K, Mp] with zero columns M .. Mp-1 (dY and N are
 * ignored; 16-bit T only).
 * mbnb_train_last_kernel(): "grad_w_t+dense" / "grad_w_generic" / "grad_w_t" (the pass alone).
 * ------------------------------------------------------------------------- */
/* Mp: M rounded up to a multiple of 64, at least 128 */
int64_t mbnb_train_padded_rows(int64_t M);
int64_t mbnb_linear_grad_weight_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype);
int mbnb_linear_grad_weight(const void *dY, const void *X, int64_t M, int64_t N, int64_t K, int dtype, void *dW, void *workspace,
                            int64_t workspace_bytes, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_TRAIN_H */
