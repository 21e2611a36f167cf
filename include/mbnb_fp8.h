/*
 * mbnb_fp8.h — C ABI of the W8A8 FP8 linear on gfx950's FP8 MFMA (libmbnb_fp8.so).
 *
 * A sixteenth library, with the conventions of the other fifteen:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the workspace included; the library never allocates, frees or retains device
 *     memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_fp8_last_error() returns a thread-local description of the last failure and
 *     mbnb_fp8_last_launch() the form of this thread's last successful launch.
 *
 * Both operands are OCP E4M3 (e4m3fn, maximum 448) codes, one byte per element, row-major with K innermost: the
 * activation uint8 [M, K] with one f32 scale per row, the weight uint8 [N, K] with one f32 scale per row.  A
 * LinearFP8.weight buffer is such a weight as it lies in memory.
 *
 * The row quantiser, on the values of a row read as f32 (K % 16 == 0):
 *   amax = max_k |x[m, k]| over the f32 bit patterns (an Inf or a NaN tops every finite value)
 *   sA[m] = amax / 448.0f, r = 448.0f / amax                       one IEEE f32 division each
 *   q[m, k] = E4M3( f32(x[m, k]) * r )                             one f32 product, then round to nearest even,
 *                                                                  saturating at +-448, sign of zero kept, never the NaN code
 *   amax == 0: sA[m] = 0 and codes 0;  amax Inf or NaN: sA[m] = NaN and codes 0 (the output row is NaN through the scale).
 *
 * The GEMM:
 *   acc[m, n] = sum_k dec(a[m, k]) * dec(w[n, k])                  v_mfma_scale_f32_16x16x128_f8f6f4, unit scales, f32
 *   out[m, n] = round( (acc * sA[m]) * sW[n] + bias[n] )           each operation one f32 rounding, ONE rounding to out_dtype;
 *                                                                  bias NULL: no addition
 * Non-finite sA / sW / bias follow IEEE arithmetic.  An E4M3 NaN code (0x7F / 0xFF) in a or w is outside the contract: the
 * call does not fault, and outputs whose row and column hold no such code are not affected.
 *
 * The first mbnb_fp8_matmul / mbnb_fp8_linear call on a device raises the dynamic-LDS limit of every k_gemm_fp8 form
 * (hipFuncSetAttribute, once per device and process): make that first call outside a stream capture.
 *
 * Alignment: x, a, w, q and the workspace on 16 bytes; sA, sW on 4; out and bias on their element size.
 */
#ifndef MBNB_FP8_H
#define MBNB_FP8_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_FP8_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_FP8_F16 = 0, MBNB_FP8_BF16 = 1, MBNB_FP8_F32 = 2 };

/* status codes */
enum { MBNB_FP8_OK = 0, MBNB_FP8_ERR_ARG = -1, MBNB_FP8_ERR_SHAPE = -2, MBNB_FP8_ERR_WORKSPACE = -3 };

/* k_gemm_fp8: the workgroup's output tile (the narrow one where the wide grid would not fill the chip), its K-step and
 * the K-steps whose LDS-DMA is in flight at once */
#define MBNB_FP8_TILE_M 256
#define MBNB_FP8_TILE_N 256
#define MBNB_FP8_TILE_N_NARROW 128
#define MBNB_FP8_K_STEP 128
#define MBNB_FP8_STEPS_IN_FLIGHT 2
/* the wide tile is taken from this many wide tiles up (one per compute unit of an MI355X) */
#define MBNB_FP8_WIDE_TILES 256

int mbnb_fp8_abi_version(void);
const char *mbnb_fp8_last_error(void);
/* e.g. "fp8_quant_rows bf16 5x4096", "gemm_fp8 256x128 33x261x1024" or both joined by " + "; "" before the first launch */
const char *mbnb_fp8_last_launch(void);

/* x [M, K] of x_dtype -> q uint8 [M, K], sA f32 [M] (k_fp8_quantize_rows).  M == 0 is a no-op success. */
int mbnb_fp8_quantize_rows(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, void *stream);

/* out [M, N] of out_dtype from the codes and scales of both operands (k_gemm_fp8).  M == 0 is a no-op success. */
int mbnb_fp8_matmul(const void *a, const void *sA, int64_t M, int64_t K, const void *w, const void *sW, int64_t N,
                    const void *bias, int bias_dtype, void *out, int out_dtype, void *stream);

/* Bytes of workspace mbnb_fp8_linear needs: the activation's codes, then its scales, each rounded up to 256.  A negative
 * status for arguments the linear would refuse. */
int64_t mbnb_fp8_workspace_bytes(int64_t M, int64_t K);

/* mbnb_fp8_quantize_rows into the workspace, then mbnb_fp8_matmul over it: two launches, the bits of the two calls. */
int mbnb_fp8_linear(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N,
                    const void *bias, int bias_dtype, void *out, int out_dtype, void *workspace, int64_t workspace_bytes,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_FP8_H */
