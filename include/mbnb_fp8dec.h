/*
 * mbnb_fp8dec.h — C ABI of the weight-only decode linear over a block-scaled FP8 weight (libmbnb_fp8dec.so).
 *
 * An eighteenth library, with the conventions of the other seventeen:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory, owns no stream, needs no
 *     workspace and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation): ONE launch;
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_fp8dec_last_error() returns a thread-local description of the last failure and
 *     mbnb_fp8dec_last_launch() the form of this thread's last successful launch.
 *
 * The weight is mbnb_fp8blk.h's: `w` uint8 [N, K] of OCP E4M3 (e4m3fn) codes, row-major with K innermost, and `sW` f32
 * [ceil(N / 128), ceil(K / 128)] row-major, a checkpoint's `weight_scale_inv`.  K % 16 == 0, so the last block column and the
 * last block row may be partial.  The activation `x` [M, K] of bf16 / f16 / f32 is NOT quantised: the weight is streamed once
 * and decoded in registers, for the 1 to 16 rows of a token-generation step (more rows run as further row chunks of the launch).
 *
 * For output (m, n), with block t the k in [128 t, min(128 t + 128, K)):
 *   p_t      = sum over the k of block t of x[m, k] * dec(w[n, k])      f32, in any order; x read as f32
 *   acc      = sum over t of sW[n / 128, t] * p_t                        the scale multiplies the block's PARTIAL SUM: f32 fma, any
 *                                                                        order over t (and over parts of a block's sum)
 *   out[m, n] = round( bias ? acc + bias[n] : acc )                      one f32 addition, ONE rounding to out_dtype (round to
 *                                                                        nearest even, overflow to +-Inf)
 * For 16-bit x every product x * dec(w) is exact in f32 (an 8- or 11-bit significand times a 4-bit one), so on operands whose
 * sums are exact too the result is the real-number chain rounded once, whatever the order.
 *
 * Non-finite x, sW and bias follow IEEE arithmetic: a NaN or an Inf in row m of x touches row m only; a NaN sW[nb, t] touches the
 * 128 columns of block row nb, in every row, and no other column.  An E4M3 NaN code (0x7F / 0xFF) in w is outside the contract:
 * the call does not fault, and columns without such a code are not affected.
 *
 * The form is chosen by the row count and the dtype of x: k_fp8_block_decode_mfma (16-bit x, 2 rows and more: the
 * v_mfma_f32_16x16x32 instructions, 16 rows a chunk) or k_fp8_block_decode (one 16-bit row, and every f32 call: FMAs, 1 / 2 / 4 rows
 * a chunk).
 *
 * Alignment: x and w on 16 bytes; sW on 4; out and bias on their element size.
 */
#ifndef MBNB_FP8DEC_H
#define MBNB_FP8DEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_FP8DEC_ABI_VERSION 1

/* element dtypes and status codes: the values of mbnb_fp8blk.h */
enum { MBNB_FP8DEC_F16 = 0, MBNB_FP8DEC_BF16 = 1, MBNB_FP8DEC_F32 = 2 };
enum { MBNB_FP8DEC_OK = 0, MBNB_FP8DEC_ERR_ARG = -1, MBNB_FP8DEC_ERR_SHAPE = -2 };

/* the scale block's edge, and the weight rows (and the activation rows of a chunk) of a k_fp8_block_decode_mfma workgroup */
#define MBNB_FP8DEC_BLOCK 128
#define MBNB_FP8DEC_ROWS 16

int mbnb_fp8dec_abi_version(void);
const char *mbnb_fp8dec_last_error(void);
/* e.g. "fp8_block_decode bf16 MT1 1x4096x4096", "fp8_block_decode f32 MT4 5x129x400" or
 * "fp8_block_decode_mfma bf16 MT16 8x4096x4096" (rows of a chunk, then M x N x K); "" before the first launch */
const char *mbnb_fp8dec_last_launch(void);

/* out [M, N] of out_dtype = x [M, K] . dec(w)^T under sW, + bias.  M == 0 is a no-op success.  A launch of more than 2^31 - 1
 * workgroups is refused. */
int mbnb_fp8dec_linear_weight_only(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N,
                                   const void *bias, int bias_dtype, void *out, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_FP8DEC_H */
