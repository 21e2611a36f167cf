/*
 * mbnb_fp8blk.h — C ABI of the block-scaled FP8 linear on gfx950's FP8 MFMA (libmbnb_fp8blk.so).
 *
 * A seventeenth library, with the conventions of the other sixteen:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the workspace included; the library never allocates, frees or retains device
 *     memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_fp8blk_last_error() returns a thread-local description of the last failure and
 *     mbnb_fp8blk_last_launch() the form of this thread's last successful launch.
 *
 * The format is the block-scaled FP8 checkpoint layout (DeepSeek-V3 / R1, the Qwen3 -FP8 releases).  Both operands are OCP
 * E4M3 (e4m3fn, maximum 448) codes, one byte per element, row-major with K innermost.  With KB = ceil(K / 128) and
 * NB = ceil(N / 128):
 *   the weight      uint8 [N, K] with one f32 scale per 128 x 128 block, sW f32 [NB, KB] row-major: a checkpoint's
 *                   `weight_scale_inv` (weight_block_size = [128, 128]) as it lies in memory;
 *   the activation  uint8 [M, K] with one f32 scale per row and 128-wide k group, sA f32 [M, KB] row-major.
 * K % 16 == 0, so the last group of a row (the last block column) may be partial; the last block row may be too.
 *
 * The quantisers apply mbnb_fp8_quantize_rows' rule to one 1 x 128 group of a row (activation) or to one 128 x 128 block
 * (weight) instead of to a whole row, on the values read as f32:
 *   amax = max |x| of the group over the f32 bit patterns (an Inf or a NaN tops every finite value)
 *   s = amax / 448.0f, r = 448.0f / amax                           one IEEE f32 division each
 *   q = E4M3( f32(x) * r )                                         one f32 product, then round to nearest even, saturating at
 *                                                                  +-448, sign of zero kept, never the NaN code
 *   amax == 0: s = 0 and codes 0;  amax Inf or NaN: s = NaN and codes 0 (the outputs that the group reaches are NaN
 *   through the scale).
 *
 * The GEMM, for output (m, n) with nb = n / 128:
 *   p_t = sum over the k of block t of dec(a[m, k]) * dec(w[n, k])   one K-step of v_mfma_scale_f32_16x16x128_f8f6f4 with unit
 *                                                                    scale bytes into a ZERO accumulator, f32
 *   acc = fmaf(p_t, sA[m, t] * sW[nb, t], acc)                       t = 0 .. KB - 1 in order, acc starts at +0; the scale
 *                                                                    product is one f32 rounding, the fmaf one
 *   out[m, n] = round( bias ? acc + bias[n] : acc )                  one f32 addition, ONE rounding to out_dtype
 * Non-finite sA / sW / bias follow IEEE arithmetic: a NaN group scale poisons its row and no other row, a NaN block scale
 * its 128 columns and no other column.  An E4M3 NaN code (0x7F / 0xFF) in a or w is outside the contract: the call does
 * not fault, and outputs whose row and column hold no such code are not affected.
 *
 * The first mbnb_fp8blk_matmul / mbnb_fp8blk_linear call on a device raises the dynamic-LDS limit of every k_gemm_fp8_block
 * form (hipFuncSetAttribute, once per device and process): make that first call outside a stream capture.
 *
 * Alignment: x, a, w, q and the workspace on 16 bytes; sA, sW on 4; out and bias on their element size.
 */
#ifndef MBNB_FP8BLK_H
#define MBNB_FP8BLK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_FP8BLK_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_FP8BLK_F16 = 0, MBNB_FP8BLK_BF16 = 1, MBNB_FP8BLK_F32 = 2 };

/* status codes */
enum { MBNB_FP8BLK_OK = 0, MBNB_FP8BLK_ERR_ARG = -1, MBNB_FP8BLK_ERR_SHAPE = -2, MBNB_FP8BLK_ERR_WORKSPACE = -3 };

/* the scale block: 128 x 128 of the weight, 1 x 128 of the activation */
#define MBNB_FP8BLK_BLOCK 128
/* k_gemm_fp8_block: the workgroup's output tile (its columns lie in one block row of sW), its K-step (one scale group of
 * both operands) and the K-steps whose LDS-DMA is in flight at once */
#define MBNB_FP8BLK_TILE_M 128
#define MBNB_FP8BLK_TILE_N 128
#define MBNB_FP8BLK_K_STEP 128
#define MBNB_FP8BLK_STEPS_IN_FLIGHT 2

int mbnb_fp8blk_abi_version(void);
const char *mbnb_fp8blk_last_error(void);
/* e.g. "fp8_quant_groups bf16 5x4096", "fp8_quant_blocks f32 129x400", "gemm_fp8_block 128x128 33x261x1024" or the first and
 * the last joined by " + "; "" before the first launch */
const char *mbnb_fp8blk_last_launch(void);

/* x [M, K] of x_dtype -> q uint8 [M, K], sA f32 [M, KB] (k_fp8_quantize_groups).  M == 0 is a no-op success. */
int mbnb_fp8blk_quantize_groups(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, void *stream);

/* w [N, K] of w_dtype -> q uint8 [N, K], sW f32 [NB, KB] (k_fp8_quantize_blocks).  N == 0 is a no-op success. */
int mbnb_fp8blk_quantize_blocks(const void *w, int w_dtype, int64_t N, int64_t K, void *q, void *sW, void *stream);

/* out [M, N] of out_dtype from the codes and scales of both operands (k_gemm_fp8_block).  M == 0 is a no-op success. */
int mbnb_fp8blk_matmul(const void *a, const void *sA, int64_t M, int64_t K, const void *w, const void *sW, int64_t N,
                       const void *bias, int bias_dtype, void *out, int out_dtype, void *stream);

/* Bytes of workspace mbnb_fp8blk_linear needs: the activation's codes, then its scales, each rounded up to 256.  A negative
 * status for arguments the linear would refuse. */
int64_t mbnb_fp8blk_workspace_bytes(int64_t M, int64_t K);

/* mbnb_fp8blk_quantize_groups into the workspace, then mbnb_fp8blk_matmul over it: two launches, the bits of the two calls. */
int mbnb_fp8blk_linear(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N,
                       const void *bias, int bias_dtype, void *out, int out_dtype, void *workspace, int64_t workspace_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_FP8BLK_H */
