/*
 * mbnb_mx.h — C ABI of the OCP MX (microscaling) quantiser and the MXFP4 linear on gfx950's block-scaled MFMA
 * (libmbnb_mx.so).
 *
 * A tenth library, with the conventions of the other nine:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the workspace included; the library never allocates, frees or retains device
 *     memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_mx_last_error() returns a thread-local description of the last failure and
 *     mbnb_mx_last_launch() the form of this thread's last successful launch.
 *
 * The format.  An MX tensor is 2-D [rows, K] with K % 32 == 0, stored as element codes plus one E8M0
 * scale byte per block of 32 consecutive k: `scales` is uint8 [rows, K / 32], row-major; byte b means 2^(b - 127) and
 * 0xFF means NaN for the whole block.  Elements:
 *   MBNB_MX_FP4  E2M1 (magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6; sign in bit 3), two codes per byte with the EVEN k in the
 *                low nibble: uint8 [rows, K / 2];
 *   MBNB_MX_FP8  OCP E4M3 (e4m3fn, maximum 448), one byte per element: uint8 [rows, K].
 * Quantising a block: amax = max|v| over its f32 values, E = the biased exponent field of amax, byte = max(E - emax, 0)
 * with emax = 2 (fp4) or 8 (fp8); a block that holds a NaN or an Inf gets byte 0xFF and codes 0.  Each element is
 * v * 2^(127 - byte) (exact), rounded to the nearest element value, ties to the even code, saturating at +-6 / +-448; the
 * fp8 NaN code is never produced and the sign of zero is kept.  Decoding is value(code) * 2^(byte - 127), formed exactly
 * and rounded once (RNE, overflow to +-Inf) to the output dtype; byte 0xFF, and the fp8 NaN codes, give NaN.
 *
 * Alignment: x, codes, w_codes, the dequantiser's out and the workspace on 16 bytes; out and bias of mbnb_mx_linear and
 * mbnb_mx_linear_weight_only on their element size; scales need none.
 */
#ifndef MBNB_MX_H
#define MBNB_MX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MX_ABI_VERSION 2

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_MX_F16 = 0, MBNB_MX_BF16 = 1, MBNB_MX_F32 = 2 };

/* element formats */
enum { MBNB_MX_FP4 = 0, MBNB_MX_FP8 = 1 };

/* status codes */
enum { MBNB_MX_OK = 0, MBNB_MX_ERR_ARG = -1, MBNB_MX_ERR_SHAPE = -2, MBNB_MX_ERR_WORKSPACE = -3 };

/* k_gemm_mx: the workgroup's output tile and its K-step */
#define MBNB_MX_TILE_M 128
#define MBNB_MX_TILE_N 128
#define MBNB_MX_K_STEP 128

/* k_mx_decode: the most activation rows one workgroup pass of the weight-only linear serves */
#define MBNB_MX_DECODE_ROWS 16

int mbnb_mx_abi_version(void);
const char *mbnb_mx_last_error(void);
/* e.g. "mx_quant fp8 + gemm_mx fp8 128x128" or "mx_decode bf16 MT8"; "" before this thread's first launch */
const char *mbnb_mx_last_launch(void);

/* x [rows, K] of `dtype` -> codes, scales (k_mx_quantize).  rows == 0 is a no-op success. */
int mbnb_mx_quantize(const void *x, int64_t rows, int64_t K, int dtype, int elem, void *codes, void *scales, void *stream);

/* codes, scales -> out [rows, K] of `out_dtype` (k_mx_dequantize). */
int mbnb_mx_dequantize(const void *codes, const void *scales, int64_t rows, int64_t K, int elem, int out_dtype, void *out,
                       void *stream);

/* Bytes of workspace mbnb_mx_linear needs: the activation's codes plus its scale bytes, each rounded up to 256.
 * A negative status for arguments the linear would refuse. */
int64_t mbnb_mx_workspace_bytes(int64_t M, int64_t K, int act_elem);

/*
 * out[M, N] = Q(x[M, K]) . W^T + bias: Q quantises the activation rows to `act_elem` by the rule above into the
 * workspace (k_mx_quantize, the kernel of mbnb_mx_quantize), then k_gemm_mx runs the block-scaled MFMA over the codes
 * and scale bytes of both operands as they lie in memory.  The weight is always fp4: w_codes uint8 [N, K / 2],
 * w_scales uint8 [N, K / 32].  f32 accumulation by the MFMA, the bias (NULL: none; [N] of bias_dtype) added in f32, ONE
 * rounding to out_dtype.  A 0xFF scale byte of either operand makes every output of its row (activation) or column
 * (weight) NaN.  M == 0 is a no-op success.
 */
int mbnb_mx_linear(const void *x, int64_t M, int64_t K, int x_dtype, const void *w_codes, const void *w_scales, int64_t N,
                   int act_elem, const void *bias, int bias_dtype, void *out, int out_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream);

/*
 * out[M, N] = x[M, K] . W^T + bias over the MXFP4 weight as it lies in memory, the activation NOT quantised (k_mx_decode,
 * DESIGN.md §27).  One launch, no workspace:
 *   out[m, n] = round( sum_b 2^(s[n, b] - 127) * ( sum_{k in block b} x[m, k] * value(code[n, k]) ) + bias[n] )
 * with x read as f32, every sum in f32 (FMA), the scale applied to the block's partial sum, the bias added in f32 and ONE
 * rounding to out_dtype.  A 0xFF scale byte anywhere in weight row n makes out[:, n] NaN; Inf / NaN in x propagate as IEEE
 * arithmetic over the decoded weight does.  Any M >= 0 (M == 0: no-op success); a workgroup pass serves up to
 * MBNB_MX_DECODE_ROWS rows (half as many f32 rows), rows beyond that run as further row chunks of the same launch, which
 * stream the weight again.  The conventions and checks are mbnb_mx_linear's.
 */
int mbnb_mx_linear_weight_only(const void *x, int64_t M, int64_t K, int x_dtype, const void *w_codes, const void *w_scales,
                               int64_t N, const void *bias, int bias_dtype, void *out, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MX_H */
