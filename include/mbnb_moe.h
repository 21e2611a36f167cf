/*
 * mbnb_moe.h — C ABI of the MXFP4 expert linears of a mixture-of-experts layer (libmbnb_moe.so).
 *
 * An eleventh library, with the conventions of the other ten:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory, owns no stream and
 *     keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation): the expert ids are read ON THE DEVICE, so a
 *     captured graph serves a new routing once the ids tensor is overwritten in place;
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_moe_last_error() returns a thread-local description of the last failure and
 *     mbnb_moe_last_launch() the form of this thread's last successful launch.
 *
 * The weight format is mbnb_mx.h's MXFP4, one tensor per expert, experts stacked: w_codes uint8
 * [E, N, K / 2] (E2M1, two codes per byte, the even k in the low nibble), w_scales uint8 [E, N, K / 32] (E8M0: byte b
 * means 2^(b - 127), 0xFF means NaN for the block), K % 32 == 0.  These are the bytes of a checkpoint's
 * [E, N, K / 32, 16] blocks and [E, N, K / 32] scales.
 *
 * Alignment: x and w_codes on 16 bytes (K % 32 == 0 then puts every expert's codes on 16 bytes); ids on 4; out and bias
 * on their element size; w_scales need none.
 */
#ifndef MBNB_MOE_H
#define MBNB_MOE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MOE_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_MOE_F16 = 0, MBNB_MOE_BF16 = 1, MBNB_MOE_F32 = 2 };

/* status codes (the values of mbnb_mx.h's) */
enum { MBNB_MOE_OK = 0, MBNB_MOE_ERR_ARG = -1, MBNB_MOE_ERR_SHAPE = -2 };

/* the most (token, slot) pairs of one launch: the workgroup's pair list in LDS holds 2 bytes each */
#define MBNB_MOE_MAX_PAIRS 1024

int mbnb_moe_abi_version(void);
const char *mbnb_moe_last_error(void);
/* e.g. "mx_experts bf16 shared E32 P64" or "mx_experts f16 slot E4 P5"; "" before this thread's first launch */
const char *mbnb_moe_last_launch(void);

/*
 * One launch of k_mx_experts: P = T * A pairs, pair p = t * A + a, e = ids[p] (int32 [T, A], read on the device).
 *   out[p, n] = round( sum_b 2^(s[e, n, b] - 127) * ( sum_{k in block b} x_row(p)[k] * value(code[e, n, k]) ) + bias[e, n] )
 * with x_row(p) = x[t] of x [T, K] (x_per_slot == 0: every slot of a token shares its row) or x[t, a] of x [T, A, K]
 * (x_per_slot != 0), x of f16 or bf16 (x_dtype; f32 is refused), f32 accumulation with the scale applied to the block's
 * partial sum, the bias (NULL: none; [E, N] of bias_dtype) added in f32 and ONE rounding to out_dtype (any of the three);
 * out is [T, A, N].  The bits of a pair do not depend on the other pairs of the call: they are those of
 * mbnb_mx_linear_weight_only for that row against expert e in its MFMA form.  A 0xFF scale byte anywhere in row n of
 * expert e makes out[p, n] NaN for every pair routed to e and for no other.  A pair whose id is outside [0, E) (-1 is the
 * padding value; any int32 is legal) gets a row of +0.0 and no bias, and nothing but its id is read for it.  Every element
 * of out is written exactly once.  T * A <= MBNB_MOE_MAX_PAIRS; T * A == 0 is a no-op success with unread pointers.
 */
int mbnb_moe_mxfp4_experts(const void *x, int64_t T, int64_t A, int x_per_slot, int64_t K, int x_dtype,
                           const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                           const int32_t *ids, const void *bias, int bias_dtype,
                           void *out, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MOE_H */
