/*
 * mbnb_router.h — C ABI of the mixture-of-experts router of a decode batch (libmbnb_router.so): the router's
 * logits, the top-k selection and the softmax over the selected logits in ONE launch, so that the tensors mbnb_moemlp.h reads on
 * the device (`ids`, `rw`) are produced on the device too.
 *
 * A thirteenth library, with the conventions of the other twelve:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory, takes no workspace, owns no
 *     stream and keeps no per-call state;
 *   - the call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_router_last_error() returns a thread-local description of the last failure and
 *     mbnb_router_last_launch() the form of this thread's last successful launch.
 *
 * Alignment: x and w on 16 bytes; ids and logits_out on 4; bias and rw on their element size.
 */
#ifndef MBNB_ROUTER_H
#define MBNB_ROUTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_ROUTER_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_ROUTER_F16 = 0, MBNB_ROUTER_BF16 = 1, MBNB_ROUTER_F32 = 2 };

/* status codes (the values of mbnb_moemlp.h's) */
enum { MBNB_ROUTER_OK = 0, MBNB_ROUTER_ERR_ARG = -1, MBNB_ROUTER_ERR_SHAPE = -2 };

/* the most experts: mbnb_moemlp.h's limit; the workgroup keeps an f32 logit each in LDS, and one wave 16 candidates per lane */
#define MBNB_ROUTER_MAX_EXPERTS 1024
/* the most selected experts per token: slot a of a token is lane a of the wave that evaluates the softmax */
#define MBNB_ROUTER_MAX_TOPK 32
/* the widest activation row: the workgroup stages one row in LDS, 2 bytes an element, 32 KiB at this limit beside the 4 KiB of
 * logits, which leaves room for four workgroups on a compute unit's 160 KiB */
#define MBNB_ROUTER_MAX_K 16384

int mbnb_router_abi_version(void);
const char *mbnb_router_last_error(void);
/* e.g. "router bf16 E128 K2880 A4 T3"; "" before this thread's first launch */
const char *mbnb_router_last_launch(void);

/*
 * One launch, one workgroup per token.  x [T, K] of f16 or bf16 (x_dtype); w [E, K] of the same dtype, row-major; bias NULL or
 * [E] of bias_dtype (any of the three, read as f32); A = top_k.
 *
 *   l[t, e]   = f32( sum_k x[t, k] * w[e, k] ) + bias[e]     f32 accumulation of the exact products, then ONE f32 add of the bias
 *                                                           (none without a bias); NOT rounded to 16 bits
 *   rank      : a NaN (either sign) above everything, then by value with -0 == +0; equal keys: the LOWER expert index first
 *   ids[t, a] = the expert of rank a, a = 0 .. A - 1 (descending), int32
 *   v[a] = l[t, ids[t, a]];  d[a] = v[a] - v[0];  e[a] = expf(d[a]);  s = ((e[0] + e[1]) + e[2]) + ... in slot order;  w[a] = e[a] / s
 *   rw[t, a]  = w[a] rounded once to rw_dtype (any of the three)
 *
 * every operation a separate f32 rounding, the division IEEE, expf OCML's.  Inf and NaN follow IEEE arithmetic: a NaN logit is
 * selected first and makes all A weights of its token NaN; two +Inf among the selected give NaN; a selected -Inf beside a finite
 * maximum gets +0.  The summation order of l is fixed per (token, expert): it does not depend on T, on the token's place in the
 * call or on logits_out, so a token's ids, weights and logits are bit-equal alone and in any batch.
 *
 * logits_out is NULL or f32 [T, E]: the l above, the very values the selection ran on.  Every element of ids, rw and logits_out
 * is written exactly once.
 *
 * Refused (before any HIP call): x_dtype other than f16 / bf16, an unknown bias_dtype (with a bias) or rw_dtype:
 * MBNB_ROUTER_ERR_ARG; K not a positive multiple of 8 or over MBNB_ROUTER_MAX_K, E not in [1, MBNB_ROUTER_MAX_EXPERTS], A not in
 * [1, min(E, MBNB_ROUTER_MAX_TOPK)], T negative or over 2^31 - 1 (one launch's grid): MBNB_ROUTER_ERR_SHAPE; then, for T > 0, a
 * NULL x, w, ids or rw and a misaligned pointer: MBNB_ROUTER_ERR_ARG.  T == 0 is a no-op success with unread pointers.
 */
int mbnb_router_topk_softmax(const void *x, int64_t T, int64_t K, int x_dtype, const void *w, int64_t E, const void *bias,
                             int bias_dtype, int64_t A, int32_t *ids, void *rw, int rw_dtype, float *logits_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_ROUTER_H */
