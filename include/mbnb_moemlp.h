/*
 * mbnb_moemlp.h — C ABI of the MXFP4 mixture-of-experts MLP of a decode batch (libmbnb_moemlp.so): the gate / up
 * projection with the gated activation as its epilogue, and the down projection with the routed, weighted sum over a token's
 * slots, both on a grid sized by the routing.
 *
 * A twelfth library, with the conventions of the other eleven:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the workspace included; the library never allocates, frees or retains device
 *     memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation): the expert ids and the routing weights are read
 *     ON THE DEVICE, so a captured graph serves a new routing once both tensors are overwritten in place;
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_moemlp_last_error() returns a thread-local description of the last failure and
 *     mbnb_moemlp_last_launch() the form of this thread's last successful call.
 *
 * The weight format is mbnb_mx.h's MXFP4, experts stacked as in mbnb_moe.h: w_codes uint8 [E, N, K / 2] (E2M1, the even k in
 * the low nibble), w_scales uint8 [E, N, K / 32] (E8M0; 0xFF means NaN for the block), K % 32 == 0.
 *
 * P = T * A (token, slot) pairs, pair p = t * A + a, e = ids[p] (int32 [T, A]).  `pre` below is the f32 value
 *   sum_b 2^(s[e, n, b] - 127) * ( sum_{k in block b} row(p)[k] * value(code[e, n, k]) ) + bias[e, n]
 * with the bits mbnb_moe_mxfp4_experts writes for out_dtype f32: the same K walk, so a pair's bits do not depend on what
 * else is in the call.  A pair whose id is outside [0, E) (-1 pads; any int32 is legal) is skipped: nothing but its id is
 * read for it.
 *
 * Both expert launches run ceil(N / 16) x R workgroups, R = min(E, P): grid row j serves the j-th smallest distinct id in
 * [0, E) of the call, which it finds itself, and leaves at once when there are fewer.
 *
 * Alignment: x, h, w_codes and workspace on 16 bytes; ids on 4; out, bias and rw on their element size; w_scales none.
 */
#ifndef MBNB_MOEMLP_H
#define MBNB_MOEMLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MOEMLP_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_MOEMLP_F16 = 0, MBNB_MOEMLP_BF16 = 1, MBNB_MOEMLP_F32 = 2 };

/* status codes (the values of mbnb_moe.h's, and the workspace status of mbnb_mx.h) */
enum { MBNB_MOEMLP_OK = 0, MBNB_MOEMLP_ERR_ARG = -1, MBNB_MOEMLP_ERR_SHAPE = -2, MBNB_MOEMLP_ERR_WORKSPACE = -3 };

/* the most (token, slot) pairs of one call: the workgroup's pair list in LDS holds 2 bytes each */
#define MBNB_MOEMLP_MAX_PAIRS 1024
/* the most experts: the workgroup's presence array in LDS holds a byte each */
#define MBNB_MOEMLP_MAX_EXPERTS 1024

int mbnb_moemlp_abi_version(void);
const char *mbnb_moemlp_last_error(void);
/* e.g. "mx_glu bf16 E32 P4 R4" or "mx_down_sum f16 E9 P64 R9 A4"; "" before this thread's first launch */
const char *mbnb_moemlp_last_launch(void);

/*
 * One launch.  x [T, K] of f16 or bf16, shared by a token's slots; w_codes / w_scales [E, 2I, K / 2] / [E, 2I, K / 32] with
 * the rows interleaved: row 2j is gate j, row 2j + 1 is up j; bias NULL or [E, 2I] of bias_dtype, interleaved the same way.
 *   g = pre[p, 2j], u = pre[p, 2j + 1]
 *   g = g > limit ? limit : g;   u = u > limit ? limit : (u < -limit ? -limit : u)            (a NaN stays a NaN)
 *   out[p, j] = round( (u + 1) * (g * (1 / (1 + expf(-(alpha * g))))) )
 * every operation a separate f32 rounding, the division IEEE, ONE rounding to out_dtype (any of the three); out is [T, A, I].
 * alpha must be finite; limit > 0, +Inf included.  A pair whose id is outside [0, E) gets a row of +0.0.  A 0xFF scale byte in
 * gate row 2j or up row 2j + 1 of expert e makes out[p, j] NaN for every pair routed to e and for no other.  Every element
 * of out is written exactly once.  T * A <= MBNB_MOEMLP_MAX_PAIRS; T * A == 0 is a no-op success with unread pointers.
 */
int mbnb_moemlp_gate_up_glu(const void *x, int64_t T, int64_t A, int64_t K, int x_dtype,
                            const void *w_codes, const void *w_scales, int64_t E, int64_t I,
                            const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit,
                            void *out, int out_dtype, void *stream);

/* T * A * N * 4 bytes rounded up to 256; MBNB_MOEMLP_ERR_SHAPE for sizes mbnb_moemlp_down_sum refuses */
int64_t mbnb_moemlp_workspace_bytes(int64_t T, int64_t A, int64_t N);

/*
 * Two launches.  h [T, A, K] of f16 or bf16, a row per pair; w_codes / w_scales [E, N, K / 2] / [E, N, K / 32]; bias NULL or
 * [E, N]; rw [T, A] of rw_dtype (any of the three, read as f32).  The first launch stores y[p, n] = pre[p, n] (f32, not
 * rounded) into the workspace for every pair whose id is in [0, E); the second evaluates, one thread per output,
 *   acc = +0.0;  for a = 0 .. A - 1 in this order, pairs with an id outside [0, E) skipped:  acc = fmaf(rw[t, a], y[t * A + a, n], acc)
 *   out[t, n] = round(acc)
 * to out_dtype; out is [T, N].  Neither rw nor the workspace is read for a skipped pair; a token whose slots are all skipped
 * gets a row of +0.0.  A 0xFF scale byte in row n of expert e makes out[t, n] NaN for exactly the tokens that route a slot
 * to e.  Every element of out is written exactly once.  The workspace holds at least
 * mbnb_moemlp_workspace_bytes(T, A, N) bytes (else MBNB_MOEMLP_ERR_WORKSPACE); its contents are undefined afterwards.
 */
int mbnb_moemlp_down_sum(const void *h, int64_t T, int64_t A, int64_t K, int h_dtype,
                         const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                         const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype,
                         void *out, int out_dtype, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MOEMLP_H */
