/*
 * mbnb_moegemm.h — C ABI of the prefill-sized grouped GEMM over MXFP4 experts (libmbnb_moegemm.so): the three
 * expert projections of mbnb_moe.h and mbnb_moemlp.h for any number of (token, slot) pairs in one launch each, every expert's
 * pairs taken MBNB_MOEGEMM_ROW_TILE at a time against one decode of the weight tile, with the bits of the decode launches.
 *
 * A fourteenth library, with the conventions of the other thirteen:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the plan and the workspace included; the library never allocates, frees or retains
 *     device memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation): the expert ids and the routing weights are read
 *     ON THE DEVICE, the plan is built there, so a captured graph serves a new routing once the tensors are overwritten in place;
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_moegemm_last_error() returns a thread-local description of the last failure and
 *     mbnb_moegemm_last_launch() the form of this thread's last successful call.
 *
 * The weight format is mbnb_mx.h's MXFP4, experts stacked as in mbnb_moe.h: w_codes uint8 [E, N, K / 2] (E2M1, the even k in
 * the low nibble), w_scales uint8 [E, N, K / 32] (E8M0; 0xFF means NaN for the block), K % 32 == 0.
 *
 * P = T * A (token, slot) pairs, pair p = t * A + a, e = ids[p] (int32 [T, A]).  `pre` below is the f32 value
 *   sum_b 2^(s[e, n, b] - 127) * ( sum_{k in block b} row(p)[k] * value(code[e, n, k]) ) + bias[e, n]
 * with EXACTLY the bits mbnb_moe_mxfp4_experts writes for out_dtype f32: per MX block one v_mfma_f32_16x16x32 onto a zero
 * accumulator and acc = fmaf(d, scale, acc); wave w of eight takes the k-steps w, w + 8, ... of four blocks in block order; the
 * eight partial sums are added from +0.0 in wave order; the bias is added in f32; a column that met a 0xFF scale byte is NaN.
 * A pair whose id is outside [0, E) (-1 pads; any int32 is legal) is skipped: nothing but its id is read for it.
 *
 * THE PLAN.  mbnb_moegemm_plan builds, in two small launches and without a host round trip, a function of the ids alone,
 * as int32 words in this order (R = MBNB_MOEGEMM_ROW_TILE, max_tiles = min(E, P) + P / R):
 *   counts[E]            the pairs routed to each expert
 *   n_tiles, n_listed    the entries of the tile table in use, and the pairs with an id in [0, E)
 *   tiles[max_tiles][3]  (expert, first index into sorted, rows <= R): expert e owns ceil(counts[e] / R) consecutive entries,
 *                        experts ascending; the entries past n_tiles are not written
 *   sorted[P]            pair indices: the listed pairs grouped by expert, experts ascending, pair indices ascending within
 *                        an expert; then the pairs with an id outside [0, E), ascending
 * The three projection calls read a plan that mbnb_moegemm_plan built from the SAME ids, P and E on the same stream (or
 * ordered before them); they launch ceil(N / (16 NT)) x max_tiles workgroups, and those past n_tiles leave before they touch
 * a weight byte.
 *
 * Alignment: x, h, w_codes, plan and workspace on 16 bytes; ids on 4; out, bias and rw on their element size; w_scales none.
 */
#ifndef MBNB_MOEGEMM_H
#define MBNB_MOEGEMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MOEGEMM_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_MOEGEMM_F16 = 0, MBNB_MOEGEMM_BF16 = 1, MBNB_MOEGEMM_F32 = 2 };

/* status codes (the values of mbnb_moemlp.h's); a short plan is a short workspace */
enum { MBNB_MOEGEMM_OK = 0, MBNB_MOEGEMM_ERR_ARG = -1, MBNB_MOEGEMM_ERR_SHAPE = -2, MBNB_MOEGEMM_ERR_WORKSPACE = -3 };

/* the listed pairs of one expert that a workgroup takes against one decode of its weight tile: a multiple of 16 */
#define MBNB_MOEGEMM_ROW_TILE 64
/* the most experts */
#define MBNB_MOEGEMM_MAX_EXPERTS 1024
/* the most (token, slot) pairs of one call */
#define MBNB_MOEGEMM_MAX_PAIRS 1048576

int mbnb_moegemm_abi_version(void);
const char *mbnb_moegemm_last_error(void);
/* e.g. "mx_plan E32 P4096 R64", "mx_grouped bf16 shared E32 P4096 R64", "mx_grouped_glu bf16 E32 P4096 R64" or
 * "mx_grouped_down_sum f16 E9 P64 R64 A4"; "" before this thread's first launch */
const char *mbnb_moegemm_last_launch(void);

/* 4 * (E + 2 + 3 * max_tiles + P) bytes rounded up to 256; MBNB_MOEGEMM_ERR_SHAPE unless 0 <= P <= MBNB_MOEGEMM_MAX_PAIRS and
 * 1 <= E <= MBNB_MOEGEMM_MAX_EXPERTS */
int64_t mbnb_moegemm_plan_bytes(int64_t P, int64_t E);

/*
 * Two launches: the plan of ids [P] over E experts into plan (at least mbnb_moegemm_plan_bytes(P, E) bytes, else
 * MBNB_MOEGEMM_ERR_WORKSPACE).  Every word a projection call reads is written here.  P == 0 is a no-op success.
 */
int mbnb_moegemm_plan(const int32_t *ids, int64_t P, int64_t E, void *plan, int64_t plan_bytes, void *stream);

/*
 * One launch: mbnb_moe_mxfp4_experts.  x [T, K] (x_per_slot == 0: shared by a token's slots) or [T, A, K] (a row per pair) of
 * f16 or bf16; bias NULL or [E, N]; out [T, A, N] = round(pre) to out_dtype (any of the three), a pair whose id is outside
 * [0, E) a row of +0.0.  Every element of out is written exactly once.  T * A <= MBNB_MOEGEMM_MAX_PAIRS; T * A == 0 is a
 * no-op success with unread pointers.
 */
int mbnb_moegemm_experts(const void *x, int64_t T, int64_t A, int x_per_slot, int64_t K, int x_dtype,
                         const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                         const int32_t *ids, const void *bias, int bias_dtype, void *out, int out_dtype,
                         const void *plan, int64_t plan_bytes, void *stream);

/*
 * One launch: mbnb_moemlp_gate_up_glu.  x [T, K]; w_codes / w_scales [E, 2I, ...] with row 2j gate j and row 2j + 1 up j, bias
 * NULL or [E, 2I] interleaved the same way; with g = pre[p, 2j], u = pre[p, 2j + 1]
 *   g = g > limit ? limit : g;   u = u > limit ? limit : (u < -limit ? -limit : u)
 *   out[p, j] = round( (u + 1) * (g * (1 / (1 + expf(-(alpha * g))))) )
 * every operation a separate f32 rounding; out is [T, A, I]; a pair whose id is outside [0, E) gets a row of +0.0.  alpha
 * must be finite; limit > 0, +Inf included.
 */
int mbnb_moegemm_gate_up_glu(const void *x, int64_t T, int64_t A, int64_t K, int x_dtype,
                             const void *w_codes, const void *w_scales, int64_t E, int64_t I,
                             const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit,
                             void *out, int out_dtype, const void *plan, int64_t plan_bytes, void *stream);

/* P * N * 4 bytes rounded up to 256; MBNB_MOEGEMM_ERR_SHAPE for sizes mbnb_moegemm_down_sum refuses */
int64_t mbnb_moegemm_workspace_bytes(int64_t P, int64_t N);

/*
 * Two launches: mbnb_moemlp_down_sum.  h [T, A, K]; the first launch stores y[p, n] = pre[p, n] (f32) into the workspace for
 * every pair whose id is in [0, E); the second evaluates, one thread per output,
 *   acc = +0.0;  for a = 0 .. A - 1 in this order, pairs with an id outside [0, E) skipped:  acc = fmaf(rw[t, a], y[t * A + a, n], acc)
 *   out[t, n] = round(acc)
 * to out_dtype; out is [T, N].  Neither rw nor the workspace is read for a skipped pair.  The workspace holds at least
 * mbnb_moegemm_workspace_bytes(T * A, N) bytes (else MBNB_MOEGEMM_ERR_WORKSPACE); its contents are undefined afterwards.
 */
int mbnb_moegemm_down_sum(const void *h, int64_t T, int64_t A, int64_t K, int h_dtype,
                          const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                          const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype,
                          void *out, int out_dtype, void *workspace, int64_t workspace_bytes,
                          const void *plan, int64_t plan_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MOEGEMM_H */
