/*
 * mbnb_moemx.h — C ABI of the grouped GEMM over MXFP4 experts on the block-scaled MFMA, with MX activations
 * (libmbnb_moemx.so): the plain expert projection of mbnb_moegemm.h for any number of (token, slot) pairs in
 * one launch, the activation rows quantised to MXFP8 / MXFP4 beforehand (mbnb_mx_quantize), both operands read by
 * v_mfma_scale_f32_16x16x128_f8f6f4 as they lie in memory: no decode, no per-block FMA.
 *
 * A fifteenth library, with the conventions of the other fourteen:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the quantised activation and the plan included; the library never allocates, frees or
 *     retains device memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation): the expert ids were read ON THE DEVICE by the plan;
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any HIP call,
 *     >0 hipError_t); mbnb_moemx_last_error() returns a thread-local description of the last failure and
 *     mbnb_moemx_last_launch() the form of this thread's last successful call.
 *
 * The formats are mbnb_mx.h's.  Weights, experts stacked as in mbnb_moe.h: w_codes uint8 [E, N, K / 2] (E2M1, the even k in the
 * low nibble), w_scales uint8 [E, N, K / 32] (E8M0; 0xFF means NaN for the block), K % 32 == 0.  Activation rows, as
 * mbnb_mx_quantize writes them: x_codes uint8 [rows, K] (act_elem MBNB_MOEMX_FP8, E4M3) or [rows, K / 2] (MBNB_MOEMX_FP4, E2M1),
 * x_scales uint8 [rows, K / 32].
 *
 * P = T * A (token, slot) pairs, pair p = t * A + a, e = ids[p].  out[p, n] has EXACTLY the bits mbnb_mx_linear writes for the
 * row of pair p against W[e] with the same act_elem: ONE f32 accumulator per output takes the K-steps of 128 in ascending order,
 * one scaled MFMA per step (the k past K count as zeros in both operands); the bias is added in f32; one rounding.  A pair whose
 * activation row holds a 0xFF scale byte is NaN over its whole row; a weight row (e, n) that holds one is NaN for every pair of
 * expert e at column n.  A pair whose id is outside [0, E) gets a row of +0.0.
 *
 * THE PLAN is mbnb_moegemm_plan's, built from the same ids, P and E (mbnb_moegemm.h; this library reads it, it does not build
 * it; both go through ONE text of the layout, csrc/mx_plan.h), as int32 words in this order, R = MBNB_MOEMX_ROW_TILE =
 * MBNB_MOEGEMM_ROW_TILE, max_tiles = min(E, P) + P / R:
 *   counts[E]            (not read here)
 *   n_tiles, n_listed    the entries of the tile table in use, and the pairs with an id in [0, E)
 *   tiles[max_tiles][3]  (expert, first index into sorted, rows <= R), the entries past n_tiles unwritten
 *   sorted[P]            pair indices: the listed pairs grouped by expert, then the pairs with an id outside [0, E)
 * The launch has ceil(N / MBNB_MOEMX_COL_TILE) x max_tiles workgroups; those past n_tiles leave before they touch a weight byte.
 *
 * Alignment: x_codes, w_codes and plan on 16 bytes; ids on 4; out and bias on their element size; x_scales and w_scales none.
 *
 * THE EXPERT MLP on the same kernel: mbnb_moemx_gate_up_glu, then mbnb_moemx_down_sum over its output, with the
 * conventions, limits and order of checks of mbnb_moemx_experts.  The intermediate exists in memory as MX codes and scale bytes
 * only: h_codes uint8 [T * A, I] (fp8) or [T * A, I / 2] (fp4) and h_scales uint8 [T * A, I / 32], what mbnb_mx_quantize would
 * write for the f32 activated rows.
 */
#ifndef MBNB_MOEMX_H
#define MBNB_MOEMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MOEMX_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_MOEMX_F16 = 0, MBNB_MOEMX_BF16 = 1, MBNB_MOEMX_F32 = 2 };

/* activation element formats (the values of mbnb_mx.h's MBNB_MX_FP4 / MBNB_MX_FP8) */
enum { MBNB_MOEMX_FP4 = 0, MBNB_MOEMX_FP8 = 1 };

/* status codes (the values of mbnb_moegemm.h's); a short plan is a short workspace */
enum { MBNB_MOEMX_OK = 0, MBNB_MOEMX_ERR_ARG = -1, MBNB_MOEMX_ERR_SHAPE = -2, MBNB_MOEMX_ERR_WORKSPACE = -3 };

/* the listed pairs of one expert that a workgroup takes: the R of the plan it reads */
#define MBNB_MOEMX_ROW_TILE 64
/* the weight rows of a workgroup: four waves of 64 columns */
#define MBNB_MOEMX_COL_TILE 256
/* the k of one scaled MFMA */
#define MBNB_MOEMX_K_STEP 128
/* the most experts, and the most (token, slot) pairs of one call: mbnb_moegemm.h's */
#define MBNB_MOEMX_MAX_EXPERTS 1024
#define MBNB_MOEMX_MAX_PAIRS 1048576

int mbnb_moemx_abi_version(void);
const char *mbnb_moemx_last_error(void);
/* e.g. "mx_grouped_scaled fp8 shared E32 P4096 64x256" or "mx_grouped_scaled fp4 slot E9 P300 64x256";
 * "mx_grouped_scaled_glu fp8>fp8 E32 P4096 64x256"; "mx_grouped_scaled_down_sum fp8 E32 P4096 64x256 A4"; "" before this
 * thread's first launch */
const char *mbnb_moemx_last_launch(void);

/*
 * One launch.  x_codes / x_scales: T rows (x_per_slot == 0: a token's slots share its row) or T * A rows (a row per pair) of
 * act_elem; bias NULL or [E, N]; out [T, A, N] of out_dtype (any of the three).  Every element of out is written exactly once.
 * plan: at least 4 * (E + 2 + 3 * max_tiles + T * A) bytes rounded up to 256 (mbnb_moegemm_plan_bytes), else
 * MBNB_MOEMX_ERR_WORKSPACE.  E <= MBNB_MOEMX_MAX_EXPERTS, T * A <= MBNB_MOEMX_MAX_PAIRS, any N; T * A == 0 is a no-op success
 * with unread pointers.
 */
int mbnb_moemx_experts(const void *x_codes, const void *x_scales, int act_elem,
                       int64_t T, int64_t A, int x_per_slot, int64_t K,
                       const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                       const int32_t *ids, const void *bias, int bias_dtype, void *out, int out_dtype,
                       const void *plan, int64_t plan_bytes, void *stream);

/*
 * One launch: the gate / up projection with the gated activation and the MX quantiser as its epilogue.  x_codes / x_scales: T
 * rows of act_elem, shared by a token's slots.  w_codes [E, 2 I, K / 2] and w_scales [E, 2 I, K / 32] with interleaved rows, row
 * 2 j gate j and row 2 j + 1 up j; bias NULL or [E, 2 I], interleaved the same way.  I % 32 == 0 (else MBNB_MOEMX_ERR_SHAPE): an
 * activated row is quantised in whole blocks.  With pre[p, n] the f32 value mbnb_moemx_experts writes for out_dtype f32,
 *   g = min(pre[p, 2 j], limit);  u = clamp(pre[p, 2 j + 1], -limit, limit);  h[p, j] = (u + 1) * (g * (1 / (1 + expf(-(alpha * g)))))
 * every operation a separate f32 rounding, the operation chain of mbnb_moegemm_gate_up_glu; then the 32 values of every block of
 * h[p] are quantised by mbnb_mx.h's rule to h_elem: byte = max(E(amax) - emax, 0), a block that holds a NaN or an Inf gets byte
 * 0xFF and codes 0, elements round to nearest, ties to the even code, saturating, the sign of zero kept.  h_elem must equal
 * act_elem (MBNB_MOEMX_ERR_ARG otherwise).  alpha finite, limit > 0 (+Inf: no clamp), else MBNB_MOEMX_ERR_ARG.  A pair whose id
 * is outside [0, E) gets codes 0 and scale bytes 0, the quantised row of +0.0.  Every byte of h_codes and h_scales is written
 * exactly once.  h_codes on 16 bytes, h_scales none.
 */
int mbnb_moemx_gate_up_glu(const void *x_codes, const void *x_scales, int act_elem,
                           int64_t T, int64_t A, int64_t K,
                           const void *w_codes, const void *w_scales, int64_t E, int64_t I,
                           const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit,
                           void *h_codes, void *h_scales, int h_elem,
                           const void *plan, int64_t plan_bytes, void *stream);

/* The bytes of mbnb_moemx_down_sum's workspace for P = T * A pairs: 4 P N rounded up to 256; negative: a status. */
int64_t mbnb_moemx_workspace_bytes(int64_t P, int64_t N);

/*
 * Two launches: the down projection and the routed sum.  h_codes / h_scales: a row per pair, T * A rows of act_elem over K.  The
 * first launch is mbnb_moemx_experts with out_dtype f32 into the workspace y [T * A, N]; the second evaluates, one thread per
 * four consecutive outputs of a token,
 *   acc = +0.0;  for a = 0 .. A - 1 in this order, pairs with an id outside [0, E) skipped:  acc = fmaf(rw[t, a], y[t * A + a, n], acc)
 *   out[t, n] = round(acc)
 * the formula of mbnb_moegemm_down_sum.  A skipped pair's routing weight and workspace row are not read.  rw [T, A] of rw_dtype
 * (any of the three), on its element size; out [T, N] of out_dtype.  workspace: 16-byte aligned, at least
 * mbnb_moemx_workspace_bytes(T * A, N) bytes (else MBNB_MOEMX_ERR_WORKSPACE); its contents are undefined afterwards.
 */
int mbnb_moemx_down_sum(const void *h_codes, const void *h_scales, int act_elem,
                        int64_t T, int64_t A, int64_t K,
                        const void *w_codes, const void *w_scales, int64_t E, int64_t N,
                        const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype,
                        void *out, int out_dtype, void *workspace, int64_t workspace_bytes,
                        const void *plan, int64_t plan_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MOEMX_H */
