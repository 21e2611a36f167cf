/*
 * mbnb_batch.h — C ABI of the grouped 4-bit decode launches for 2 to 16 activation rows (libmbnb_batch.so).
 *
 * An eighth library, with the conventions of mbnb_group.h and mbnb_lora.h, whose member and adapter structs it reuses:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the f32 workspaces `t` included; the library never allocates, frees or
 *     retains device memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation, no copy: the tables travel in the kernel
 *     arguments, so a call can be captured into a graph);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch,
 *     >0 hipError_t or MBNB_BATCH_NOT_APPLICABLE); mbnb_batch_last_error() returns a thread-local description of
 *     the last failure.
 *
 * mbnb_group_gemv4 and mbnb_lora_gemv4 serve ONE activation row.  A serving loop (continuous batching, speculative
 * decoding) hands every projection 2 to 16 rows per step; for those row counts mbnb_matmul_4bit streams the weight
 * through k_skinny4 (16 weight rows x all M activation rows per workgroup on v_mfma_f32_16x16x32).  The calls here put
 * that workgroup behind the member table of mbnb_group.h: up to MBNB_GROUP_MAX_MEMBERS weights that share the
 * activation matrix x[M, K] in ONE launch, each output equal to mbnb_matmul_4bit's bit for bit, and with un-merged
 * LoRA adapters in TWO.
 */
#ifndef MBNB_BATCH_H
#define MBNB_BATCH_H

#include "mbnb_group.h"
#include "mbnb_lora.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_BATCH_ABI_VERSION 1

/* status codes: those of mbnb_group.h.  MBNB_BATCH_NOT_APPLICABLE: the arguments are valid but the fused launches do
 * not serve them (the reason is in mbnb_batch_last_error()); nothing was launched or dereferenced. */
enum { MBNB_BATCH_OK = 0, MBNB_BATCH_ERR_ARG = -1, MBNB_BATCH_ERR_SHAPE = -2, MBNB_BATCH_NOT_APPLICABLE = 65536 };

/* the activation rows a call serves */
#define MBNB_BATCH_MIN_M 2
#define MBNB_BATCH_MAX_M 16

int mbnb_batch_abi_version(void);
const char *mbnb_batch_last_error(void);

/* The form of this thread's last call that launched: "skinny_group G<members> M<rows>" for mbnb_batch_gemm4,
 * "lora_down_rows G<members> R<sum of R> M<rows> ku<chunks of 2048 k>/KU<instantiation> + skinny_group_lora G<members>
 * M<rows>" for mbnb_batch_gemm4_lora.  Empty until the first launch; a call that launches nothing leaves it as it was. */
const char *mbnb_batch_last_launch(void);

/*
 * out_g[M, N_g] = x[M, K] . dequant(W_g)^T + bias_g for the `n` members (0 <= n <= MBNB_GROUP_MAX_MEMBERS) in one launch
 * of sum(ceil(N_g / 16)) workgroups of 1024 threads; no workgroup covers two members.  members[g].out is a dense
 * row-major [M, N_g] block.  `dtype` is the dtype of x, of the decoded weight, of every bias and of every output.
 * Each workgroup is mbnb_matmul_4bit's k_skinny4 workgroup (MT = 1, NR = 1) on its member's pointers, so the values
 * equal that call's bit for bit.  n == 0 is a no-op success.
 *
 * Returns 0 after the launch; a negative code for n outside 0..16, a NULL table, x, packed, out or absmax (int8 codes
 * without absmax2 included), an unknown dtype, quant type or flag (none is defined: flags must be 0), M, K, blocksize
 * or N <= 0; MBNB_BATCH_NOT_APPLICABLE, before any launch, unless all of these hold:
 *   2 <= M <= 16; a 16-bit dtype; blocksize a power of two >= 32; K % 128 == 0, K % blocksize == 0 and
 *   128 <= K <= 16384; x and every `packed` 16-byte aligned; N * K / 2 < 2^40 per member; fewer than 2^31 workgroups in
 *   all; all members plain or all members double-quantised, and then blocksize2 > 0 for each.
 */
int mbnb_batch_gemm4(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize,
                     const struct mbnb_group_member *members, int n, int flags, void *stream);

/*
 * out_g[M, N_g] = x . dequant(W_g)^T + bias_g + scaling_g * (x . A_g^T) . B_g^T in two launches on `stream`:
 * k_lora_down_rows over sum(R_g) workgroups (t_g[m, j] = A_g[j, :] . x[m, :] in f32), then k_skinny4_group with a rank-R
 * epilogue.  Here adapters[g].t is an f32 workspace [M, R_g], row-major; every row of the batch uses the member's one
 * adapter.  A member with R == 0 gets mbnb_batch_gemm4's value bit for bit.  Every sum runs in a fixed order (no
 * atomics): equal inputs give equal bits on every call.  n == 0 is a no-op success.
 *
 * Returns 0 after the launches; a negative code for what mbnb_batch_gemm4 answers so, for a NULL `adapters`, R < 0, or
 * R > 0 with a NULL a or b; MBNB_BATCH_NOT_APPLICABLE, before any launch, unless all conditions of mbnb_batch_gemm4 hold
 * and, for every member with R > 0: R <= MBNB_LORA_MAX_R, `a` 16-byte aligned, `b` 2-byte aligned, `t` non-NULL and
 * 4-byte aligned, `scaling` finite; and at least one member has R > 0 (otherwise the call is mbnb_batch_gemm4's).
 */
int mbnb_batch_gemm4_lora(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize,
                          const struct mbnb_group_member *members, const struct mbnb_lora_adapter *adapters, int n,
                          int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_BATCH_H */
