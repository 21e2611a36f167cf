/*
 * mbnb_mlora.h — C ABI of the grouped 4-bit decode launches for 2 to 16 activation rows that carry a DIFFERENT un-merged
 * LoRA adapter per row (libmbnb_mlora.so).
 *
 * A ninth library, with the conventions of mbnb_group.h, whose member struct it reuses, and of mbnb_batch.h, whose
 * mbnb_batch_gemm4_lora serves the same rows with the member's ONE adapter (see that header for the workgroup, the
 * conditions of the base launch and the argument errors; they are the same here):
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the f32 workspaces `t` included; the library never allocates, frees or
 *     retains device memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation, no copy: the tables travel in the kernel
 *     arguments, so a call can be captured into a graph);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch,
 *     >0 hipError_t or MBNB_MLORA_NOT_APPLICABLE); mbnb_mlora_last_error() returns a thread-local description of
 *     the last failure.
 *
 * Continuous batching over one frozen 4-bit base hands every projection a few rows whose requests carry different
 * adapters.  Here each member has a BANK of S adapters, and row m of the batch uses slot ids[m] of every bank.  `ids`
 * lives in DEVICE memory and is read by the kernels only: the host never dereferences it, so a call, or a captured
 * graph of calls, serves a new assignment once the ids are overwritten in place.
 */
#ifndef MBNB_MLORA_H
#define MBNB_MLORA_H

#include "mbnb_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_MLORA_ABI_VERSION 1

/* status codes: those of mbnb_group.h.  MBNB_MLORA_NOT_APPLICABLE: the arguments are valid but the fused launches do
 * not serve them (the reason is in mbnb_mlora_last_error()); nothing was launched or dereferenced. */
enum { MBNB_MLORA_OK = 0, MBNB_MLORA_ERR_ARG = -1, MBNB_MLORA_ERR_SHAPE = -2, MBNB_MLORA_NOT_APPLICABLE = 65536 };

/* the activation rows a call serves (those of mbnb_batch.h) */
#define MBNB_MLORA_MIN_M 2
#define MBNB_MLORA_MAX_M 16

/* the largest rank: one wave-wide slice.  The 16 rows of B are staged in LDS per (activation row, weight row) */
#define MBNB_MLORA_MAX_R 64

/* the adapter bank of one member (banks[i] belongs to members[i]): S adapters of one rank R */
struct mbnb_mlora_bank {
    const void *a;              /* [S, R, K] row-major, the call's dtype: slot s is the dense [R, K] block s */
    const void *b;              /* [S, N, R] row-major, the call's dtype */
    const float *scaling;       /* f32 [S], DEVICE memory */
    float *t;                   /* f32 [M, R] workspace, caller-allocated; row m holds A_{ids[m]} . x[m] after the call,
                                   and is left as it was for a row without an adapter */
    int32_t R;                  /* 0: the member has no bank; the other fields are then ignored */
    int32_t S;
};

/* the layout, for bindings in other languages */
#define MBNB_MLORA_BANK_BYTES 40
#define MBNB_MLORA_BANK_OFF_A 0
#define MBNB_MLORA_BANK_OFF_B 8
#define MBNB_MLORA_BANK_OFF_SCALING 16
#define MBNB_MLORA_BANK_OFF_T 24
#define MBNB_MLORA_BANK_OFF_R 32
#define MBNB_MLORA_BANK_OFF_S 36
MBNB_GROUP_ASSERT(sizeof(struct mbnb_mlora_bank) == MBNB_MLORA_BANK_BYTES);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, a) == MBNB_MLORA_BANK_OFF_A);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, b) == MBNB_MLORA_BANK_OFF_B);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, scaling) == MBNB_MLORA_BANK_OFF_SCALING);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, t) == MBNB_MLORA_BANK_OFF_T);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, R) == MBNB_MLORA_BANK_OFF_R);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_mlora_bank, S) == MBNB_MLORA_BANK_OFF_S);

int mbnb_mlora_abi_version(void);
const char *mbnb_mlora_last_error(void);

/* The form of this thread's last call that launched: "lora_down_sel G<members> R<sum of R> M<rows> ku<chunks of 2048
 * k>/KU<instantiation> + skinny_mlora G<members> M<rows>".  Empty until the first launch; a call that launches nothing
 * leaves it as it was. */
const char *mbnb_mlora_last_launch(void);

/*
 * out_g[m, :] = x[m] . dequant(W_g)^T + bias_g + scaling_g[s] * (x[m] . A_{g,s}^T) . B_{g,s}^T with s = ids[m], in two
 * launches on `stream`: k_lora_down_sel over sum(R_g) * M workgroups (t_g[m, j] = A_{g,s}[j, :] . x[m, :] in f32), then
 * k_skinny4_mlora, the workgroup of mbnb_batch_gemm4 with a per-row rank-R epilogue.
 *
 * A row whose ids[m] lies outside [0, S_g) -- -1, S_g, any other int32 -- uses no adapter of member g: it reads nothing
 * from the bank or from t, and its values are mbnb_batch_gemm4's bit for bit, as are those of a member with R == 0.  A
 * row with an adapter gets the bits mbnb_batch_gemm4_lora gives that row with the adapter (A_{g,s}, B_{g,s},
 * scaling_g[s]): the summation chains are the same.  Every sum runs in a fixed order (no atomics): equal inputs give
 * equal bits on every call.  n == 0 is a no-op success.
 *
 * Returns 0 after the launches; a negative code for what mbnb_batch_gemm4 answers so, for a NULL `banks` or `ids`,
 * R < 0 or S < 0, or R > 0 with a NULL a or b; MBNB_MLORA_NOT_APPLICABLE, before any launch, unless all conditions of
 * mbnb_batch_gemm4 hold (2 <= M <= 16 among them), `ids` is 4-byte aligned and, for every member with R > 0:
 * R <= MBNB_MLORA_MAX_R and S >= 1, `a` 16-byte aligned, `b` 2-byte aligned, `scaling` and `t` non-NULL and 4-byte
 * aligned; and at least one member has R > 0 (otherwise the call is mbnb_batch_gemm4's).
 */
int mbnb_mlora_gemm4(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize,
                     const struct mbnb_group_member *members, const struct mbnb_mlora_bank *banks,
                     const int32_t *ids /* DEVICE, [M] */, int n, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_MLORA_H */
