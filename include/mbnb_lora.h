/*
 * mbnb_lora.h — C ABI of the grouped M = 1 decode GEMV with un-merged LoRA adapters (libmbnb_lora.so).
 *
 * A seventh library, with the conventions of mbnb_group.h, whose member struct it reuses:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything, the f32 workspaces `t` included; the library never allocates, frees or
 *     retains device memory, owns no stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation, no copy: both tables travel in the
 *     kernel arguments, so a call can be captured into a graph);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch,
 *     >0 hipError_t or MBNB_LORA_NOT_APPLICABLE); mbnb_lora_last_error() returns a thread-local description of
 *     the last failure.
 *
 * A LoRA adapter trained over a 4-bit base cannot be merged into it, so a decode step evaluates, per adapted layer,
 *     out_g[N_g] = x . dequant(W_g)^T + bias_g + scaling_g * (B_g . (A_g . x))
 * One call does that for up to MBNB_GROUP_MAX_MEMBERS layers that share x in TWO launches: t_g = A_g . x for every
 * adapter row of every member (f32), then mbnb_group_gemv4's launch with a rank-R epilogue that adds
 * scaling_g * B_g[n, :] . t_g to the f32 accumulator of row n before the bias add and the single rounding.
 */
#ifndef MBNB_LORA_H
#define MBNB_LORA_H

#include "mbnb_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_LORA_ABI_VERSION 1

/* status codes: those of mbnb_group.h.  MBNB_LORA_NOT_APPLICABLE: the arguments are valid but the fused launches do not
 * serve them (the reason is in mbnb_lora_last_error()); nothing was launched or dereferenced. */
enum { MBNB_LORA_OK = 0, MBNB_LORA_ERR_ARG = -1, MBNB_LORA_ERR_SHAPE = -2, MBNB_LORA_NOT_APPLICABLE = 65536 };

/* the largest rank the row epilogue serves: four wave-wide slices of a row of B */
#define MBNB_LORA_MAX_R 256

/* the adapter of one member (adapters[i] belongs to members[i]) */
struct mbnb_lora_adapter {
    const void *a;      /* [R, K] row-major, the call's dtype */
    const void *b;      /* [N, R] row-major, the call's dtype */
    float *t;           /* f32 [R] workspace, caller-allocated; holds A . x after the call */
    int32_t R;          /* 0: the member has no adapter; a, b, t are then ignored */
    float scaling;
};

/* the layout, for bindings in other languages */
#define MBNB_LORA_ADAPTER_BYTES 32
#define MBNB_LORA_ADAPTER_OFF_A 0
#define MBNB_LORA_ADAPTER_OFF_B 8
#define MBNB_LORA_ADAPTER_OFF_T 16
#define MBNB_LORA_ADAPTER_OFF_R 24
#define MBNB_LORA_ADAPTER_OFF_SCALING 28
MBNB_GROUP_ASSERT(sizeof(struct mbnb_lora_adapter) == MBNB_LORA_ADAPTER_BYTES);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_lora_adapter, a) == MBNB_LORA_ADAPTER_OFF_A);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_lora_adapter, b) == MBNB_LORA_ADAPTER_OFF_B);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_lora_adapter, t) == MBNB_LORA_ADAPTER_OFF_T);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_lora_adapter, R) == MBNB_LORA_ADAPTER_OFF_R);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_lora_adapter, scaling) == MBNB_LORA_ADAPTER_OFF_SCALING);

int mbnb_lora_abi_version(void);
const char *mbnb_lora_last_error(void);

/* The form of this thread's last call that launched:
 * "lora_down G<members> R<sum of R> ku<chunks of 2048 k>/KU<instantiation> + gemv_lora G<members> ku<..>/KU<..>", e.g.
 * "lora_down G3 R48 ku2/KU2 + gemv_lora G3 ku2/KU2".  Empty until the first launch; a call that launches nothing
 * leaves it as it was. */
const char *mbnb_lora_last_launch(void);

/*
 * out_g = x[K] . dequant(W_g)^T + bias_g + scaling_g * B_g . (A_g . x) for the `n` members (0 <= n <=
 * MBNB_GROUP_MAX_MEMBERS) in two launches on `stream`: k_lora_down over sum(R_g) workgroups, then k_gemv4_group_lora
 * over sum(ceil(N_g / 4)).  A member with R == 0 gets mbnb_group_gemv4's value bit for bit.  The contraction over K and
 * the one over R accumulate in f32 in a fixed order (no atomics): equal inputs give equal bits on every call.
 * n == 0 is a no-op success.
 *
 * Returns 0 after the launches; a negative code for what mbnb_group_gemv4 answers so, for a NULL `adapters`, R < 0, or
 * R > 0 with a NULL a or b; MBNB_LORA_NOT_APPLICABLE, before any launch, unless all conditions of mbnb_group_gemv4
 * hold and, for every member with R > 0: R <= MBNB_LORA_MAX_R, `a` 16-byte aligned, `b` 2-byte aligned, `t` non-NULL
 * and 4-byte aligned, `scaling` finite; and at least one member has R > 0 (otherwise the call is mbnb_group_gemv4's).
 */
int mbnb_lora_gemv4(const void *x, int64_t K, int quant_type, int dtype, int blocksize,
                    const struct mbnb_group_member *members, const struct mbnb_lora_adapter *adapters, int n,
                    int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_LORA_H */
