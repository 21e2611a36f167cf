/*
 * mbnb_paged.h — C ABI of the fused full-precision optimizer step (libmbnb_paged.so).
 *
 * A fifth library, with the conventions of mbnb_optim.h:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory, owns no
 *     stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any
 *     launch, >0 hipError_t); mbnb_paged_last_error() returns a thread-local description of the last failure.
 *
 * One call steps up to MBNB_PAGED_MAX_SEGMENTS *segments* of one dtype in ONE kernel launch.  A segment is any
 * element range of a tensor: pointers to its parameter, gradient and moment elements (all of the call's dtype,
 * as the reference's zeros_like(p) state) and a count.  The step is purely elementwise, so the kernel knows
 * nothing about paging: the moment pointers may be a tensor's own storage or a staging slot that a page of
 * host-resident moments was copied into.  Every pointer is device memory, aligned to its element size.  Where
 * all pointers of a segment share one offset modulo 16 bytes the body moves in 16-byte vectors and only the
 * head and the tail go element by element; otherwise the whole segment does.
 */
#ifndef MBNB_PAGED_H
#define MBNB_PAGED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_PAGED_ABI_VERSION 1

/* optimizer rules */
enum {
    MBNB_PAGED_ADAM = 0,          /* L2 weight decay folded into the gradient (PagedAdam) */
    MBNB_PAGED_ADAMW = 1,         /* decoupled weight decay (PagedAdamW) */
    MBNB_PAGED_LION = 2,
};

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_PAGED_F16 = 0, MBNB_PAGED_BF16 = 1, MBNB_PAGED_F32 = 2 };

/* status codes */
enum { MBNB_PAGED_OK = 0, MBNB_PAGED_ERR_ARG = -1, MBNB_PAGED_ERR_SHAPE = -2 };

/* segments per call: the table and the group scalars fill at most 4 KiB of kernel arguments */
#define MBNB_PAGED_MAX_SEGMENTS 48

/* group scalars, f32.  The host computes each in double and rounds it once to f32 ("s32") or, where the
 * reference's op takes it as the `alpha` of a tensor op, to f32 and then to the tensor dtype ("sT"). */
struct mbnb_paged_scalars {
    float beta1;          /* s32(beta1) */
    float one_minus_beta1;/* sT(1 - beta1) */
    float beta2;          /* s32(beta2) */
    float one_minus_beta2;/* Adam: s32(1 - beta2) (the `value` of addcmul_); Lion: sT(1 - beta2) */
    float eps;            /* Adam: s32(eps) */
    float weight_decay;   /* Adam: sT(wd) */
    float decay;          /* AdamW, Lion: s32(1 - lr * wd) */
    float neg_lr;         /* Lion: sT(-lr) */
    int32_t flags;        /* MBNB_PAGED_WEIGHT_DECAY: apply weight decay (the reference skips it when wd == 0) */
    int32_t pad_;
};
enum { MBNB_PAGED_WEIGHT_DECAY = 1 };

/* one segment of a call */
struct mbnb_paged_segment {
    void *param;          /* parameter elements, updated in place */
    const void *grad;     /* gradient elements */
    void *exp_avg;        /* first moment, updated in place */
    void *exp_avg_sq;     /* Adam: second moment, updated in place; NULL for Lion */
    int64_t numel;
    float bc2_sqrt;       /* Adam: s32(sqrt(1 - beta2 ** step)) of the segment's tensor */
    float neg_step_size;  /* Adam: s32(-(lr / (1 - beta1 ** step))) of the segment's tensor */
};

int mbnb_paged_abi_version(void);
const char *mbnb_paged_last_error(void);

/*
 * One fused step over `n` segments (0 <= n <= MBNB_PAGED_MAX_SEGMENTS): every element of the parameter, the
 * gradient and the moments is read once, updated in f32 registers and written once.  No workgroup covers two
 * segments.  flags & MBNB_PAGED_FORCE_SCALAR takes every segment element by element (tests compare the two
 * paths).  n == 0 is a no-op success.
 */
enum { MBNB_PAGED_FORCE_SCALAR = 1 };
int mbnb_paged_step(int kind, int dtype, const struct mbnb_paged_scalars *scalars,
                    const struct mbnb_paged_segment *table, int n, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_PAGED_H */
