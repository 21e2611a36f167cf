/*
 * mbnb_optim.h — C ABI of the 8-bit optimizer step (libmbnb_optim.so).
 *
 * A separate library from libmbnb_hip.so (whose ABI version 2 is frozen), with the same conventions:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory and
 *     keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any
 *     launch, >0 hipError_t); mbnb_optim_last_error() returns a thread-local description of the last failure.
 *
 * One call steps up to MBNB_OPTIM_MAX_TENSORS tensors of one parameter dtype and one gradient dtype in ONE
 * kernel launch (multi-tensor apply): the descriptor table travels in the kernel arguments.  The state layout
 * is the reference's (mps_bitsandbytes/optim/adam8bit.py): per tensor, signed int8 codes q with f32 block
 * maxima (value = q / 127 * absmax) and, for Adam's second moment, unsigned sqrt-compressed uint8 codes
 * (value = (q / 255)^2 * max); `block_size` consecutive elements of the flattened tensor share one maximum,
 * the last block of a tensor may be partial.  All tensors are dense and contiguous; the parameter and
 * gradient pointers are 16-byte aligned, the code pointers 4-byte aligned.
 */
#ifndef MBNB_OPTIM_H
#define MBNB_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_OPTIM_ABI_VERSION 1

/* optimizer rules */
enum {
    MBNB_OPTIM_ADAM = 0,          /* L2 weight decay folded into the gradient (Adam8bit) */
    MBNB_OPTIM_ADAMW = 1,         /* decoupled weight decay (AdamW8bit) */
    MBNB_OPTIM_LION = 2,
    MBNB_OPTIM_SGD_MOMENTUM = 3,
    MBNB_OPTIM_SGD_NESTEROV = 4,
};

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) */
enum { MBNB_OPTIM_F16 = 0, MBNB_OPTIM_BF16 = 1, MBNB_OPTIM_F32 = 2 };

/* status codes */
enum { MBNB_OPTIM_OK = 0, MBNB_OPTIM_ERR_ARG = -1, MBNB_OPTIM_ERR_SHAPE = -2 };

/* tensors per call: the table and the group scalars fill at most 4 KiB of kernel arguments */
#define MBNB_OPTIM_MAX_TENSORS 48

/* group scalars, f32, as the reference rounds them (computed in double on the host, then rounded once) */
struct mbnb_optim_scalars {
    float beta1;          /* Adam, Lion: beta1; SGD: momentum */
    float one_minus_beta1;/* Adam, Lion: 1 - beta1; SGD: 1 - dampening */
    float beta2;          /* Adam, Lion: beta2 */
    float one_minus_beta2;/* Adam, Lion: 1 - beta2 */
    float eps;            /* Adam */
    float weight_decay;   /* Adam: wd (f32); SGD: wd rounded to the gradient dtype */
    float decay;          /* AdamW, Lion: 1 - lr * wd */
    float neg_lr;         /* Lion, SGD: -lr rounded to the parameter dtype */
    int32_t flags;        /* MBNB_OPTIM_WEIGHT_DECAY: apply weight decay (the reference skips it when wd == 0) */
    int32_t pad_;
};
enum { MBNB_OPTIM_WEIGHT_DECAY = 1 };

/* one tensor of a call */
struct mbnb_optim_tensor {
    void *param;          /* parameter, updated in place */
    const void *grad;     /* gradient: the parameter dtype or f32 */
    void *state1;         /* int8 codes: Adam exp_avg, Lion exp_avg, SGD momentum */
    float *absmax1;       /* [ceil(numel / block_size)] */
    void *state2;         /* Adam: uint8 codes of exp_avg_sq; NULL otherwise */
    float *max2;          /* Adam: [ceil(numel / block_size)]; NULL otherwise */
    int64_t numel;
    float bc2_sqrt;       /* Adam: sqrt(1 - beta2 ** step) */
    float neg_step_size;  /* Adam: -lr / (1 - beta1 ** step) */
};

int mbnb_optim_abi_version(void);
const char *mbnb_optim_last_error(void);

/*
 * One fused step over `n` tensors (0 <= n <= MBNB_OPTIM_MAX_TENSORS): each block of state is read once,
 * updated in f32 and written once.  block_size 256 runs one wave per block; any other positive block_size runs
 * one 256-thread workgroup per block (flags & MBNB_OPTIM_FORCE_GENERIC selects that path at 256 too).
 * grad_dtype must be param_dtype or MBNB_OPTIM_F32.  n == 0 is a no-op success.
 */
enum { MBNB_OPTIM_FORCE_GENERIC = 1 };
int mbnb_optim_step(int kind, int param_dtype, int grad_dtype, int64_t block_size,
                    const struct mbnb_optim_scalars *scalars, const struct mbnb_optim_tensor *table, int n,
                    int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_OPTIM_H */
