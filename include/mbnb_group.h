/*
 * mbnb_group.h — C ABI of the grouped M = 1 decode GEMV (libmbnb_group.so).
 *
 * A sixth library, with the conventions of mbnb_paged.h:
 *
 *   - plain C types only: device pointers, int64 sizes, int enums, an opaque hipStream_t passed as void*;
 *   - the CALLER allocates everything; the library never allocates, frees or retains device memory, owns no
 *     stream and keeps no per-call state;
 *   - every call is asynchronous on `stream` (no device synchronisation, no copy: the member table travels in
 *     the kernel arguments, so a call can be captured into a graph);
 *   - errors are returned as an int status (0 ok, <0 argument error detected on the host before any launch,
 *     >0 hipError_t or MBNB_GROUP_NOT_APPLICABLE); mbnb_group_last_error() returns a thread-local description
 *     of the last failure.
 *
 * One call contracts ONE activation row x[K] with up to MBNB_GROUP_MAX_MEMBERS 4-bit weights [N_g, K] that share
 * K, the code table, the blocksize and the dtype (q / k / v, or gate / up, of a decoder block) in ONE kernel
 * launch: out_g[N_g] = x . dequant(W_g)^T + bias_g.  Each output row is computed by the code of
 * mbnb_matmul_4bit's M = 1 kernel (k_gemv4_lean), so the values equal that call's bit for bit; what the launch
 * saves is the fixed cost per launch (the launch itself, staging x, the code table, the barrier).
 */
#ifndef MBNB_GROUP_H
#define MBNB_GROUP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBNB_GROUP_ABI_VERSION 1

/* element dtypes (the values of libmbnb_hip's MBNB_F16 / MBNB_BF16 / MBNB_F32) and code tables (MBNB_NF4 / MBNB_FP4) */
enum { MBNB_GROUP_F16 = 0, MBNB_GROUP_BF16 = 1, MBNB_GROUP_F32 = 2 };
enum { MBNB_GROUP_NF4 = 0, MBNB_GROUP_FP4 = 1 };

/* status codes.  MBNB_GROUP_NOT_APPLICABLE: the arguments are valid but the fused launch does not serve them (the
 * reason is in mbnb_group_last_error()); nothing was launched and the caller runs the members one by one through
 * mbnb_matmul_4bit.  Above every hipError_t. */
enum { MBNB_GROUP_OK = 0, MBNB_GROUP_ERR_ARG = -1, MBNB_GROUP_ERR_SHAPE = -2, MBNB_GROUP_NOT_APPLICABLE = 65536 };

/* members per call: the table fills about 1 KiB of kernel arguments */
#define MBNB_GROUP_MAX_MEMBERS 16

/* one member of a call: a weight [N, K] with its absmax, bias and output row.  The absmax is given in one of the two
 * forms of struct mbnb_absmax (mbnb_hip.h): plain f32 [N * K / blocksize] in `absmax_f32` (absmax_i8 NULL), or
 * double-quantised: int8 codes in `absmax_i8`, their f32 absmax in `absmax2`, one per `blocksize2` codes. */
struct mbnb_group_member {
    const void *packed;       /* u8 [N, K / 2] */
    const float *absmax_f32;
    const int8_t *absmax_i8;
    const float *absmax2;
    const void *bias;         /* [N] in the call's dtype, or NULL */
    void *out;                /* [N] in the call's dtype */
    int64_t N;
    int32_t blocksize2;
    int32_t pad_;
};

/* the layout, for bindings in other languages */
#define MBNB_GROUP_MEMBER_BYTES 64
#define MBNB_GROUP_MEMBER_OFF_PACKED 0
#define MBNB_GROUP_MEMBER_OFF_ABSMAX_F32 8
#define MBNB_GROUP_MEMBER_OFF_ABSMAX_I8 16
#define MBNB_GROUP_MEMBER_OFF_ABSMAX2 24
#define MBNB_GROUP_MEMBER_OFF_BIAS 32
#define MBNB_GROUP_MEMBER_OFF_OUT 40
#define MBNB_GROUP_MEMBER_OFF_N 48
#define MBNB_GROUP_MEMBER_OFF_BLOCKSIZE2 56
#define MBNB_GROUP_MEMBER_OFF_PAD_ 60
#ifdef __cplusplus
#define MBNB_GROUP_ASSERT(c) static_assert(c, #c)
#else
#define MBNB_GROUP_ASSERT(c) _Static_assert(c, #c)
#endif
MBNB_GROUP_ASSERT(sizeof(struct mbnb_group_member) == MBNB_GROUP_MEMBER_BYTES);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, packed) == MBNB_GROUP_MEMBER_OFF_PACKED);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, absmax_f32) == MBNB_GROUP_MEMBER_OFF_ABSMAX_F32);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, absmax_i8) == MBNB_GROUP_MEMBER_OFF_ABSMAX_I8);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, absmax2) == MBNB_GROUP_MEMBER_OFF_ABSMAX2);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, bias) == MBNB_GROUP_MEMBER_OFF_BIAS);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, out) == MBNB_GROUP_MEMBER_OFF_OUT);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, N) == MBNB_GROUP_MEMBER_OFF_N);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, blocksize2) == MBNB_GROUP_MEMBER_OFF_BLOCKSIZE2);
MBNB_GROUP_ASSERT(offsetof(struct mbnb_group_member, pad_) == MBNB_GROUP_MEMBER_OFF_PAD_);

int mbnb_group_abi_version(void);
const char *mbnb_group_last_error(void);

/* The form of this thread's last launch: "gemv_group G<members> ku<chunks of 2048 k>/KU<the instantiation>", e.g.
 * "gemv_group G3 ku2/KU2".  Empty until the first launch; a call that launches nothing leaves it as it was. */
const char *mbnb_group_last_launch(void);

/*
 * out_g = x[K] . dequant(W_g)^T + bias_g for the `n` members of `members` (0 <= n <= MBNB_GROUP_MAX_MEMBERS) in one
 * launch of Σ ceil(N_g / 4) workgroups; no workgroup covers two members.  `dtype` is the dtype of x, of the decoded
 * weight, of every bias and of every output.  n == 0 is a no-op success.
 *
 * Returns 0 after the launch; a negative code for n outside 0..16, a NULL table, x, packed, out or absmax (int8
 * codes without absmax2 included), an unknown dtype, quant type or flag (none is defined: flags must be 0), K,
 * blocksize or N <= 0; MBNB_GROUP_NOT_APPLICABLE, before any launch, unless all of these hold (the conditions of
 * k_gemv4_lean):
 *   blocksize == 64; K % 64 == 0 and 1024 <= K <= 16384; a 16-bit dtype; x and every `packed` 16-byte aligned;
 *   N * K / 2 < 2^40 per member; fewer than 2^31 workgroups in all; all members plain or all members
 *   double-quantised, and then for each: blocksize2 a power of two, absmax_i8 4-byte aligned, (K / 64) % 4 == 0.
 */
int mbnb_group_gemv4(const void *x, int64_t K, int quant_type, int dtype, int blocksize,
                     const struct mbnb_group_member *members, int n, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MBNB_GROUP_H */
