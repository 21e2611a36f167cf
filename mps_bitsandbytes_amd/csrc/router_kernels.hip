// router_kernels.hip — the router of a mixture-of-experts block for a decode batch, and the C ABI of libmbnb_router.so
// (include/mbnb_router.h).
//
//   k_router  one workgroup of 16 waves per token.  The token's row is staged in LDS; wave w takes the experts w, w + 16, ..., four
//             of them at a time: each lane walks the 16-byte chunks lane, lane + 64, ... of the row in ascending order with fmaf into
//             ONE f32 accumulator per expert (a 16-bit x 16-bit product is exact in f32), the 64 partial sums are folded by a fixed
//             xor butterfly (32 down to 1), and one lane adds the bias and keeps the logit in LDS (and in logits_out).  After a
//             barrier wave 0 selects: every lane holds up to 16 candidates as a 64-bit key (the order-preserving image of the f32,
//             NaN the maximum, -0 on +0's key, above the inverted expert index: one max decides value and tie), A rounds of wave
//             arg-max retire their winner, and lanes 0 .. A - 1 evaluate the softmax chain, slot a on lane a.
//
// The order of a logit's sum is fixed by (K, lane, chunk) alone: it does not depend on T, blockIdx or logits_out.
#include "../../include/mbnb_router.h"
#include "host.h"

static_assert(MBNB_ROUTER_F16 == mbnb::kF16 && MBNB_ROUTER_BF16 == mbnb::kBF16 && MBNB_ROUTER_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_ROUTER_MAX_EXPERTS == 1024, "wave 0 holds 16 candidates per lane");
static_assert(MBNB_ROUTER_MAX_TOPK <= 64, "slot a of a token is lane a");
static_assert(MBNB_ROUTER_MAX_K % 8 == 0 && MBNB_ROUTER_MAX_K * 2 + MBNB_ROUTER_MAX_EXPERTS * 4 <= 64 * 1024, "a row and the logits in LDS");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

constexpr int kWaves = 16;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxExperts = MBNB_ROUTER_MAX_EXPERTS;
constexpr int kCand = kMaxExperts / 64;     // candidates per lane of the selecting wave
constexpr int kU = 4;                       // experts a wave walks at a time: their loads are in flight together

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));

// the two 16-bit elements of a dword as f32, the lower address first
template <typename T> __device__ __forceinline__ void widen2(uint32_t u, float &lo, float &hi);
template <> __device__ __forceinline__ void widen2<bf16_t>(uint32_t u, float &lo, float &hi) {
    lo = __uint_as_float(u << 16);
    hi = __uint_as_float(u & 0xFFFF0000u);
}
template <> __device__ __forceinline__ void widen2<f16_t>(uint32_t u, float &lo, float &hi) {
    const v2h h = __builtin_bit_cast(v2h, u);
    lo = (float)h[0];
    hi = (float)h[1];
}

// acc += the eight products of a chunk, k ascending, one rounding each
template <typename T> __device__ __forceinline__ float dot8(float acc, v4u xv, v4u wv) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float x0, x1, w0, w1;
        widen2<T>(xv[q], x0, x1);
        widen2<T>(wv[q], w0, w1);
        acc = __builtin_fmaf(x0, w0, acc);
        acc = __builtin_fmaf(x1, w1, acc);
    }
    return acc;
}

__device__ __forceinline__ float load_f32(const void *p, int dtype, int64_t i) {
    if (dtype == MBNB_ROUTER_F32) return ((const float *)p)[i];
    if (dtype == MBNB_ROUTER_BF16) return (float)((const bf16_t *)p)[i];
    return (float)((const f16_t *)p)[i];
}

__device__ __forceinline__ void store_round(void *p, int dtype, int64_t i, float v) {     // ONE rounding to dtype
    if (dtype == MBNB_ROUTER_F32) ((float *)p)[i] = v;
    else if (dtype == MBNB_ROUTER_BF16) ((bf16_t *)p)[i] = (bf16_t)v;
    else ((f16_t *)p)[i] = (f16_t)v;
}

// The rank of a logit as an unsigned integer: a NaN of either sign the maximum, -0 on +0's key, the rest in the order of their
// values.  Below it the inverted expert index, so that among equal logits the LOWER index is the larger key.  Never 0.
__device__ __forceinline__ uint64_t rank_key(float v, int e) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    uint32_t k;
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) k = 0xFFFFFFFFu;
    else k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)k << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)e);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
    return ((uint64_t)hi << 32) | lo;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_router(const T *__restrict__ x, const T *__restrict__ W, const void *__restrict__ bias,
                                                     int bias_dtype, int K, int E, int A, int32_t *__restrict__ ids,
                                                     void *__restrict__ rw, int rw_dtype, float *__restrict__ logits_out) {
    static_assert(sizeof(T) == 2, "16-bit activations");
    extern __shared__ v4u row[];                             // K / 8 chunks of 16 bytes
    __shared__ float logit[kMaxExperts];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t t = blockIdx.x;
    const int chunks = K / 8;

    const v4u *x_row = (const v4u *)(x + t * K);
    for (int c = tid; c < chunks; c += kThreads) row[c] = x_row[c];
    __syncthreads();

    for (int e0 = wave; e0 < E; e0 += kWaves * kU) {         // wave-uniform
        const v4u *w_row[kU];
        float acc[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {                       // an expert past E reads the last row and stores nothing
            const int e = e0 + kWaves * u < E ? e0 + kWaves * u : E - 1;
            w_row[u] = (const v4u *)(W + (int64_t)e * K);
            acc[u] = 0.0f;
        }
        for (int c = lane; c < chunks; c += 64) {
            const v4u xv = row[c];
            v4u wv[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) wv[u] = w_row[u][c];
#pragma unroll
            for (int u = 0; u < kU; ++u) acc[u] = dot8<T>(acc[u], xv, wv[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[u] += __shfl_xor(acc[u], m);       // both partners add the same two values
            const int e = e0 + kWaves * u;
            if (lane == 0 && e < E) {
                const float l = bias ? acc[u] + load_f32(bias, bias_dtype, e) : acc[u];
                logit[e] = l;
                if (logits_out) logits_out[t * E + e] = l;
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;

    // candidate j of a lane is expert lane + 64 j; 0 marks none (past E, or retired)
    const int nc = (E + 63) / 64;                            // uniform
    uint64_t key[kCand];
#pragma unroll
    for (int j = 0; j < kCand; ++j) {
        const int e = lane + 64 * j;
        key[j] = e < E ? rank_key(logit[e], e) : 0ull;
    }
    int my_id = 0;
    for (int a = 0; a < A; ++a) {
        uint64_t best = 0ull;
#pragma unroll
        for (int j = 0; j < kCand; ++j)
            if (j < nc) best = key[j] > best ? key[j] : best;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t other = shfl_xor64(best, m);
            best = other > best ? other : best;
        }
#pragma unroll
        for (int j = 0; j < kCand; ++j)
            if (j < nc) key[j] = key[j] == best ? 0ull : key[j];
        if (lane == a) my_id = (int)(0xFFFFFFFFu - (uint32_t)best);
    }

    // slot a on lane a; the lanes past A carry slot 0's value through the shuffles and store nothing
    const bool live = lane < A;
    const float v = logit[live ? my_id : 0];
    const float v0 = __shfl(v, 0);
    const float d = (live ? v : v0) - v0;
    const float ex = expf(d);
    float s = __shfl(ex, 0);
    for (int a = 1; a < A; ++a) s = s + __shfl(ex, a);       // uniform: ((e0 + e1) + e2) + ...
    const float wgt = ex / s;
    if (live) {
        ids[t * A + lane] = my_id;
        store_round(rw, rw_dtype, t * A + lane, wgt);
    }
}

// ---------------------------------------------------------------- host side
bool known_dtype(int d) { return d >= MBNB_ROUTER_F16 && d <= MBNB_ROUTER_F32; }
const char *name16(int d) { return d == MBNB_ROUTER_BF16 ? "bf16" : "f16"; }

template <typename T>
int launch(const void *x, const void *w, const void *bias, int bias_dtype, int64_t T_, int64_t K, int64_t E, int64_t A, int32_t *ids,
           void *rw, int rw_dtype, float *logits_out, hipStream_t s) {
    hipLaunchKernelGGL((k_router<T>), dim3((unsigned)T_), dim3(kThreads), (size_t)(K * 2), s, (const T *)x, (const T *)w, bias, bias_dtype,
                       (int)K, (int)E, (int)A, ids, rw, rw_dtype, logits_out);
    return mbnb::launch_status("k_router");
}

}  // namespace

extern "C" {

int mbnb_router_abi_version(void) { return MBNB_ROUTER_ABI_VERSION; }

const char *mbnb_router_last_error(void) { return mbnb::last_error(); }

const char *mbnb_router_last_launch(void) { return mbnb::last_launch(); }

int mbnb_router_topk_softmax(const void *x, int64_t T, int64_t K, int x_dtype, const void *w, int64_t E, const void *bias, int bias_dtype,
                             int64_t A, int32_t *ids, void *rw, int rw_dtype, float *logits_out, void *stream) {
    const char *const what = "mbnb_router_topk_softmax";
    if (!known_dtype(x_dtype) || !known_dtype(rw_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_ROUTER_ERR_ARG, "%s: unknown dtype (x %d, bias %d, rw %d)", what, x_dtype, bias_dtype, rw_dtype);
    if (!mbnb::is16(x_dtype)) return fail(MBNB_ROUTER_ERR_ARG, "%s: 16-bit activations and router weight only (f16 or bf16)", what);
    if (K <= 0 || K % 8) return fail(MBNB_ROUTER_ERR_SHAPE, "%s: K = %lld is not a positive multiple of 8", what, (long long)K);
    if (K > MBNB_ROUTER_MAX_K)
        return fail(MBNB_ROUTER_ERR_SHAPE, "%s: K = %lld, at most %d (one row in LDS)", what, (long long)K, MBNB_ROUTER_MAX_K);
    if (E <= 0) return fail(MBNB_ROUTER_ERR_SHAPE, "%s: E = %lld", what, (long long)E);
    if (E > MBNB_ROUTER_MAX_EXPERTS)
        return fail(MBNB_ROUTER_ERR_SHAPE, "%s: E = %lld experts, at most %d", what, (long long)E, MBNB_ROUTER_MAX_EXPERTS);
    if (A < 1 || A > E || A > MBNB_ROUTER_MAX_TOPK)
        return fail(MBNB_ROUTER_ERR_SHAPE, "%s: top_k A = %lld is not in [1, min(E = %lld, %d)]", what, (long long)A, (long long)E,
                    MBNB_ROUTER_MAX_TOPK);
    if (T < 0 || T > INT32_MAX)
        return fail(MBNB_ROUTER_ERR_SHAPE, "%s: T = %lld tokens, 0 to 2^31 - 1 workgroups in one launch", what, (long long)T);
    if (T == 0) return 0;
    if (!x || !w || !ids || !rw) return fail(MBNB_ROUTER_ERR_ARG, "%s: NULL x, w, ids or rw", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w, 16)) return fail(MBNB_ROUTER_ERR_ARG, "%s: misaligned x or w (16 bytes each)", what);
    if (!mbnb::aligned(ids, 4) || (logits_out && !mbnb::aligned(logits_out, 4)))
        return fail(MBNB_ROUTER_ERR_ARG, "%s: misaligned ids or logits_out (4 bytes each)", what);
    if (!mbnb::aligned(rw, mbnb::esize(rw_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_ROUTER_ERR_ARG, "%s: misaligned rw or bias (the element size each)", what);
    hipStream_t s = (hipStream_t)stream;
    const int st = x_dtype == MBNB_ROUTER_BF16 ? launch<bf16_t>(x, w, bias, bias_dtype, T, K, E, A, ids, rw, rw_dtype, logits_out, s)
                                               : launch<f16_t>(x, w, bias, bias_dtype, T, K, E, A, ids, rw, rw_dtype, logits_out, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "router %s E%lld K%lld A%lld T%lld", name16(x_dtype), (long long)E, (long long)K,
                 (long long)A, (long long)T);
    return st;
}

}  // extern "C"
