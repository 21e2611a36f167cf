// paged_kernels.hip — the fused full-precision optimizer step (Adam / AdamW / Lion) and the C ABI of
// libmbnb_paged.so (include/mbnb_paged.h).
//
// One pass per step: every element of the parameter, the gradient and the moments is read once, updated in f32
// registers and written once.  The rule restates the reference's Python path (mps_bitsandbytes/optim/paged.py) op for
// op on tensors of ONE dtype T, so every tensor op rounds its result to T:
//   torch `mul_(c)` = r(x * s32(c)); `add_(x, alpha=a)` = r(fmaf(x, sT(a), self));
//   `addcmul_(x, x, value=c)` = r(fmaf(s32(c) * x, x, self)); `addcdiv_(m, den, value=c)` = r(self + (s32(c) * m) / den);
//   `.sqrt()` and every division correctly rounded, true divisions, no reciprocals.
// The kernel is purely elementwise over *segments* (element ranges of tensors) and knows nothing about paging: the
// moment pointers are a tensor's own storage or a staging slot.
#include "../../include/mbnb_paged.h"
#include "host.h"

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

constexpr int kThreads = 256;          // every launch: 4 waves
constexpr int kChunks = 4;             // 16-byte chunks per thread and stream: a workgroup covers 16 KiB of each tensor

struct PagedArgs {
    mbnb_paged_scalars s;
    int32_t n;
    int32_t pad_;
    int64_t first_block[MBNB_PAGED_MAX_SEGMENTS + 1];   // cumulative workgroup counts: segment i owns [first_block[i], first_block[i+1])
    mbnb_paged_segment t[MBNB_PAGED_MAX_SEGMENTS];
    uint8_t off[MBNB_PAGED_MAX_SEGMENTS];               // elements between the last 16-byte boundary and the segment's first element
    uint8_t vec[MBNB_PAGED_MAX_SEGMENTS];               // all pointers share that offset: the body moves in 16-byte vectors
};
static_assert(sizeof(PagedArgs) <= 4096, "the segment table must fit the kernel-argument segment");

// x rounded (RNE) to T and back.  The empty asm keeps the compiler from folding a preceding multiply or add into a
// mixed-precision op that would round the exact result once: the reference rounds to f32 first, then to T.
template <typename T> __device__ __forceinline__ float rnd(float x) {
    asm("" : "+v"(x));
    return (float)(T)x;
}
template <> __device__ __forceinline__ float rnd<float>(float x) { return x; }

// IEEE division and square root, correctly rounded: what plain `/` and sqrtf lower to under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

// ---------------------------------------------------------------- the rules, per element, in f32 registers
// p, m, v hold values of T and are updated in place; g is the gradient value.
template <int KIND, typename T>
__device__ __forceinline__ void rule(const mbnb_paged_scalars &s, float bc2_sqrt, float neg_step_size, float &p, float g, float &m,
                                     float &v) {
    const bool wd = s.flags & MBNB_PAGED_WEIGHT_DECAY;
    if constexpr (KIND == MBNB_PAGED_LION) {
        if (wd) p = rnd<T>(p * s.decay);                                        // p.mul_(1 - lr * wd)
        const float u = rnd<T>(fmaf(g, s.one_minus_beta1, rnd<T>(m * s.beta1)));   // exp_avg.mul(b1).add(g, alpha=1-b1)
        const float sg = (float)((u > 0.0f) - (u < 0.0f));                      // update.sign()
        p = rnd<T>(fmaf(sg, s.neg_lr, p));                                      // p.add_(sign, alpha=-lr)
        m = rnd<T>(fmaf(g, s.one_minus_beta2, rnd<T>(m * s.beta2)));            // exp_avg.mul_(b2).add_(g, alpha=1-b2)
    } else {
        if (KIND == MBNB_PAGED_ADAM && wd) g = rnd<T>(fmaf(p, s.weight_decay, g));   // grad.add(p, alpha=wd)
        if (KIND == MBNB_PAGED_ADAMW && wd) p = rnd<T>(p * s.decay);            // p.mul_(1 - lr * wd)
        m = rnd<T>(m * s.beta1);                                                // exp_avg.mul_(b1)
        m = rnd<T>(fmaf(g, s.one_minus_beta1, m));                              //        .add_(g, alpha=1-b1)
        v = rnd<T>(v * s.beta2);                                                // exp_avg_sq.mul_(b2)
        v = rnd<T>(fmaf(s.one_minus_beta2 * g, g, v));                          //           .addcmul_(g, g, value=1-b2)
        const float den = rnd<T>(rnd<T>(div_rn(rnd<T>(sqrt_rn(v)), bc2_sqrt)) + s.eps);   // (v.sqrt() / bc2 ** 0.5).add_(eps)
        p = rnd<T>(p + div_rn(neg_step_size * m, den));                         // p.addcdiv_(m, den, value=-step_size)
    }
}

// the segment that owns workgroup `blk` (uniform: the table lives in the kernel arguments)
__device__ __forceinline__ int owner(const PagedArgs &a, int64_t blk) {
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first_block[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Elements are addressed through a virtual index u = element + off, so that u % VEC == 0 is a 16-byte boundary of every
// pointer of a vectorisable segment.  A chunk [u0, u0 + VEC) that lies inside [off, off + numel) is one vector per
// stream; the head chunk, the tail chunk and every chunk of an unaligned segment go element by element, bounds checked.
template <int KIND, typename T>
__global__ __launch_bounds__(kThreads) void k_paged_step(const PagedArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr bool kTwo = KIND != MBNB_PAGED_LION;
    typedef T tvec __attribute__((ext_vector_type(VEC)));
    const int64_t blk = blockIdx.x;
    if (blk >= a.first_block[a.n]) return;
    const int si = owner(a, blk);
    const mbnb_paged_segment &t = a.t[si];
    const int64_t lb = blk - a.first_block[si];
    const int64_t off = a.off[si];
    const bool vec = a.vec[si];
    const int64_t end = off + t.numel;
    T *P = (T *)t.param;
    const T *G = (const T *)t.grad;
    T *M = (T *)t.exp_avg;
    T *V = (T *)t.exp_avg_sq;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int64_t u0 = ((lb * kChunks + c) * kThreads + threadIdx.x) * VEC;
        if (u0 >= end) continue;
        const int64_t e0 = u0 - off;                                            // may be negative in the head chunk only
        float p[VEC], g[VEC], m[VEC], v[VEC];
        if (vec && u0 >= off && u0 + VEC <= end) {
            const tvec pv = *(const tvec *)(P + e0);
            const tvec gv = *(const tvec *)(G + e0);
            const tvec mv = *(const tvec *)(M + e0);
            tvec vv;
            if (kTwo) vv = *(const tvec *)(V + e0);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                p[j] = (float)pv[j];
                g[j] = (float)gv[j];
                m[j] = (float)mv[j];
                v[j] = kTwo ? (float)vv[j] : 0.0f;
                rule<KIND, T>(a.s, t.bc2_sqrt, t.neg_step_size, p[j], g[j], m[j], v[j]);
            }
            tvec po, mo, vo;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                po[j] = (T)p[j];                                                // already values of T: the casts are exact
                mo[j] = (T)m[j];
                vo[j] = (T)v[j];
            }
            *(tvec *)(P + e0) = po;
            *(tvec *)(M + e0) = mo;
            if (kTwo) *(tvec *)(V + e0) = vo;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int64_t e = e0 + j;
                if (e < 0 || e >= t.numel) continue;
                float pe = (float)P[e], me = (float)M[e], ve = kTwo ? (float)V[e] : 0.0f;
                rule<KIND, T>(a.s, t.bc2_sqrt, t.neg_step_size, pe, (float)G[e], me, ve);
                P[e] = (T)pe;
                M[e] = (T)me;
                if (kTwo) V[e] = (T)ve;
            }
        }
    }
}

// ---------------------------------------------------------------- host side
template <int KIND, typename T>
int launch(const PagedArgs &a, hipStream_t stream) {
    const int64_t blocks = a.first_block[a.n];
    if (blocks == 0) return 0;
    if (blocks > INT32_MAX) return fail(MBNB_PAGED_ERR_SHAPE, "mbnb_paged_step: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL((k_paged_step<KIND, T>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
    return mbnb::launch_status("mbnb_paged_step");
}

template <typename T>
int dispatch_kind(int kind, const PagedArgs &a, hipStream_t stream) {
    switch (kind) {
    case MBNB_PAGED_ADAM: return launch<MBNB_PAGED_ADAM, T>(a, stream);
    case MBNB_PAGED_ADAMW: return launch<MBNB_PAGED_ADAMW, T>(a, stream);
    default: return launch<MBNB_PAGED_LION, T>(a, stream);
    }
}

}  // namespace

extern "C" {

int mbnb_paged_abi_version(void) { return MBNB_PAGED_ABI_VERSION; }

const char *mbnb_paged_last_error(void) { return mbnb::last_error(); }

int mbnb_paged_step(int kind, int dtype, const mbnb_paged_scalars *scalars, const mbnb_paged_segment *table, int n, int flags,
                    void *stream) {
    if (kind < MBNB_PAGED_ADAM || kind > MBNB_PAGED_LION)
        return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: unknown optimizer kind %d", kind);
    if (dtype < MBNB_PAGED_F16 || dtype > MBNB_PAGED_F32) return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: unknown dtype %d", dtype);
    if (flags & ~MBNB_PAGED_FORCE_SCALAR) return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: unknown flags 0x%x", flags);
    if (n < 0 || n > MBNB_PAGED_MAX_SEGMENTS)
        return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: n = %d segments, 0..%d per call", n, MBNB_PAGED_MAX_SEGMENTS);
    if (n == 0) return 0;
    if (!scalars || !table) return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: NULL scalars or table");
    const bool two = kind != MBNB_PAGED_LION;
    const int esize = dtype == MBNB_PAGED_F32 ? 4 : 2;
    const int64_t per_block = (int64_t)kChunks * kThreads * (16 / esize);
    PagedArgs a;
    a.s = *scalars;
    a.n = n;
    a.pad_ = 0;
    a.first_block[0] = 0;
    for (int i = 0; i < n; ++i) {
        const mbnb_paged_segment &t = table[i];
        if (t.numel < 0) return fail(MBNB_PAGED_ERR_SHAPE, "mbnb_paged_step: segment %d has numel %lld", i, (long long)t.numel);
        a.t[i] = t;
        a.off[i] = 0;
        a.vec[i] = 0;
        if (t.numel > 0) {
            if (!t.param || !t.grad || !t.exp_avg || (two && !t.exp_avg_sq))
                return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: segment %d has a NULL pointer", i);
            const uintptr_t ptrs[4] = {(uintptr_t)t.param, (uintptr_t)t.grad, (uintptr_t)t.exp_avg, two ? (uintptr_t)t.exp_avg_sq : (uintptr_t)t.param};
            bool same = true;
            for (int k = 0; k < 4; ++k) {
                if (ptrs[k] % esize)
                    return fail(MBNB_PAGED_ERR_ARG, "mbnb_paged_step: segment %d is misaligned (every pointer needs the element size, %d bytes)", i, esize);
                same = same && ptrs[k] % 16 == ptrs[0] % 16;
            }
            if (t.numel > INT64_MAX / 8) return fail(MBNB_PAGED_ERR_SHAPE, "mbnb_paged_step: segment %d is too large", i);
            if (same && !(flags & MBNB_PAGED_FORCE_SCALAR)) {
                a.vec[i] = 1;
                a.off[i] = (uint8_t)(ptrs[0] % 16 / esize);
            }
        }
        a.first_block[i + 1] = a.first_block[i] + (a.off[i] + t.numel + per_block - 1) / per_block;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
    case MBNB_PAGED_F16: return dispatch_kind<f16_t>(kind, a, s);
    case MBNB_PAGED_BF16: return dispatch_kind<bf16_t>(kind, a, s);
    default: return dispatch_kind<float>(kind, a, s);
    }
}

}  // extern "C"
