// optim_kernels.hip — fused 8-bit optimizer steps (Adam / AdamW / Lion / SGD momentum) and the C ABI of
// libmbnb_optim.so (include/mbnb_optim.h).
//
// One pass per step: every block of state is read once (parameter, gradient, 8-bit codes, the block's old
// maxima), dequantised, updated in f32, its new maxima reduced in registers, requantised and written once
// (parameter, codes, maxima).  The f32 moments never reach memory.  The rules restate the reference's Python
// path (mps_bitsandbytes/optim/*.py) op for op, in its order and with its fusions:
//   torch `add_(x, alpha=a)` = fmaf(x, a, self), `addcmul_(x, x, value=c)` = fmaf(c * x, x, self);
//   `.sqrt()` and every division correctly rounded; `.round()` half to even.
// Non-finite inputs are outside that contract: a NaN moment is stored as code 0 and a NaN is never a block
// maximum (fmaxf drops it); an infinite maximum gives codes 0 for its block.  Nothing here can fault on them.
#include "../../include/mbnb_optim.h"
#include "host.h"

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

constexpr int kThreads = 256;          // every launch: 4 waves
constexpr int kFastBlock = 256;        // the wave-per-block path: 64 lanes x 4 elements

struct OptimArgs {
    mbnb_optim_scalars s;
    int32_t n;
    int32_t pad_;
    int64_t block_size;
    int64_t first_block[MBNB_OPTIM_MAX_TENSORS + 1];   // cumulative block counts: tensor i owns [first_block[i], first_block[i+1])
    mbnb_optim_tensor t[MBNB_OPTIM_MAX_TENSORS];
};
static_assert(sizeof(OptimArgs) <= 4096, "the descriptor table must fit the kernel-argument segment");

// x rounded (RNE) to T and back.  The empty asm keeps the compiler from folding a preceding multiply or add into a
// mixed-precision op that would round the exact result once: the reference rounds to f32 first, then to T.
template <typename T> __device__ __forceinline__ float rnd(float x) {
    asm("" : "+v"(x));
    return (float)(T)x;
}
template <> __device__ __forceinline__ float rnd<float>(float x) { return x; }

template <typename T> __device__ __forceinline__ T store_as(float x) {
    asm("" : "+v"(x));
    return (T)x;
}

// IEEE division and square root, correctly rounded: what plain `/` and sqrtf lower to under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.  (HIP's __fsqrt_rn is the 1-ulp native v_sqrt_f32 unless the OCML rounded
// operations are enabled, so it is not used here.)
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
    return x;
}

// ---------------------------------------------------------------- state codes (adam8bit.py quantize_state*, dequantize_state*)
__device__ __forceinline__ float deq_signed(int q, float absmax) { return div_rn((float)q, 127.0f) * absmax; }
__device__ __forceinline__ float deq_unsigned(int q, float mx) {
    const float s = div_rn((float)q, 255.0f);
    return (s * s) * mx;
}
__device__ __forceinline__ int8_t q_signed(float x, float absmax) {
    float r = rintf(div_rn(x, absmax) * 127.0f);
    r = r == r ? fminf(fmaxf(r, -127.0f), 127.0f) : 0.0f;
    return (int8_t)(int)r;
}
__device__ __forceinline__ uint8_t q_unsigned(float x, float mx) {
    float r = rintf(sqrt_rn(div_rn(fmaxf(x, 0.0f), mx)) * 255.0f);
    r = r == r ? fminf(fmaxf(r, 0.0f), 255.0f) : 0.0f;
    return (uint8_t)(int)r;
}

// ---------------------------------------------------------------- the rules, per element, in f32
// p, g: the parameter and gradient values; m, v: the dequantised moments (updated in place).  Returns the new
// parameter value, already rounded to PT.
template <int KIND, typename PT, typename GT>
__device__ __forceinline__ float rule(const mbnb_optim_scalars &s, const mbnb_optim_tensor &t, float p, float g, float &m,
                                      float &v) {
    const bool wd = s.flags & MBNB_OPTIM_WEIGHT_DECAY;
    if constexpr (KIND == MBNB_OPTIM_ADAM || KIND == MBNB_OPTIM_ADAMW) {
        if (KIND == MBNB_OPTIM_ADAM && wd) g = fmaf(p, s.weight_decay, g);      // grad.add(p.float(), alpha=wd)
        if (KIND == MBNB_OPTIM_ADAMW && wd) p = rnd<PT>(p * s.decay);          // p.mul_(1 - lr * wd)
        m = fmaf(g, s.one_minus_beta1, m * s.beta1);                            // exp_avg.mul_(b1).add_(g, alpha=1-b1)
        v = fmaf(s.one_minus_beta2 * g, g, v * s.beta2);                        // exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2)
        const float den = div_rn(sqrt_rn(v), t.bc2_sqrt) + s.eps;         // (sqrt(v) / bc2 ** 0.5).add_(eps)
        const float u = div_rn(m, den) * t.neg_step_size;                    // exp_avg / denom * (-step_size)
        return rnd<PT>(p + rnd<PT>(u));                                         // p.add_(update.to(p.dtype))
    } else if constexpr (KIND == MBNB_OPTIM_LION) {
        if (wd) p = rnd<PT>(p * s.decay);
        const float u = fmaf(g, s.one_minus_beta1, m * s.beta1);                // exp_avg.mul(b1).add(g, alpha=1-b1)
        const float sg = (float)((u > 0.0f) - (u < 0.0f));                      // update.sign()
        m = fmaf(g, s.one_minus_beta2, m * s.beta2);
        return rnd<PT>(fmaf(sg, s.neg_lr, p));                                  // p.add_(sign, alpha=-lr)
    } else {                                                                    // SGD with momentum
        if (wd) g = rnd<GT>(fmaf(p, s.weight_decay, g));                        // grad.add(p, alpha=wd), in the grad dtype
        m = fmaf(g, s.one_minus_beta1, m * s.beta1);                            // buf.mul_(momentum).add_(g, alpha=1-dampening)
        float d = KIND == MBNB_OPTIM_SGD_NESTEROV ? fmaf(m, s.beta1, g) : m;    // g.add(buf, alpha=momentum) or buf
        d = rnd<PT>(d);                                                         // .to(p.dtype)
        return rnd<PT>(fmaf(d, s.neg_lr, p));                                   // p.add_(grad, alpha=-lr)
    }
}

template <int KIND> constexpr bool kTwoMoments = KIND == MBNB_OPTIM_ADAM || KIND == MBNB_OPTIM_ADAMW;

// the tensor that owns global block `blk` (wave-uniform: the table lives in the kernel arguments)
__device__ __forceinline__ int owner(const OptimArgs &a, int64_t blk) {
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first_block[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------- block 256: one wave per block, 4 contiguous elements per lane
template <int KIND, typename PT, typename GT>
__global__ __launch_bounds__(kThreads) void k_optim8_wave(const OptimArgs a) {
    typedef PT pvec __attribute__((ext_vector_type(4)));
    typedef GT gvec __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (blk >= a.first_block[a.n]) return;                                      // whole waves only
    const int ti = owner(a, blk);
    const mbnb_optim_tensor &t = a.t[ti];
    const int64_t lb = blk - a.first_block[ti];
    const int64_t e0 = lb * kFastBlock + lane * 4;
    PT *P = (PT *)t.param + e0;
    const GT *G = (const GT *)t.grad + e0;
    int8_t *Q1 = (int8_t *)t.state1 + e0;
    uint8_t *Q2 = (uint8_t *)t.state2 + e0;
    const float am1 = t.absmax1[lb];
    const float am2 = kTwoMoments<KIND> ? t.max2[lb] : 0.0f;
    const bool full = e0 + 4 <= t.numel;
    const int cnt = full ? 4 : (e0 < t.numel ? (int)(t.numel - e0) : 0);

    float p[4], g[4], m[4], v[4];
    if (full) {
        const pvec pv = *(const pvec *)P;
        const gvec gv = *(const gvec *)G;
        const uint32_t q1 = *(const uint32_t *)Q1;
        const uint32_t q2 = kTwoMoments<KIND> ? *(const uint32_t *)Q2 : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = (float)pv[j];
            g[j] = (float)gv[j];
            m[j] = deq_signed((int8_t)(q1 >> (8 * j)), am1);
            v[j] = kTwoMoments<KIND> ? deq_unsigned((q2 >> (8 * j)) & 0xff, am2) : 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = j < cnt;
            p[j] = in ? (float)P[j] : 0.0f;
            g[j] = in ? (float)G[j] : 0.0f;
            m[j] = in ? deq_signed(Q1[j], am1) : 0.0f;
            v[j] = in && kTwoMoments<KIND> ? deq_unsigned(Q2[j], am2) : 0.0f;
        }
    }
    float mx1 = 0.0f, mx2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            p[j] = rule<KIND, PT, GT>(a.s, t, p[j], g[j], m[j], v[j]);
            mx1 = fmaxf(mx1, fabsf(m[j]));
            mx2 = fmaxf(mx2, fmaxf(v[j], 0.0f));
        }
    }
    mx1 = fmaxf(wave_max(mx1), 1e-8f);                                          // .clamp(min=1e-8); padding counts as 0
    if (kTwoMoments<KIND>) mx2 = fmaxf(wave_max(mx2), 1e-12f);
    if (full) {
        pvec pv;
        uint32_t q1 = 0, q2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pv[j] = store_as<PT>(p[j]);
            q1 |= (uint32_t)(uint8_t)q_signed(m[j], mx1) << (8 * j);
            if (kTwoMoments<KIND>) q2 |= (uint32_t)q_unsigned(v[j], mx2) << (8 * j);
        }
        *(pvec *)P = pv;
        *(uint32_t *)Q1 = q1;
        if (kTwoMoments<KIND>) *(uint32_t *)Q2 = q2;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                P[j] = store_as<PT>(p[j]);
                Q1[j] = q_signed(m[j], mx1);
                if (kTwoMoments<KIND>) Q2[j] = q_unsigned(v[j], mx2);
            }
        }
    }
    if (lane == 0) {                                                            // one lane, ordinary vector store
        t.absmax1[lb] = mx1;
        if (kTwoMoments<KIND>) t.max2[lb] = mx2;
    }
}

// ---------------------------------------------------------------- any block size: one workgroup per block, two passes
// Pass 1 computes the new moments and reduces the block's maxima (LDS across the 4 waves) without writing; pass 2
// recomputes the same values from the same inputs (each element is owned by the same thread in both passes, so
// nothing it reads has been written yet) and writes the parameter and the codes.  Slow for large blocks, exact.
template <int KIND, typename PT, typename GT>
__global__ __launch_bounds__(kThreads) void k_optim8_generic(const OptimArgs a) {
    __shared__ float red[2][kThreads / 64];
    const int64_t blk = blockIdx.x;
    if (blk >= a.first_block[a.n]) return;                                      // whole workgroups only
    const int ti = owner(a, blk);
    const mbnb_optim_tensor &t = a.t[ti];
    const int64_t lb = blk - a.first_block[ti];
    const int64_t base = lb * a.block_size;
    const int64_t rem = t.numel - base;
    const int64_t cnt = rem < a.block_size ? rem : a.block_size;
    PT *P = (PT *)t.param + base;
    const GT *G = (const GT *)t.grad + base;
    int8_t *Q1 = (int8_t *)t.state1 + base;
    uint8_t *Q2 = (uint8_t *)t.state2 + base;
    const float am1 = t.absmax1[lb];
    const float am2 = kTwoMoments<KIND> ? t.max2[lb] : 0.0f;

    float mx1 = 0.0f, mx2 = 0.0f;
    for (int64_t i = threadIdx.x; i < cnt; i += kThreads) {
        float m = deq_signed(Q1[i], am1);
        float v = kTwoMoments<KIND> ? deq_unsigned(Q2[i], am2) : 0.0f;
        rule<KIND, PT, GT>(a.s, t, (float)P[i], (float)G[i], m, v);
        mx1 = fmaxf(mx1, fabsf(m));
        mx2 = fmaxf(mx2, fmaxf(v, 0.0f));
    }
    mx1 = wave_max(mx1);
    mx2 = wave_max(mx2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mx1;
        red[1][threadIdx.x >> 6] = mx2;
    }
    __syncthreads();                                                            // also: every thread has read am1 / am2
    mx1 = mx2 = 0.0f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        mx1 = fmaxf(mx1, red[0][w]);
        mx2 = fmaxf(mx2, red[1][w]);
    }
    mx1 = fmaxf(mx1, 1e-8f);
    mx2 = fmaxf(mx2, 1e-12f);
    for (int64_t i = threadIdx.x; i < cnt; i += kThreads) {
        float m = deq_signed(Q1[i], am1);
        float v = kTwoMoments<KIND> ? deq_unsigned(Q2[i], am2) : 0.0f;
        const float p = rule<KIND, PT, GT>(a.s, t, (float)P[i], (float)G[i], m, v);
        P[i] = store_as<PT>(p);
        Q1[i] = q_signed(m, mx1);
        if (kTwoMoments<KIND>) Q2[i] = q_unsigned(v, mx2);
    }
    if (threadIdx.x == 0) {
        t.absmax1[lb] = mx1;
        if (kTwoMoments<KIND>) t.max2[lb] = mx2;
    }
}

// ---------------------------------------------------------------- host side
template <int KIND, typename PT, typename GT>
int launch(const OptimArgs &a, bool generic, hipStream_t stream) {
    const int64_t blocks = a.first_block[a.n];
    if (blocks == 0) return 0;
    const int64_t grid = generic ? blocks : (blocks + kThreads / 64 - 1) / (kThreads / 64);
    if (grid > INT32_MAX) return fail(MBNB_OPTIM_ERR_SHAPE, "mbnb_optim_step: %lld blocks exceed one launch", (long long)blocks);
    if (generic)
        hipLaunchKernelGGL((k_optim8_generic<KIND, PT, GT>), dim3((unsigned)grid), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((k_optim8_wave<KIND, PT, GT>), dim3((unsigned)grid), dim3(kThreads), 0, stream, a);
    return mbnb::launch_status("mbnb_optim_step");
}

template <typename PT, typename GT>
int dispatch_kind(int kind, const OptimArgs &a, bool generic, hipStream_t stream) {
    switch (kind) {
    case MBNB_OPTIM_ADAM: return launch<MBNB_OPTIM_ADAM, PT, GT>(a, generic, stream);
    case MBNB_OPTIM_ADAMW: return launch<MBNB_OPTIM_ADAMW, PT, GT>(a, generic, stream);
    case MBNB_OPTIM_LION: return launch<MBNB_OPTIM_LION, PT, GT>(a, generic, stream);
    case MBNB_OPTIM_SGD_MOMENTUM: return launch<MBNB_OPTIM_SGD_MOMENTUM, PT, GT>(a, generic, stream);
    default: return launch<MBNB_OPTIM_SGD_NESTEROV, PT, GT>(a, generic, stream);
    }
}

template <typename PT>
int dispatch_grad(int kind, int grad_dtype, const OptimArgs &a, bool generic, hipStream_t stream) {
    if (grad_dtype == MBNB_OPTIM_F32) return dispatch_kind<PT, float>(kind, a, generic, stream);
    return dispatch_kind<PT, PT>(kind, a, generic, stream);
}

}  // namespace

extern "C" {

int mbnb_optim_abi_version(void) { return MBNB_OPTIM_ABI_VERSION; }

const char *mbnb_optim_last_error(void) { return mbnb::last_error(); }

int mbnb_optim_step(int kind, int param_dtype, int grad_dtype, int64_t block_size, const mbnb_optim_scalars *scalars,
                    const mbnb_optim_tensor *table, int n, int flags, void *stream) {
    if (kind < MBNB_OPTIM_ADAM || kind > MBNB_OPTIM_SGD_NESTEROV)
        return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: unknown optimizer kind %d", kind);
    if (param_dtype < MBNB_OPTIM_F16 || param_dtype > MBNB_OPTIM_F32)
        return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: unknown parameter dtype %d", param_dtype);
    if (grad_dtype != param_dtype && grad_dtype != MBNB_OPTIM_F32)
        return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: gradient dtype %d must be the parameter dtype %d or f32", grad_dtype,
                    param_dtype);
    if (block_size <= 0) return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: block_size must be positive, got %lld", (long long)block_size);
    if (flags & ~MBNB_OPTIM_FORCE_GENERIC) return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: unknown flags 0x%x", flags);
    if (n < 0 || n > MBNB_OPTIM_MAX_TENSORS)
        return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: n = %d tensors, 0..%d per call", n, MBNB_OPTIM_MAX_TENSORS);
    if (n == 0) return 0;
    if (!scalars || !table) return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: NULL scalars or table");
    const bool two = kind == MBNB_OPTIM_ADAM || kind == MBNB_OPTIM_ADAMW;
    const int psize = param_dtype == MBNB_OPTIM_F32 ? 4 : 2;
    OptimArgs a;
    a.s = *scalars;
    a.n = n;
    a.pad_ = 0;
    a.block_size = block_size;
    a.first_block[0] = 0;
    for (int i = 0; i < n; ++i) {
        const mbnb_optim_tensor &t = table[i];
        if (t.numel < 0) return fail(MBNB_OPTIM_ERR_SHAPE, "mbnb_optim_step: tensor %d has numel %lld", i, (long long)t.numel);
        if (t.numel > 0) {
            if (!t.param || !t.grad || !t.state1 || !t.absmax1 || (two && (!t.state2 || !t.max2)))
                return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: tensor %d has a NULL pointer", i);
            if (((uintptr_t)t.param | (uintptr_t)t.grad) % 16 || ((uintptr_t)t.state1 | (two ? (uintptr_t)t.state2 : 0)) % 4)
                return fail(MBNB_OPTIM_ERR_ARG, "mbnb_optim_step: tensor %d is misaligned (parameter and gradient need 16 bytes, codes 4)", i);
            if (t.numel > INT64_MAX / psize) return fail(MBNB_OPTIM_ERR_SHAPE, "mbnb_optim_step: tensor %d is too large", i);
        }
        a.t[i] = t;
        a.first_block[i + 1] = a.first_block[i] + (t.numel + block_size - 1) / block_size;
    }
    const bool generic = block_size != kFastBlock || (flags & MBNB_OPTIM_FORCE_GENERIC);
    hipStream_t s = (hipStream_t)stream;
    switch (param_dtype) {
    case MBNB_OPTIM_F16: return dispatch_grad<f16_t>(kind, grad_dtype, a, generic, s);
    case MBNB_OPTIM_BF16: return dispatch_grad<bf16_t>(kind, grad_dtype, a, generic, s);
    default: return dispatch_kind<float, float>(kind, a, generic, s);
    }
}

}  // extern "C"
