// mx_experts.h — what the two MXFP4 expert MLP libraries share on top of mx_decode.h: moemlp_kernels.hip
// (k_mx_experts_rt, the decode route) and moegemm_kernels.hip (k_mx_experts_grouped, the prefill route).  What makes the two routes
// bit-equal after the decode tile is here and nowhere else.
//
//   device   glu (the gated activation), glu_store (the Glu epilogue's lane exchange and store) and k_routed_sum, the fmaf chain
//            over the slots of a token.
//   host     launch_routed_sum, and the refusals both libraries word alike: check_glu_params, check_workspace; ws_bytes,
//            known_dtype, name16.
// A header of its own, not more of mx_decode.h: mx_kernels.hip and moe_kernels.hip include that one and get no k_routed_sum.
#pragma once

#include "mx_decode.h"

namespace mbnb {
namespace mx {

// The gated activation, every operation a separate f32 rounding (-ffp-contract=off), the division IEEE, expf OCML's.
__device__ __forceinline__ float glu(float g, float u, float alpha, float limit) {
    g = g > limit ? limit : g;
    u = u > limit ? limit : (u < -limit ? -limit : u);
    const float t = alpha * g;
    const float den = 1.0f + expf(-t);
    const float sig = 1.0f / den;
    const float gs = g * sig;
    const float up = u + 1.0f;
    return up * gs;
}

// The Glu epilogue of a lane that holds `pre` of column `col` (lane fr of its 16) of pair `row`.  N = 2I: lanes fr, fr ^ 1 hold
// (gate, up) of one output, both inside N or both outside.  All 64 lanes exchange, so the call stands outside any divergent
// branch; the even lane of a column that `stores` (inside N, of a listed pair) writes the output.
__device__ __forceinline__ void glu_store(float pre, int fr, bool stores, void *out, int out_dtype, int64_t row, int64_t N, int64_t col,
                                          float alpha, float limit) {
    const float other = __shfl_xor(pre, 1);
    if (stores && !(fr & 1)) store_out(out, out_dtype, row * (N / 2) + col / 2, glu(pre, other, alpha, limit));
}

constexpr int kSumThreads = 256;

// One thread per out[t, n].  A skipped pair's routing weight and workspace row are not read.
static __global__ __launch_bounds__(kSumThreads) void k_routed_sum(const float *__restrict__ ws, const int32_t *__restrict__ ids,
                                                                   const void *__restrict__ rw, int rw_dtype, int64_t T, int A, int E,
                                                                   int64_t N, void *__restrict__ out, int out_dtype) {
    const int64_t i = (int64_t)blockIdx.x * kSumThreads + threadIdx.x;
    if (i >= T * N) return;
    const int64_t t = i / N, n = i - t * N;
    float acc = 0.0f;
    for (int a = 0; a < A; ++a) {
        const int64_t p = t * A + a;
        const int id = ids[p];
        if (id < 0 || id >= E) continue;
        acc = __builtin_fmaf(load_bias(rw, rw_dtype, p), ws[p * N + n], acc);
    }
    store_out(out, out_dtype, i, acc);
}

// ---------------------------------------------------------------- host
constexpr int kErrWorkspace = -3;      // beside kErrArg / kErrShape: each library asserts its own

static inline bool known_dtype(int d) { return d >= kF16 && d <= kF32; }
static inline int64_t ws_bytes(int64_t P, int64_t N) { return round256(P * N * 4); }

static inline int launch_routed_sum(const void *ws, const int32_t *ids, const void *rw, int rw_dtype, int64_t T, int64_t A, int64_t E,
                                    int64_t N, void *out, int out_dtype, hipStream_t stream) {
    hipLaunchKernelGGL(k_routed_sum, dim3((unsigned)((T * N + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads), 0, stream,
                       (const float *)ws, ids, rw, rw_dtype, T, (int)A, (int)E, N, out, out_dtype);
    return launch_status("k_routed_sum");
}

static inline int check_glu_params(const char *what, float alpha, float limit) {
    if (!(alpha - alpha == 0.0f)) return fail(kErrArg, "%s: alpha = %g is not finite", what, (double)alpha);
    if (!(limit > 0.0f)) return fail(kErrArg, "%s: limit = %g is not positive (+Inf: no clamp)", what, (double)limit);
    return 0;
}

static inline int check_workspace(const char *what, const void *workspace, int64_t workspace_bytes, int64_t P, int64_t N) {
    if (!workspace || workspace_bytes < ws_bytes(P, N))
        return fail(kErrWorkspace, "%s: the workspace is NULL or holds %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)ws_bytes(P, N));
    return 0;
}

}  // namespace mx
}  // namespace mbnb
