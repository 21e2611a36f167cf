// moemlp_kernels.hip — the MXFP4 mixture-of-experts MLP of a decode batch, and the C ABI of libmbnb_moemlp.so
// (include/mbnb_moemlp.h).
//
//   k_mx_experts_rt  k_mx_experts (moe_kernels.hip) on a grid sized by the routing: ceil(N / 16) weight tiles x
//                    R = min(E, P) rows.  Workgroup (tile, j) finds the j-th smallest distinct id in [0, E) of the call on its own
//                    (a presence byte per expert in LDS, walked 64 experts per step with a ballot), leaves when there are fewer,
//                    and is k_mx_experts' workgroup from there on: the one pair list and the one decode tile of mx_decode.h, so
//                    `pre` carries the bits that kernel writes in f32.  Two epilogues: Glu exchanges the (gate, up) columns of
//                    a tile between neighbour lanes and stores the gated activation; PlainF32 stores the f32 value into the
//                    workspace.
//   k_routed_sum     out[t, n] = the fmaf chain over the slots of token t, in slot order, one thread per output.
#include "../../include/mbnb_moemlp.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MOEMLP_F16 == mbnb::kF16 && MBNB_MOEMLP_BF16 == mbnb::kBF16 && MBNB_MOEMLP_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOEMLP_MAX_PAIRS == mbnb::mx::kMaxPairs, "mx_decode.h's pair list");
static_assert(MBNB_MOEMLP_ERR_ARG == mbnb::mx::kErrArg && MBNB_MOEMLP_ERR_SHAPE == mbnb::mx::kErrShape, "mx_decode.h's statuses");
static_assert(MBNB_MOEMLP_MAX_EXPERTS == 1024, "the presence array is zeroed by 256 threads, 4 bytes each");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;
using mbnb::mx::v4f;
using mbnb::mx::kMfmaWaves;
using mbnb::mx::kMaxPairs;
using mbnb::mx::kPairRows;
using mbnb::mx::load_bias;
using mbnb::mx::store_out;
using mbnb::mx::TileLds;
using mbnb::mx::TileSums;
using mbnb::mx::PairCounts;
using mbnb::mx::tile_walk;
using mbnb::mx::tile_reduce;
using mbnb::mx::list_pairs;
using mbnb::mx::lane_rank;
using mbnb::mx::check_expert_call;
using mbnb::mx::check_expert_pointers;
using mbnb::mx::check_expert_nulls;
using mbnb::mx::check_expert_alignment;

constexpr int kMaxExperts = MBNB_MOEMLP_MAX_EXPERTS;
constexpr int kSumThreads = 256;

struct Glu { static constexpr bool kGlu = true; };
struct PlainF32 { static constexpr bool kGlu = false; };

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

// Workgroup (tile, j).  The expert: every id in [0, E) sets its presence byte (plain stores of the same value: no order matters),
// and after the barrier every wave walks the bytes 64 experts per step, so every wave knows `e` without another barrier.  From
// there on the pair list and the decode tile are mx_decode.h's (list_pairs, tile_walk, tile_reduce), the functions k_mx_experts
// calls; row j == 0 takes the part of that kernel's expert 0 and, with Glu, also lists the out-of-range pairs and stores their
// zeros (with PlainF32 nothing is stored for them: k_routed_sum never reads their rows).  When no id is in range, row 0 has no
// expert and only stores those zeros.  What is this kernel's own: the presence walk, the loop over passes of 16 listed pairs,
// and the two epilogues.
template <typename T, typename EPI>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mx_experts_rt(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                    const uint8_t *__restrict__ Ws, const int32_t *__restrict__ ids, int P,
                                                                    int x_div, int E, int64_t N, int64_t K, const void *__restrict__ bias,
                                                                    int bias_dtype, void *__restrict__ out, int out_dtype, int tiles,
                                                                    float alpha, float limit) {
    __shared__ TileLds lds;
    __shared__ uint16_t list[kMaxPairs];
    __shared__ uint32_t present_words[kMaxExperts / 4];
    uint8_t *present = (uint8_t *)present_words;
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = blockIdx.x / tiles;
    const int64_t n0 = (int64_t)(blockIdx.x % tiles) * 16;

    if (tid < kMaxExperts / 4) present_words[tid] = 0u;
    __syncthreads();
    for (int p = tid; p < P; p += 64 * kMfmaWaves) {
        const int id = ids[p];
        if (id >= 0 && id < E) present[id] = 1;
    }
    __syncthreads();
    int e = -1;
    for (int base = 0, seen = 0; base < E; base += 64) {     // uniform: the ballot gives every lane the same counts
        const bool here = base + lane < E && present[base + lane] != 0;
        const uint64_t bm = __ballot(here);
        const int c = __popcll(bm);
        if (seen + c > j) {
            e = base + (int)__builtin_ctzll(__ballot(here && lane_rank(bm) == j - seen));
            break;
        }
        seen += c;
    }
    const bool lists_zeros = EPI::kGlu && j == 0;
    if (e < 0 && !lists_zeros) return;                       // fewer than j + 1 distinct experts: no weight byte is touched

    const PairCounts pairs = list_pairs(ids, P, e, E, lists_zeros, wave, lane, list);
    const int count = pairs.count, zeros = pairs.zeros;
    if (count == 0 && zeros == 0) return;                    // uniform
    __syncthreads();

    if (EPI::kGlu) {                                         // the rows of +0.0 of the out-of-range pairs, this tile's 8 outputs
        const int64_t I = N / 2;
        for (int i = tid >> 3; i < zeros; i += (64 * kMfmaWaves) >> 3) {
            const int64_t col = n0 / 2 + (tid & 7);
            if (col < I) store_out(out, out_dtype, (int64_t)list[kMaxPairs - 1 - i] * I + col, 0.0f);
        }
    }
    if (count == 0) return;                                  // uniform: row 0 of a call with no id in range

    const int64_t KB = K / 32, ldw = K / 2;
    const int64_t n = n0 + fr < N ? n0 + fr : N - 1;         // a column past N reads the last weight row and stores nothing
    const uint8_t *w_row = W + ((int64_t)e * N + n) * ldw, *s_row = Ws + ((int64_t)e * N + n) * KB;

    for (int c16 = 0; c16 < count; c16 += kPairRows) {
        const bool x_live = c16 + fr < count;
        const int pair = x_live ? (int)list[c16 + fr] : 0;
        const T *x_row = x + (int64_t)(x_div == 1 ? pair : pair / x_div) * K + 8 * g;

        const TileSums part = tile_walk<T>(x_row, x_live, w_row, s_row, KB, wave, g);
        const float b = wave == 0 && bias ? load_bias(bias, bias_dtype, (int64_t)e * N + n) : 0.0f;   // requested before the reduction's barrier
        v4f s;
        const bool col_nan = tile_reduce(lds, part, wave, lane, s);
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = c16 + 4 * g + r;
                const float pre = col_nan ? __uint_as_float(0x7FC00000u) : s[r] + b;
                if (EPI::kGlu) {
                    // N = 2I: lanes fr, fr ^ 1 hold (gate, up) of one output, both inside N or both outside; all 64 lanes exchange
                    const float other = __shfl_xor(pre, 1);
                    if (!(fr & 1) && n0 + fr < N && i < count)
                        store_out(out, out_dtype, (int64_t)list[i] * (N / 2) + (n0 + fr) / 2, glu(pre, other, alpha, limit));
                } else if (n0 + fr < N && i < count) {
                    ((float *)out)[(int64_t)list[i] * N + n] = pre;
                }
            }
        }
        if (c16 + kPairRows < count) __syncthreads();        // uniform: wave 0 is done with the sums before the next pass writes them
    }
}

// One thread per out[t, n].  A skipped pair's routing weight and workspace row are not read.
__global__ __launch_bounds__(kSumThreads) void k_routed_sum(const float *__restrict__ ws, const int32_t *__restrict__ ids,
                                                            const void *__restrict__ rw, int rw_dtype, int64_t T, int A, int E, int64_t N,
                                                            void *__restrict__ out, int out_dtype) {
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

// ---------------------------------------------------------------- host side
bool known_dtype(int d) { return d >= MBNB_MOEMLP_F16 && d <= MBNB_MOEMLP_F32; }
const char *name16(int d) { return d == MBNB_MOEMLP_BF16 ? "bf16" : "f16"; }

template <typename T, typename EPI>
int launch_rt(const void *x, const void *W, const void *Ws, const int32_t *ids, int64_t P, int64_t x_div, int64_t E, int64_t N, int64_t K,
              const void *bias, int bias_dtype, void *out, int out_dtype, float alpha, float limit, hipStream_t s) {
    const int64_t tiles = (N + 15) / 16, R = E < P ? E : P;
    hipLaunchKernelGGL((k_mx_experts_rt<T, EPI>), dim3((unsigned)(tiles * R)), dim3(64 * kMfmaWaves), 0, s, (const T *)x, (const uint8_t *)W,
                       (const uint8_t *)Ws, ids, (int)P, (int)x_div, (int)E, N, K, bias, bias_dtype, out, out_dtype, (int)tiles, alpha, limit);
    return mbnb::launch_status("k_mx_experts_rt");
}

int64_t ws_bytes(int64_t P, int64_t N) { return mbnb::round256(P * N * 4); }

}  // namespace

extern "C" {

int mbnb_moemlp_abi_version(void) { return MBNB_MOEMLP_ABI_VERSION; }

const char *mbnb_moemlp_last_error(void) { return mbnb::last_error(); }

const char *mbnb_moemlp_last_launch(void) { return mbnb::last_launch(); }

int mbnb_moemlp_gate_up_glu(const void *x, int64_t T, int64_t A, int64_t K, int x_dtype, const void *w_codes, const void *w_scales,
                            int64_t E, int64_t I, const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit, void *out,
                            int out_dtype, void *stream) {
    const char *const what = "mbnb_moemlp_gate_up_glu";
    if (I <= 0 || I > mbnb::kMaxElems / 2) return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: I = %lld", what, (long long)I);
    const int64_t N = 2 * I;
    if (const int st = check_expert_call(what, T, A, K, x_dtype, E, N, bias_dtype, bias != nullptr, out_dtype, kMaxExperts, true)) return st;
    if (!(alpha - alpha == 0.0f)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: alpha = %g is not finite", what, (double)alpha);
    if (!(limit > 0.0f)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: limit = %g is not positive (+Inf: no clamp)", what, (double)limit);
    const int64_t P = T * A;
    if (P == 0) return 0;
    if (const int st = check_expert_pointers(what, {{"x", x, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                    {"out", out, mbnb::esize(out_dtype)}, {"bias", bias, mbnb::esize(bias_dtype), true}}))
        return st;
    hipStream_t s = (hipStream_t)stream;
    const int st = x_dtype == MBNB_MOEMLP_BF16
                       ? launch_rt<bf16_t, Glu>(x, w_codes, w_scales, ids, P, A, E, N, K, bias, bias_dtype, out, out_dtype, alpha, limit, s)
                       : launch_rt<f16_t, Glu>(x, w_codes, w_scales, ids, P, A, E, N, K, bias, bias_dtype, out, out_dtype, alpha, limit, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_glu %s E%lld P%lld R%lld", name16(x_dtype), (long long)E, (long long)P,
                 (long long)(E < P ? E : P));
    return st;
}

int64_t mbnb_moemlp_workspace_bytes(int64_t T, int64_t A, int64_t N) {
    const char *const what = "mbnb_moemlp_workspace_bytes";
    if (T < 0 || A < 0 || N <= 0) return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: T = %lld, A = %lld, N = %lld", what, (long long)T, (long long)A, (long long)N);
    if (T > 0 && A > MBNB_MOEMLP_MAX_PAIRS / T)
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: T x A = %lld x %lld pairs, at most %d in one call", what, (long long)T, (long long)A, MBNB_MOEMLP_MAX_PAIRS);
    if (T * A > 0 && N > mbnb::kMaxElems / (T * A))
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: %lld x %lld outputs exceed one launch", what, (long long)(T * A), (long long)N);
    return ws_bytes(T * A, N);
}

int mbnb_moemlp_down_sum(const void *h, int64_t T, int64_t A, int64_t K, int h_dtype, const void *w_codes, const void *w_scales, int64_t E,
                         int64_t N, const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype, void *out,
                         int out_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *const what = "mbnb_moemlp_down_sum";
    if (const int st = check_expert_call(what, T, A, K, h_dtype, E, N, bias_dtype, bias != nullptr, out_dtype, kMaxExperts, true)) return st;
    if (!known_dtype(rw_dtype)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: unknown dtype (rw %d)", what, rw_dtype);
    const int64_t P = T * A;
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"h", h, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                               {"rw", rw, mbnb::esize(rw_dtype)}, {"out", out, mbnb::esize(out_dtype)},
                                                               {"bias", bias, mbnb::esize(bias_dtype), true}, {"workspace", workspace, 16, true}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (!workspace || workspace_bytes < ws_bytes(P, N))
        return fail(MBNB_MOEMLP_ERR_WORKSPACE, "%s: the workspace is NULL or holds %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)ws_bytes(P, N));
    if (const int st = check_expert_alignment(what, operands)) return st;
    hipStream_t s = (hipStream_t)stream;
    int st = h_dtype == MBNB_MOEMLP_BF16
                 ? launch_rt<bf16_t, PlainF32>(h, w_codes, w_scales, ids, P, 1, E, N, K, bias, bias_dtype, workspace, MBNB_MOEMLP_F32, 0.0f, 0.0f, s)
                 : launch_rt<f16_t, PlainF32>(h, w_codes, w_scales, ids, P, 1, E, N, K, bias, bias_dtype, workspace, MBNB_MOEMLP_F32, 0.0f, 0.0f, s);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_routed_sum, dim3((unsigned)((T * N + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads), 0, s, (const float *)workspace,
                       ids, rw, rw_dtype, T, (int)A, (int)E, N, out, out_dtype);
    st = mbnb::launch_status("k_routed_sum");
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_down_sum %s E%lld P%lld R%lld A%lld", name16(h_dtype), (long long)E, (long long)P,
                 (long long)(E < P ? E : P), (long long)A);
    return st;
}

}  // extern "C"
