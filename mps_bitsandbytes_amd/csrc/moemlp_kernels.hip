// moemlp_kernels.hip — the MXFP4 mixture-of-experts MLP of a decode batch, and the C ABI of libmbnb_moemlp.so
// (include/mbnb_moemlp.h).
//
//   k_mx_experts_rt  k_mx_experts (moe_kernels.hip) on a grid sized by the routing: ceil(N / 16) weight tiles x
//                    R = min(E, P) rows.  Workgroup (tile, j) finds the j-th smallest distinct id in [0, E) of the call on its own
//                    (a presence byte per expert in LDS, walked 64 experts per step with a ballot), leaves when there are fewer,
//                    and is k_mx_experts' workgroup from there on: the same pair list, the same K walk, so `pre` carries the bits
//                    that kernel writes in f32.  Two epilogues: Glu exchanges the (gate, up) columns of a tile between neighbour
//                    lanes and stores the gated activation; PlainF32 stores the f32 value into the workspace.
//   k_routed_sum     out[t, n] = the fmaf chain over the slots of token t, in slot order, one thread per output.
#include "../../include/mbnb_moemlp.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MOEMLP_F16 == mbnb::kF16 && MBNB_MOEMLP_BF16 == mbnb::kBF16 && MBNB_MOEMLP_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOEMLP_MAX_PAIRS <= 65536 && MBNB_MOEMLP_MAX_PAIRS % 64 == 0, "a pair index is 2 bytes in LDS");
static_assert(MBNB_MOEMLP_MAX_EXPERTS == 1024, "the presence array is zeroed by 256 threads, 4 bytes each");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;
using mbnb::mx::v4i;
using mbnb::mx::v4f;
using mbnb::mx::kNaNScale;
using mbnb::mx::kOneScale;
using mbnb::mx::kMfmaWaves;
using mbnb::mx::scale_value;
using mbnb::mx::load_bias;
using mbnb::mx::store_out;
using mbnb::mx::decode8_16;
using mbnb::mx::mfma16;

constexpr int kMaxPairs = MBNB_MOEMLP_MAX_PAIRS;
constexpr int kMaxExperts = MBNB_MOEMLP_MAX_EXPERTS;
constexpr int kRows = 16;              // listed pairs per pass of the decode loop: the rows of the MFMA's A fragment
constexpr int kSumThreads = 256;

struct Glu { static constexpr bool kGlu = true; };
struct PlainF32 { static constexpr bool kGlu = false; };

__device__ __forceinline__ int lane_rank(uint64_t bm) {     // the set bits of bm below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
}

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
// and after the barrier every wave walks the bytes 64 experts per step, so every wave knows `e` without another barrier.  The
// pair list, the decode loop and the reduction below are k_mx_experts', statement for statement; row j == 0 takes the part of
// that kernel's expert 0 and, with Glu, also lists the out-of-range pairs and stores their zeros (with PlainF32 nothing is stored
// for them: k_routed_sum never reads their rows).  When no id is in range, row 0 has no expert and only stores those zeros.
template <typename T, typename EPI>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mx_experts_rt(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                    const uint8_t *__restrict__ Ws, const int32_t *__restrict__ ids, int P,
                                                                    int x_div, int E, int64_t N, int64_t K, const void *__restrict__ bias,
                                                                    int bias_dtype, void *__restrict__ out, int out_dtype, int tiles,
                                                                    float alpha, float limit) {
    static_assert(sizeof(T) == 2, "16-bit activations");
    constexpr int U = 2;                                     // k-steps whose loads are requested before the first of them is used
    __shared__ float red[kMfmaWaves][4][64];
    __shared__ int red_ff[kMfmaWaves][64];
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

    int count = 0, zeros = 0;
    for (int s = 0; s * 64 < P; ++s) {
        const int p = s * 64 + lane;
        const bool in = p < P;
        int id = -1;
        if (in) id = ids[p];
        const bool writer = (s % kMfmaWaves) == wave;        // wave-uniform
        const bool oob = id < 0 || id >= E;
        const bool mine = in && !oob && id == e;
        const uint64_t bm = __ballot(mine);
        if (writer && mine) list[count + lane_rank(bm)] = (uint16_t)p;
        count += __popcll(bm);
        if (lists_zeros) {
            const uint64_t bz = __ballot(in && oob);
            if (writer && in && oob) list[kMaxPairs - 1 - zeros - lane_rank(bz)] = (uint16_t)p;
            zeros += __popcll(bz);
        }
    }
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

    const int64_t KB = K / 32, ldw = K / 2, last = KB - 1;
    const int64_t n = n0 + fr < N ? n0 + fr : N - 1;         // a column past N reads the last weight row and stores nothing
    const uint8_t *w_row = W + ((int64_t)e * N + n) * ldw, *s_row = Ws + ((int64_t)e * N + n) * KB;
    const int64_t steps = (KB + 3) / 4;

    for (int c16 = 0; c16 < count; c16 += kRows) {
        const bool x_live = c16 + fr < count;
        const int pair = x_live ? (int)list[c16 + fr] : 0;
        const T *x_row = x + (int64_t)(x_div == 1 ? pair : pair / x_div) * K + 8 * g;

        v4f acc = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        bool ff = false;
        for (int64_t c0 = wave; c0 < steps; c0 += kMfmaWaves * U) {
            // every load is unconditional, from a clamped (valid) address; what lies past K or the list becomes zeros in registers
            v4i wq[U], xa[U][4];
            uint32_t sb[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t c = c0 + u * kMfmaWaves, blk = 4 * c + g;
                wq[u] = __builtin_nontemporal_load((const v4i *)(w_row + (blk < KB ? blk : last) * 16));
                if (blk >= KB) wq[u] = v4i{0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool in = 4 * c + q < KB;
                    const int64_t b = in ? 4 * c + q : last;
                    sb[u][q] = s_row[b];
                    if (!in) sb[u][q] = (uint32_t)kOneScale;
                    xa[u][q] = *(const v4i *)(x_row + b * 32);
                    if (!(in && x_live)) xa[u][q] = v4i{0, 0, 0, 0};
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c0 + u * kMfmaWaves >= steps) break;         // wave-uniform
                // register q of lane group g holds dword q of block g; after the transpose, dword g of block q
                typedef unsigned v2u __attribute__((ext_vector_type(2)));
                const v2u s02 = __builtin_amdgcn_permlane32_swap((unsigned)wq[u][0], (unsigned)wq[u][2], false, false);
                const v2u s13 = __builtin_amdgcn_permlane32_swap((unsigned)wq[u][1], (unsigned)wq[u][3], false, false);
                const v2u t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                const v2u t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                const uint32_t wb[4] = {t01[0], t01[1], t23[0], t23[1]};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const v4f d = mfma16(xa[u][q], decode8_16<T>(wb[q]), T{});
                    const uint32_t byte = sb[u][q];
                    ff |= byte == (uint32_t)kNaNScale;
                    const float sv = scale_value(byte == (uint32_t)kNaNScale ? (uint32_t)kOneScale : byte);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(d[r], sv, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
        red_ff[wave][lane] = ff;
        __syncthreads();
        if (wave == 0) {                                     // the eight partial sums, in wave order
            bool col_nan = false;
            v4f s = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < kMfmaWaves; ++w) {
                col_nan |= red_ff[w][lane] != 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += red[w][r][lane];
            }
            const float b = bias ? load_bias(bias, bias_dtype, (int64_t)e * N + n) : 0.0f;
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
        if (c16 + kRows < count) __syncthreads();            // uniform: wave 0 is done with the sums before the next pass writes them
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

// the checks the two calls share: rows [., K] of `row_dtype` against [E, N, K] weights for T x A pairs; 0, or the status recorded
int check_common(const char *what, int64_t T, int64_t A, int64_t K, int row_dtype, int64_t E, int64_t N, int bias_dtype, bool has_bias,
                 int out_dtype) {
    if (!known_dtype(row_dtype) || !known_dtype(out_dtype) || (has_bias && !known_dtype(bias_dtype)))
        return fail(MBNB_MOEMLP_ERR_ARG, "%s: unknown dtype (rows %d, bias %d, out %d)", what, row_dtype, bias_dtype, out_dtype);
    if (!mbnb::is16(row_dtype)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: 16-bit activations only (f16 or bf16 rows)", what);
    if (K <= 0 || K % 32) return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: K = %lld is not a positive multiple of the MX block, 32", what, (long long)K);
    if (E <= 0 || N <= 0) return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: E = %lld, N = %lld", what, (long long)E, (long long)N);
    if (E > MBNB_MOEMLP_MAX_EXPERTS)
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: E = %lld experts, at most %d", what, (long long)E, MBNB_MOEMLP_MAX_EXPERTS);
    if (T < 0 || A < 0) return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: T = %lld, A = %lld", what, (long long)T, (long long)A);
    if (T > 0 && A > MBNB_MOEMLP_MAX_PAIRS / T)
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: T x A = %lld x %lld pairs, at most %d in one call", what, (long long)T, (long long)A, MBNB_MOEMLP_MAX_PAIRS);
    const int64_t P = T * A;
    if (N > mbnb::kMaxElems / K || E > mbnb::kMaxElems / (N * K) || (P > 0 && N > mbnb::kMaxElems / P))
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: E x N x K = %lld x %lld x %lld or %lld x N outputs exceed one launch", what, (long long)E,
                    (long long)N, (long long)K, (long long)P);
    if (P > 0 && (N + 15) / 16 > INT32_MAX / (E < P ? E : P))
        return fail(MBNB_MOEMLP_ERR_SHAPE, "%s: %lld x %lld workgroups exceed one launch", what, (long long)((N + 15) / 16), (long long)(E < P ? E : P));
    return 0;
}

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
    if (const int st = check_common(what, T, A, K, x_dtype, E, N, bias_dtype, bias != nullptr, out_dtype)) return st;
    if (!(alpha - alpha == 0.0f)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: alpha = %g is not finite", what, (double)alpha);
    if (!(limit > 0.0f)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: limit = %g is not positive (+Inf: no clamp)", what, (double)limit);
    const int64_t P = T * A;
    if (P == 0) return 0;
    if (!x || !w_codes || !w_scales || !ids || !out) return fail(MBNB_MOEMLP_ERR_ARG, "%s: NULL x, w_codes, w_scales, ids or out", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w_codes, 16)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned x or w_codes (16 bytes each)", what);
    if (!mbnb::aligned(ids, 4)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned ids (4 bytes)", what);
    if (!mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned out or bias (the element size each)", what);
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
    if (const int st = check_common(what, T, A, K, h_dtype, E, N, bias_dtype, bias != nullptr, out_dtype)) return st;
    if (!known_dtype(rw_dtype)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: unknown dtype (rw %d)", what, rw_dtype);
    const int64_t P = T * A;
    if (P == 0) return 0;
    if (!h || !w_codes || !w_scales || !ids || !rw || !out) return fail(MBNB_MOEMLP_ERR_ARG, "%s: NULL h, w_codes, w_scales, ids, rw or out", what);
    if (!workspace || workspace_bytes < ws_bytes(P, N))
        return fail(MBNB_MOEMLP_ERR_WORKSPACE, "%s: the workspace is NULL or holds %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)ws_bytes(P, N));
    if (!mbnb::aligned(h, 16) || !mbnb::aligned(w_codes, 16) || !mbnb::aligned(workspace, 16))
        return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned h, w_codes or workspace (16 bytes each)", what);
    if (!mbnb::aligned(ids, 4)) return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned ids (4 bytes)", what);
    if (!mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))) ||
        !mbnb::aligned(rw, mbnb::esize(rw_dtype)))
        return fail(MBNB_MOEMLP_ERR_ARG, "%s: misaligned out, bias or rw (the element size each)", what);
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
