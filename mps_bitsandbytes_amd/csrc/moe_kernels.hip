// moe_kernels.hip — the MXFP4 expert linears of a mixture-of-experts layer, and the C ABI of libmbnb_moe.so (include/mbnb_moe.h;
// DESIGN.md §28).
//
//   k_mx_experts   out[p, :] = x_row(p) . W[ids[p]]^T + bias[ids[p]] for the P = T * A (token, slot) pairs of a decode batch in ONE
//                  launch, the ids read on the device.  The grid is ceil(N / 16) weight tiles x E experts.  Workgroup (tile, e)
//                  scans the ids, lists the pairs routed to e in LDS in ascending order, returns at once when there is none, and
//                  otherwise runs k_mx_decode_mfma's loop (mx_kernels.hip) over its 16 weight rows of expert e once
//                  per 16 listed pairs: the same K walk, so a pair's bits are those of that kernel for its row, whatever else is in
//                  the call.  The workgroups of expert 0 also list the pairs whose id is outside [0, E) and store their zeros.
#include "../../include/mbnb_moe.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MOE_F16 == mbnb::kF16 && MBNB_MOE_BF16 == mbnb::kBF16 && MBNB_MOE_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOE_MAX_PAIRS <= 65536 && MBNB_MOE_MAX_PAIRS % 64 == 0, "a pair index is 2 bytes in LDS");

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

constexpr int kMaxPairs = MBNB_MOE_MAX_PAIRS;
constexpr int kRows = 16;              // listed pairs per pass of the decode loop: the rows of the MFMA's A fragment

// The id scan.  Every wave scans ALL P ids, 64 per step (a lane past P reads nothing), so every wave knows the counts without a
// barrier and the empty workgroup leaves uniformly before the first one; the list entries of step s are written by wave s % 8.
// Pairs routed to `e` fill list[0 .. count) in ascending pair order; the out-of-range pairs, which only the workgroups of expert 0
// collect, fill list[kMaxPairs - zeros .. kMaxPairs) from the top down (count + zeros <= P <= kMaxPairs: they never meet).
//
// The decode loop is k_mx_decode_mfma's, statement for statement: wave w takes the k-steps w, w + 8, ... of 4 blocks, the loads of
// two k-steps are requested before the first is used, every load is unconditional from a clamped address, one FMA by the scale per
// block in block order, and the eight partial sums are added in wave order.  Row fr of the A fragment is the row of listed pair
// c16 + fr; entries past the count are zero fragments in registers (their loads go to row 0 of x).
template <typename T>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mx_experts(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                 const uint8_t *__restrict__ Ws, const int32_t *__restrict__ ids, int P,
                                                                 int x_div, int64_t E, int64_t N, int64_t K, const void *__restrict__ bias,
                                                                 int bias_dtype, void *__restrict__ out, int out_dtype, int tiles) {
    static_assert(sizeof(T) == 2, "16-bit activations");
    constexpr int U = 2;                                     // k-steps whose loads are requested before the first of them is used
    __shared__ float red[kMfmaWaves][4][64];
    __shared__ int red_ff[kMfmaWaves][64];
    __shared__ uint16_t list[kMaxPairs];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t e = blockIdx.x / tiles;
    const int64_t n0 = (int64_t)(blockIdx.x % tiles) * 16;

    int count = 0, zeros = 0;
    for (int s = 0; s * 64 < P; ++s) {
        const int p = s * 64 + lane;
        const bool in = p < P;
        int id = 0;
        if (in) id = ids[p];
        const bool writer = (s % kMfmaWaves) == wave;        // wave-uniform
        const bool mine = in && (int64_t)id == e;
        const uint64_t bm = __ballot(mine);
        if (writer && mine) list[count + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u))] = (uint16_t)p;
        count += __popcll(bm);
        if (e == 0) {
            const bool oob = in && (id < 0 || (int64_t)id >= E);
            const uint64_t bz = __ballot(oob);
            if (writer && oob)
                list[kMaxPairs - 1 - zeros - (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bz >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bz, 0u))] = (uint16_t)p;
            zeros += __popcll(bz);
        }
    }
    if (count == 0 && zeros == 0) return;                    // no pair for this expert: no weight byte is touched, no barrier was met
    __syncthreads();

    // the rows of +0.0 of the out-of-range pairs, this tile's columns (expert 0 only: zeros == 0 elsewhere)
    for (int i = tid >> 4; i < zeros; i += (64 * kMfmaWaves) >> 4) {
        const int64_t col = n0 + (tid & 15);
        if (col < N) store_out(out, out_dtype, (int64_t)list[kMaxPairs - 1 - i] * N + col, 0.0f);
    }

    const int64_t KB = K / 32, ldw = K / 2, last = KB - 1;
    const int64_t n = n0 + fr < N ? n0 + fr : N - 1;         // a column past N reads the last weight row and stores nothing
    const uint8_t *w_row = W + (e * N + n) * ldw, *s_row = Ws + (e * N + n) * KB;
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
            if (n0 + fr < N) {
                const float b = bias ? load_bias(bias, bias_dtype, e * N + n) : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = c16 + 4 * g + r;
                    if (i < count) store_out(out, out_dtype, (int64_t)list[i] * N + n, col_nan ? __uint_as_float(0x7FC00000u) : s[r] + b);
                }
            }
        }
        if (c16 + kRows < count) __syncthreads();            // uniform: wave 0 is done with the sums before the next pass writes them
    }
}

// ---------------------------------------------------------------- host side
bool known_dtype(int d) { return d >= MBNB_MOE_F16 && d <= MBNB_MOE_F32; }

template <typename T>
int launch_experts(const void *x, const void *W, const void *Ws, const int32_t *ids, int64_t P, int64_t x_div, int64_t E, int64_t N,
                   int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, int64_t tiles, hipStream_t s) {
    hipLaunchKernelGGL((k_mx_experts<T>), dim3((unsigned)(tiles * E)), dim3(64 * kMfmaWaves), 0, s, (const T *)x, (const uint8_t *)W,
                       (const uint8_t *)Ws, ids, (int)P, (int)x_div, E, N, K, bias, bias_dtype, out, out_dtype, (int)tiles);
    return mbnb::launch_status("k_mx_experts");
}

}  // namespace

extern "C" {

int mbnb_moe_abi_version(void) { return MBNB_MOE_ABI_VERSION; }

const char *mbnb_moe_last_error(void) { return mbnb::last_error(); }

const char *mbnb_moe_last_launch(void) { return mbnb::last_launch(); }

int mbnb_moe_mxfp4_experts(const void *x, int64_t T, int64_t A, int x_per_slot, int64_t K, int x_dtype, const void *w_codes,
                           const void *w_scales, int64_t E, int64_t N, const int32_t *ids, const void *bias, int bias_dtype, void *out,
                           int out_dtype, void *stream) {
    const char *const what = "mbnb_moe_mxfp4_experts";
    if (!known_dtype(x_dtype) || !known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_MOE_ERR_ARG, "%s: unknown dtype (x %d, bias %d, out %d)", what, x_dtype, bias_dtype, out_dtype);
    if (!mbnb::is16(x_dtype)) return fail(MBNB_MOE_ERR_ARG, "%s: 16-bit activations only (f16 or bf16 x)", what);
    if (K <= 0 || K % 32) return fail(MBNB_MOE_ERR_SHAPE, "%s: K = %lld is not a positive multiple of the MX block, 32", what, (long long)K);
    if (E <= 0 || N <= 0) return fail(MBNB_MOE_ERR_SHAPE, "%s: E = %lld, N = %lld", what, (long long)E, (long long)N);
    if (T < 0 || A < 0) return fail(MBNB_MOE_ERR_SHAPE, "%s: T = %lld, A = %lld", what, (long long)T, (long long)A);
    if (T > 0 && A > MBNB_MOE_MAX_PAIRS / T)
        return fail(MBNB_MOE_ERR_SHAPE, "%s: T x A = %lld x %lld pairs, at most %d in one launch", what, (long long)T, (long long)A, MBNB_MOE_MAX_PAIRS);
    const int64_t P = T * A;
    if (N > mbnb::kMaxElems / K || E > mbnb::kMaxElems / (N * K) || (P > 0 && N > mbnb::kMaxElems / P))
        return fail(MBNB_MOE_ERR_SHAPE, "%s: E x N x K = %lld x %lld x %lld or %lld x N outputs exceed one launch", what, (long long)E,
                    (long long)N, (long long)K, (long long)P);
    if (P == 0) return 0;
    const int64_t tiles = (N + 15) / 16;
    if (tiles > INT32_MAX / E)
        return fail(MBNB_MOE_ERR_SHAPE, "%s: %lld x %lld workgroups exceed one launch", what, (long long)tiles, (long long)E);
    if (!x || !w_codes || !w_scales || !ids || !out) return fail(MBNB_MOE_ERR_ARG, "%s: NULL x, w_codes, w_scales, ids or out", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w_codes, 16)) return fail(MBNB_MOE_ERR_ARG, "%s: misaligned x or w_codes (16 bytes each)", what);
    if (!mbnb::aligned(ids, 4)) return fail(MBNB_MOE_ERR_ARG, "%s: misaligned ids (4 bytes)", what);
    if (!mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_MOE_ERR_ARG, "%s: misaligned out or bias (the element size each)", what);
    hipStream_t s = (hipStream_t)stream;
    const int64_t x_div = x_per_slot ? 1 : A;
    const int st = x_dtype == MBNB_MOE_BF16
                       ? launch_experts<bf16_t>(x, w_codes, w_scales, ids, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, tiles, s)
                       : launch_experts<f16_t>(x, w_codes, w_scales, ids, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, tiles, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_experts %s %s E%lld P%lld", x_dtype == MBNB_MOE_BF16 ? "bf16" : "f16",
                 x_per_slot ? "slot" : "shared", (long long)E, (long long)P);
    return st;
}

}  // extern "C"
