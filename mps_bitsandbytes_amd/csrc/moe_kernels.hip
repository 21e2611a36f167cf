// moe_kernels.hip — the MXFP4 expert linears of a mixture-of-experts layer, and the C ABI of libmbnb_moe.so (include/mbnb_moe.h;
// DESIGN.md §28).
//
//   k_mx_experts   out[p, :] = x_row(p) . W[ids[p]]^T + bias[ids[p]] for the P = T * A (token, slot) pairs of a decode batch in ONE
//                  launch, the ids read on the device.  The grid is ceil(N / 16) weight tiles x E experts.  Workgroup (tile, e)
//                  scans the ids, lists the pairs routed to e in LDS in ascending order (list_pairs), returns at once when there
//                  is none, and otherwise runs the decode tile of mx_decode.h (tile_walk, tile_reduce: the functions
//                  k_mx_decode_mfma calls) over its 16 weight rows of expert e once per 16 listed pairs, so a
//                  pair's bits are those of that kernel for its row, whatever else is in the call.  The workgroups of expert 0
//                  also list the pairs whose id is outside [0, E) and store their zeros.
#include "../../include/mbnb_moe.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MOE_F16 == mbnb::kF16 && MBNB_MOE_BF16 == mbnb::kBF16 && MBNB_MOE_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOE_MAX_PAIRS == mbnb::mx::kMaxPairs, "mx_decode.h's pair list");
static_assert(MBNB_MOE_ERR_ARG == mbnb::mx::kErrArg && MBNB_MOE_ERR_SHAPE == mbnb::mx::kErrShape, "mx_decode.h's statuses");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
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

// What is this kernel's own: the expert is the grid row, the loop over passes of 16 listed pairs, and the stores.  Row fr of the
// A fragment is the row of listed pair c16 + fr; entries past the count are zero fragments in registers (their loads go to row 0
// of x).
template <typename T>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mx_experts(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                 const uint8_t *__restrict__ Ws, const int32_t *__restrict__ ids, int P,
                                                                 int x_div, int64_t E, int64_t N, int64_t K, const void *__restrict__ bias,
                                                                 int bias_dtype, void *__restrict__ out, int out_dtype, int tiles) {
    __shared__ TileLds lds;
    __shared__ uint16_t list[kMaxPairs];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.x / tiles;
    const int64_t n0 = (int64_t)(blockIdx.x % tiles) * 16;

    const PairCounts pairs = list_pairs(ids, P, e, (int)E, e == 0, wave, lane, list);   // E fits: the host refuses tiles * E > INT32_MAX
    const int count = pairs.count, zeros = pairs.zeros;
    if (count == 0 && zeros == 0) return;                    // no pair for this expert: no weight byte is touched, no barrier was met
    __syncthreads();

    // the rows of +0.0 of the out-of-range pairs, this tile's columns (expert 0 only: zeros == 0 elsewhere)
    for (int i = tid >> 4; i < zeros; i += (64 * kMfmaWaves) >> 4) {
        const int64_t col = n0 + (tid & 15);
        if (col < N) store_out(out, out_dtype, (int64_t)list[kMaxPairs - 1 - i] * N + col, 0.0f);
    }

    const int64_t KB = K / 32, ldw = K / 2;
    const int64_t n = n0 + fr < N ? n0 + fr : N - 1;         // a column past N reads the last weight row and stores nothing
    const uint8_t *w_row = W + ((int64_t)e * N + n) * ldw, *s_row = Ws + ((int64_t)e * N + n) * KB;

    for (int c16 = 0; c16 < count; c16 += kPairRows) {
        const bool x_live = c16 + fr < count;
        const int pair = x_live ? (int)list[c16 + fr] : 0;
        const T *x_row = x + (int64_t)(x_div == 1 ? pair : pair / x_div) * K + 8 * g;

        const TileSums part = tile_walk<T>(x_row, x_live, w_row, s_row, KB, wave, g);
        const bool stores = wave == 0 && n0 + fr < N;
        const float b = stores && bias ? load_bias(bias, bias_dtype, (int64_t)e * N + n) : 0.0f;   // requested before the reduction's barrier
        v4f s;
        const bool col_nan = tile_reduce(lds, part, wave, lane, s);
        if (stores) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = c16 + 4 * g + r;
                if (i < count) store_out(out, out_dtype, (int64_t)list[i] * N + n, col_nan ? __uint_as_float(0x7FC00000u) : s[r] + b);
            }
        }
        if (c16 + kPairRows < count) __syncthreads();        // uniform: wave 0 is done with the sums before the next pass writes them
    }
}

// ---------------------------------------------------------------- host side
template <typename T>
int launch_experts(const void *x, const void *W, const void *Ws, const int32_t *ids, int64_t P, int64_t x_div, int64_t E, int64_t N,
                   int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, hipStream_t s) {
    const int64_t tiles = (N + 15) / 16;
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
    if (const int st = mbnb::mx::check_expert_call(what, T, A, K, x_dtype, E, N, bias_dtype, bias != nullptr, out_dtype, 0, false)) return st;
    const int64_t P = T * A;
    if (P == 0) return 0;
    if (const int st = mbnb::mx::check_expert_pointers(what, {{"x", x, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                              {"out", out, mbnb::esize(out_dtype)}, {"bias", bias, mbnb::esize(bias_dtype), true}}))
        return st;
    hipStream_t s = (hipStream_t)stream;
    const int64_t x_div = x_per_slot ? 1 : A;
    const int st = x_dtype == MBNB_MOE_BF16 ? launch_experts<bf16_t>(x, w_codes, w_scales, ids, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, s)
                                            : launch_experts<f16_t>(x, w_codes, w_scales, ids, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_experts %s %s E%lld P%lld", x_dtype == MBNB_MOE_BF16 ? "bf16" : "f16",
                 x_per_slot ? "slot" : "shared", (long long)E, (long long)P);
    return st;
}

}  // extern "C"
