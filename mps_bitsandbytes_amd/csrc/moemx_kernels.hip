// moemx_kernels.hip — the grouped GEMM over MXFP4 experts on the block-scaled MFMA, activations in MXFP8 / MXFP4, and the C ABI
// of libmbnb_moemx.so (include/mbnb_moemx.h).
//
//   k_mx_experts_scaled   a workgroup serves one entry of mbnb_moegemm_plan's tile table (up to 64 listed pairs of one expert)
//                         against 256 weight rows: four waves, each all 64 pairs x 64 columns as 4 x 4 accumulators of 16 x 16,
//                         one v_mfma_scale_f32_16x16x128_f8f6f4 per accumulator and K-step of 128 over the codes and scale bytes
//                         of both operands as they lie in memory.  The activation rows of the tile are a gather (row
//                         sorted[first + r]), fetched like the weight tile by 16-byte LDS-DMA with per-lane addresses into two
//                         stages, K-step t + 1 landing under the MFMAs of step t; the scale bytes go to registers one K-step
//                         ahead and meet their edge rule where they are consumed.  ONE accumulator per output walks K in ascending
//                         order: the bits are k_gemm_mx's for the pair's row against its expert (mbnb_mx_linear), whatever else
//                         is in the call.
#include "../../include/mbnb_moemx.h"
#include "host.h"
#include "mx_decode.h"
#include "mx_plan.h"
#include "mx_scaled.h"

static_assert(MBNB_MOEMX_F16 == mbnb::kF16 && MBNB_MOEMX_BF16 == mbnb::kBF16 && MBNB_MOEMX_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOEMX_ERR_ARG == mbnb::mx::kErrArg && MBNB_MOEMX_ERR_SHAPE == mbnb::mx::kErrShape, "mx_decode.h's statuses");
static_assert(MBNB_MOEMX_ERR_WORKSPACE == mbnb::mx::kErrPlan, "mx_plan.h's status");
static_assert(MBNB_MOEMX_ROW_TILE == mbnb::mx::kPlanRowTile && MBNB_MOEMX_MAX_PAIRS == mbnb::mx::kPlanMaxPairs &&
                  MBNB_MOEMX_MAX_EXPERTS == mbnb::mx::kPlanMaxExperts,
              "mx_plan.h's tile and limits");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;
using mbnb::mx::v4f;
using mbnb::mx::v4i;
using mbnb::mx::kNaNScale;
using mbnb::mx::kOneScale;
using mbnb::mx::load_bias;
using mbnb::mx::check_expert_nulls;
using mbnb::mx::check_expert_alignment;
// the plan's layout and size, and the shape checks of a grouped call: mx_plan.h, shared with moegemm_kernels.hip
using mbnb::mx::max_tiles_of;
using mbnb::mx::plan_of;
using mbnb::mx::PlanTile;
using mbnb::mx::check_grouped_call;
using mbnb::mx::check_plan;
// the stage, the LDS-DMA, the fold of a NaN mask, the scaled MFMA and the epilogue value: mx_scaled.h, shared with k_gemm_mx
using mbnb::mx::v8i;
using mbnb::mx::ScaledStage;
using mbnb::mx::dma16;
using mbnb::mx::fold16;
using mbnb::mx::scaled_mfma;
using mbnb::mx::scaled_value;

constexpr int kRowTile = MBNB_MOEMX_ROW_TILE;            // R of the plan: listed pairs of a workgroup
constexpr int kColTile = MBNB_MOEMX_COL_TILE;            // weight rows of a workgroup
constexpr int KS = MBNB_MOEMX_K_STEP;
constexpr int kThreads = mbnb::mx::kScaledThreads, kWaves = kThreads / 64;
constexpr int kStages = 2;                               // LDS stages: K-steps t and t + 1
static_assert(kRowTile == 64 && kColTile == 64 * kWaves && KS == mbnb::mx::kScaledKStep,
              "the wave grid and the chunk maps below are written for 64 x 256 x 128");
static_assert((int64_t)MBNB_MOEMX_MAX_PAIRS * 4 < INT32_MAX, "a pair index and a list offset are an int");

// s_waitcnt vmcnt(n) alone, the other counters left at their maxima (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
constexpr int vmcnt_only(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

// Workgroup (tile, column tile); the operand map of the instruction and the LDS image of a stage are mx_scaled.h's.  Thread tid
// fetches chunk i * 256 + tid of an image: pair / column (tid >> 2) (+ 64 i for the weight), g = tid & 3, so a wave's DMA writes
// 64 consecutive chunks and reads 16 rows x 64 bytes.  Every load is unconditional, from a clamped (valid) address: a pair past
// the tile's count reads the tile's first pair, a column past N weight row N - 1, a k past K the row's first bytes; all three
// become zeros in registers with the scale 2^0, and nothing past an edge is stored.
template <int AELEM, typename TOUT>
__global__ __launch_bounds__(kThreads) void k_mx_experts_scaled(const uint8_t *__restrict__ X, const uint8_t *__restrict__ Xs,
                                                                const uint8_t *__restrict__ W, const uint8_t *__restrict__ Ws,
                                                                const int32_t *__restrict__ plan, int P, int x_div, int E, int64_t N, int64_t K,
                                                                const void *__restrict__ bias, int bias_dtype, TOUT *__restrict__ out,
                                                                int col_tiles, int max_tiles) {
    constexpr bool A8 = AELEM == MBNB_MOEMX_FP8;
    using S = ScaledStage<A8, kRowTile, kColTile>;
    constexpr int A_BYTES = S::A_BYTES, STAGE = S::STAGE, NA = S::NA, NB = S::NB;
    static_assert(NA == S::AH && NB == 4, "the chunk maps below");
    __shared__ __attribute__((aligned(16))) uint8_t smem[kStages * STAGE];
    __shared__ int pairs[kRowTile];

    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x / col_tiles;
    const int64_t n0 = (int64_t)(blockIdx.x % col_tiles) * kColTile;
    const auto pl = plan_of(plan, E, max_tiles);
    const int32_t *sorted = pl.sorted;
    const int n_tiles = *pl.n_tiles, n_listed = *pl.n_listed;

    {   // the rows of +0.0 of the out-of-range pairs, this column tile's outputs: a grid-stride loop over the tile index
        const int64_t col = n0 + tid;
        for (int i = n_listed + tile; i < P; i += max_tiles)
            if (col < N) out[(int64_t)sorted[i] * N + col] = (TOUT)0.0f;
    }
    if (tile >= n_tiles) return;                             // uniform: no weight byte is touched, no barrier was met
    const PlanTile entry = pl.tile(tile);
    const int e = entry.e, first = entry.first, rows = entry.rows;
    if (tid < kRowTile) pairs[tid] = sorted[first + (tid < rows ? tid : 0)];
    __syncthreads();

    const int64_t KB = K / 32, lda = A8 ? K : K / 2, ldw = K / 2;
    const int nk = (int)((K + KS - 1) / KS);
    const int crow = tid >> 2, cg = tid & 3;                 // this thread's chunks: pair / column crow (+ 64 i), k group cg
    const uint8_t *a_src, *b_src[NB];
    {
        const int pair = pairs[crow];
        a_src = X + (int64_t)(x_div == 1 ? pair : pair / x_div) * lda;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int64_t n = n0 + 64 * i + crow;
            b_src[i] = W + ((int64_t)e * N + (n < N ? n : N - 1)) * ldw;
        }
    }
    auto stage = [&](int s, int64_t k0) {
        uint8_t *base = smem + s * STAGE + wave * 64 * 16;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int64_t k = k0 + (A8 ? 64 * i + 16 * cg : 32 * cg);
            dma16(a_src + (k < K ? (A8 ? k : k >> 1) : 0), base + i * kThreads * 16);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int64_t k = k0 + 32 * cg;
            dma16(b_src[i] + (k < K ? k >> 1 : 0), base + A_BYTES + i * kThreads * 16);
        }
    };

    // this lane's scale bytes of a K-step: pairs 16 i + fr of the tile, columns n0 + 64 wave + 16 j + fr, k block g
    const uint8_t *as_row[4], *ws_row[4];
    bool a_live[4], b_live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pair = pairs[16 * i + fr];
        const int64_t n = n0 + 64 * wave + 16 * i + fr;
        a_live[i] = 16 * i + fr < rows;
        b_live[i] = n < N;
        as_row[i] = Xs + (int64_t)(x_div == 1 ? pair : pair / x_div) * KB;
        ws_row[i] = Ws + ((int64_t)e * N + (b_live[i] ? n : N - 1)) * KB;
    }
    // the raw bytes of K-step t, from a clamped k block; use_scales makes the dead ones 2^0 where they are consumed, so that the
    // loads have a whole K-step to land
    auto load_scales = [&](int t, int ra[4], int rb[4]) {
        const int64_t kb = (int64_t)t * (KS / 32) + g, at = kb < KB ? kb : KB - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = (int)as_row[i][at];
            rb[i] = (int)ws_row[i][at];
        }
    };
    auto use_scales = [&](int t, const int ra[4], const int rb[4], int sa[4], int sb[4]) {
        const bool in = (int64_t)t * (KS / 32) + g < KB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sa[i] = in && a_live[i] ? ra[i] : kOneScale;
            sb[i] = in && b_live[i] ? rb[i] : kOneScale;
        }
    };

    v4f acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t a_nan[4] = {0, 0, 0, 0}, b_nan[4] = {0, 0, 0, 0};
    int sa[4], sb[4], sa_next[4], sb_next[4];
    const bool ragged = rows < kRowTile || n0 + kColTile > N;    // uniform: some fragment of this tile holds a dead row or column

    // K-step t lives in stage t & 1.  Step t: every request of this wave has landed (the explicit wait: DMA(t) and the scale
    // bytes of step t); the barrier says that every wave's part of stage t is in LDS and that every wave is past its fragment
    // reads of step t - 1; the fragments of step t are read; then the scale bytes and the tiles of step t + 1 are requested, into
    // the stage step t - 1 used, and land under the 16 MFMAs of step t.
    stage(0, 0);
    load_scales(0, sa_next, sb_next);
    for (int t = 0; t < nk; ++t) {
        __builtin_amdgcn_s_waitcnt(vmcnt_only(0));
        __syncthreads();
        const uint8_t *sA = smem + (t & 1) * STAGE, *sB = sA + A_BYTES;
        v8i af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 16 * i + fr;
            const v4i lo = *(const v4i *)(sA + (row * 4 + g) * 16);
            v4i hi = v4i{0, 0, 0, 0};
            if constexpr (A8) hi = *(const v4i *)(sA + (kRowTile * 4 + row * 4 + g) * 16);
            af[i] = v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const v4i lo = *(const v4i *)(sB + ((64 * wave + 16 * j + fr) * 4 + g) * 16);
            bf[j] = v8i{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
        }
        use_scales(t, sa_next, sb_next, sa, sb);
        if (t + 1 < nk) {
            load_scales(t + 1, sa_next, sb_next);
            stage((t + 1) & 1, (int64_t)(t + 1) * KS);
        }
        const bool k_tail = t == nk - 1 && K % KS;
        if (ragged || k_tail) {                              // uniform: the dead rows, columns and k count as zeros, in both operands
            const int64_t k0 = (int64_t)t * KS;
            const bool lo_out = k0 + (A8 ? 16 : 32) * g >= K, hi_out = k0 + 64 + 16 * g >= K, b_out = k0 + 32 * g >= K;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (lo_out || !a_live[i]) af[i][q] = 0;
                    if (hi_out || !a_live[i]) af[i][4 + q] = 0;
                    if (b_out || !b_live[i]) bf[i][q] = 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a_nan[i] |= fold16(__ballot(sa[i] == kNaNScale));
            b_nan[i] |= fold16(__ballot(sb[i] == kNaNScale));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = scaled_mfma<S::CBSZ, S::BLGP>(af[i], bf[j], acc[i][j], sa[i], sb[j]);
    }

    // epilogue: + bias in f32, NaN rows and columns, one rounding, guarded stores to the rows of the listed pairs
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = n0 + 64 * wave + 16 * j + fr;
        if (col >= N) continue;
        const float b = bias ? load_bias(bias, bias_dtype, (int64_t)e * N + col) : 0.0f;
        const bool col_nan = (b_nan[j] >> fr) & 1u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * g + r;
                if (row >= rows) continue;
                out[(int64_t)pairs[row] * N + col] = (TOUT)scaled_value(acc[i][j][r], b, col_nan, a_nan[i], 4 * g + r);
            }
    }
}

// ---------------------------------------------------------------- host side
template <int AELEM>
int launch_scaled(const void *X, const void *Xs, const void *W, const void *Ws, const void *plan, int64_t P, int64_t x_div, int64_t E, int64_t N,
                  int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, hipStream_t s) {
    const int64_t col_tiles = (N + kColTile - 1) / kColTile, max_tiles = max_tiles_of(P, E);
    return mbnb::with_dtype(out_dtype, [&](auto tag) {
        using TOUT = decltype(tag);
        hipLaunchKernelGGL((k_mx_experts_scaled<AELEM, TOUT>), dim3((unsigned)(col_tiles * max_tiles)), dim3(kThreads), 0, s, (const uint8_t *)X,
                           (const uint8_t *)Xs, (const uint8_t *)W, (const uint8_t *)Ws, (const int32_t *)plan, (int)P, (int)x_div, (int)E, N, K, bias,
                           bias_dtype, (TOUT *)out, (int)col_tiles, (int)max_tiles);
        return mbnb::launch_status("k_mx_experts_scaled");
    });
}

}  // namespace

extern "C" {

int mbnb_moemx_abi_version(void) { return MBNB_MOEMX_ABI_VERSION; }

const char *mbnb_moemx_last_error(void) { return mbnb::last_error(); }

const char *mbnb_moemx_last_launch(void) { return mbnb::last_launch(); }

int mbnb_moemx_experts(const void *x_codes, const void *x_scales, int act_elem, int64_t T, int64_t A, int x_per_slot, int64_t K, const void *w_codes,
                       const void *w_scales, int64_t E, int64_t N, const int32_t *ids, const void *bias, int bias_dtype, void *out, int out_dtype,
                       const void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moemx_experts";
    if (act_elem != MBNB_MOEMX_FP4 && act_elem != MBNB_MOEMX_FP8) return fail(MBNB_MOEMX_ERR_ARG, "%s: unknown act_elem %d", what, act_elem);
    // mx_plan.h's shape checks; the rows are codes here, asked as 16-bit
    if (const int st = check_grouped_call(what, T, A, K, MBNB_MOEMX_BF16, E, N, bias_dtype, bias != nullptr, out_dtype, kColTile)) return st;
    const int64_t P = T * A;
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"x_codes", x_codes, 16}, {"x_scales", x_scales, 1}, {"w_codes", w_codes, 16},
                                                               {"w_scales", w_scales, 1}, {"ids", ids, 4}, {"out", out, mbnb::esize(out_dtype)},
                                                               {"bias", bias, mbnb::esize(bias_dtype), true}, {"plan", plan, 16}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (const int st = check_plan(what, plan, plan_bytes, P, E, "holds")) return st;     // a NULL plan was refused among the pointers
    if (const int st = check_expert_alignment(what, operands)) return st;
    const int64_t x_div = x_per_slot ? 1 : A;
    hipStream_t s = (hipStream_t)stream;
    const int st = act_elem == MBNB_MOEMX_FP8
                       ? launch_scaled<MBNB_MOEMX_FP8>(x_codes, x_scales, w_codes, w_scales, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, s)
                       : launch_scaled<MBNB_MOEMX_FP4>(x_codes, x_scales, w_codes, w_scales, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_scaled %s %s E%lld P%lld %dx%d", act_elem == MBNB_MOEMX_FP8 ? "fp8" : "fp4",
                 x_per_slot ? "slot" : "shared", (long long)E, (long long)P, kRowTile, kColTile);
    return st;
}

}  // extern "C"
