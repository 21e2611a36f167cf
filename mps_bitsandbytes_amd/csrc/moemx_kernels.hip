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
//                         is in the call.  The store is one of two epilogues: Plain (the projection in out_dtype; as f32 into a
//                         workspace it is the first launch of down + sum), or GluQ: the gated activation of the
//                         interleaved gate / up rows in f32 and the MX quantiser over the wave's 32 activated values of a pair
//                         row, which are exactly one block of the down projection's input; the codes and scale bytes leave
//                         through LDS as 16-byte stores, so the intermediate never exists in 16 or 32 bits in memory.
//   k_scaled_slot_sum     the routed sum over a token's slots of that workspace: a thread per four consecutive outputs.
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
using mbnb::mx::enc_e2m1;
using mbnb::mx::enc_e4m3;

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

constexpr int kPlainEpi = -1;                            // HELEM of the Plain epilogue; GluQ: the element format of its output

// The gated activation of the GluQ epilogue.  The operation chain is mbnb_moegemm.h's (the same clamps, the same
// seven roundings in the same order; tests/test_gpu_moemx_mlp.py holds it bit for bit at alpha = 0 and within the chain's derived
// bound elsewhere): every operation a separate f32 rounding (-ffp-contract=off), the division IEEE, expf OCML's.
__device__ __forceinline__ float gated(float gate, float up, float alpha, float limit) {
    gate = gate > limit ? limit : gate;
    up = up > limit ? limit : (up < -limit ? -limit : up);
    const float ag = alpha * gate;
    const float den = 1.0f + expf(-ag);
    const float sig = 1.0f / den;
    const float gs = gate * sig;
    const float u1 = up + 1.0f;
    return u1 * gs;
}

// Workgroup (tile, column tile); the operand map of the instruction and the LDS image of a stage are mx_scaled.h's.  Thread tid
// fetches chunk i * 256 + tid of an image: pair / column (tid >> 2) (+ 64 i for the weight), g = tid & 3, so a wave's DMA writes
// 64 consecutive chunks and reads 16 rows x 64 bytes.  Every load is unconditional, from a clamped (valid) address: a pair past
// the tile's count reads the tile's first pair, a column past N weight row N - 1, a k past K the row's first bytes; all three
// become zeros in registers with the scale 2^0, and nothing past an edge is stored.
//
// GluQ<HELEM> (N = 2 I, I % 32 == 0, weight row 2 j gate j, 2 j + 1 up j): out is h_codes [P, I] (fp8) or [P, I / 2] (fp4) and
// h_scales [P, I / 32].  A wave's 64 weight rows are 32 activated columns, one MX block, so a block is wholly inside N or wholly
// outside and a wave is live or dead as a whole.  Lanes fr, fr ^ 1 hold (gate, up) of activated column 8 j + fr / 2 of the block
// for the rows 4 g + r; the even lane takes r = 0, 1 and the odd lane r = 2, 3, so each exchanges two values per accumulator and
// evaluates half of the activations.  The block's amax: the 4 j in registers, then the 8 lanes of the same parity in the 16-lane
// group.  The codes are strided in the destination row, so the workgroup's tile (64 pairs x 128 or 64 bytes, then 64 x 4 scale
// bytes) is put together in the stage memory, free after one barrier, and leaves as 16-byte stores.
template <int AELEM, typename TOUT, int HELEM>
__global__ __launch_bounds__(kThreads) void k_mx_experts_scaled(const uint8_t *__restrict__ X, const uint8_t *__restrict__ Xs,
                                                                const uint8_t *__restrict__ W, const uint8_t *__restrict__ Ws,
                                                                const int32_t *__restrict__ plan, int P, int x_div, int E, int64_t N, int64_t K,
                                                                const void *__restrict__ bias, int bias_dtype, TOUT *__restrict__ out,
                                                                int col_tiles, int max_tiles, uint8_t *__restrict__ h_scales, float alpha,
                                                                float limit) {
    constexpr bool A8 = AELEM == MBNB_MOEMX_FP8, H8 = HELEM == MBNB_MOEMX_FP8;
    constexpr int H_ROW = H8 ? 128 : 64, H_CHUNKS = H_ROW / 16, H_COLS = H8 ? 16 : 32;   // GluQ: a pair row of the tile in bytes, in 16-byte chunks, and the activated columns of a chunk
    static_assert(HELEM == kPlainEpi || sizeof(TOUT) == 1, "GluQ stores bytes");
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

    // GluQ's output geometry: I activated columns, ldh code bytes and hb scale bytes per pair, this column tile from byte h0 and block b0
    const int64_t I = N / 2, ldh = H8 ? I : I / 2, hb = I / 32, h0 = H8 ? n0 / 2 : n0 / 4, b0 = n0 / 64;
    if constexpr (HELEM == kPlainEpi) {   // the rows of +0.0 of the out-of-range pairs, this column tile's outputs: a grid-stride loop over the tile index
        const int64_t col = n0 + tid;
        for (int i = n_listed + tile; i < P; i += max_tiles)
            if (col < N) out[(int64_t)sorted[i] * N + col] = (TOUT)0.0f;
    } else {                              // what the quantiser gives a row of +0.0: codes 0 and byte 0, over the same loop
        for (int i = n_listed + tile; i < P; i += max_tiles) {
            const int64_t p = sorted[i];
            if (tid < H_CHUNKS && n0 / 2 + H_COLS * tid < I) *(uint4 *)(out + p * ldh + h0 + 16 * tid) = make_uint4(0u, 0u, 0u, 0u);
            if (tid >= 64 && tid < 68 && b0 + (tid - 64) < hb) h_scales[p * hb + b0 + (tid - 64)] = 0;
        }
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

    // epilogue: + bias in f32, NaN rows and columns; Plain: one rounding, guarded stores to the rows of the listed pairs; GluQ: the
    // value stays in its accumulator register (a dead pair row too: it is finite or NaN like any other, and is not stored)
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
                if (HELEM == kPlainEpi && row >= rows) continue;
                const float pre = scaled_value(acc[i][j][r], b, col_nan, a_nan[i], 4 * g + r);
                if constexpr (HELEM == kPlainEpi) out[(int64_t)pairs[row] * N + col] = (TOUT)pre;
                else acc[i][j][r] = pre;
            }
    }
    if constexpr (HELEM != kPlainEpi) {
        uint8_t *const tile_c = smem, *const tile_s = smem + kRowTile * H_ROW;
        static_assert(kRowTile * (H_ROW + 4) <= kStages * STAGE, "the code tile and its scale bytes fit the stage memory");
        __syncthreads();                                     // every wave is past its fragment reads of the last K-step, and no DMA is in flight
        if (n0 + 64 * wave < N) {                            // uniform: this wave's block is inside I
            const int odd = fr & 1;
            constexpr uint32_t emax = H8 ? 8u : 2u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    float h[4];
                    uint32_t amax = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {            // mine: this lane's column at the row it takes; sent: at the row its partner takes
                        const float mine = odd ? acc[i][j][2 + rr] : acc[i][j][rr], sent = odd ? acc[i][j][rr] : acc[i][j][2 + rr];
                        const float got = __shfl_xor(sent, 1);
                        h[j] = gated(odd ? got : mine, odd ? mine : got, alpha, limit);
                        amax = max(amax, __float_as_uint(h[j]) & 0x7FFFFFFFu);
                    }
                    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
                    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 4));
                    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 8));
                    // mbnb_mx.h's rule, as k_mx_quantize states it: E = 255 is an Inf or a NaN in the block
                    const uint32_t E8 = amax >> 23, byte = E8 == 255u ? (uint32_t)kNaNScale : (E8 > emax ? E8 - emax : 0u);
                    const float mult = __uint_as_float((254u - byte) << 23);
                    uint32_t c4 = 0;                         // the codes of j = 0 .. 3, a byte each
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t u = __float_as_uint(h[j] * mult), a = u & 0x7FFFFFFFu;
                        const uint32_t c = H8 ? enc_e4m3(a) | ((u >> 24) & 0x80u) : enc_e2m1(__uint_as_float(a)) | ((u >> 28) & 8u);
                        c4 |= (E8 == 255u ? 0u : c) << (8 * j);
                    }
                    const int row = 16 * i + 4 * g + 2 * odd + rr;
                    if constexpr (H8) {                      // activated column 8 j + fr / 2 of the wave's block
#pragma unroll
                        for (int j = 0; j < 4; ++j) tile_c[row * H_ROW + 32 * wave + 8 * j + (fr >> 1)] = (uint8_t)(c4 >> (8 * j));
                    } else {                                 // the even column of a byte in its low nibble: the lane two up holds the odd one
                        const uint32_t up4 = (uint32_t)__shfl_xor((int)c4, 2);
                        if (!(fr & 2)) {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                tile_c[row * H_ROW + 16 * wave + 4 * j + (fr >> 2)] = (uint8_t)(((c4 >> (8 * j)) & 15u) | (((up4 >> (8 * j)) & 15u) << 4));
                        }
                    }
                    if (fr < 2) tile_s[row * 4 + wave] = (uint8_t)byte;
                }
        }
        __syncthreads();
        for (int c = tid; c < kRowTile * H_CHUNKS; c += kThreads) {
            const int row = c / H_CHUNKS, q = c % H_CHUNKS;
            if (row < rows && n0 / 2 + H_COLS * q < I)
                *(uint4 *)(out + (int64_t)pairs[row] * ldh + h0 + 16 * q) = *(const uint4 *)(tile_c + row * H_ROW + 16 * q);
        }
        const int srow = tid >> 2, sq = tid & 3;             // the 4 scale bytes of a row: its blocks in this column tile
        if (srow < rows && b0 + sq < hb) h_scales[(int64_t)pairs[srow] * hb + b0 + sq] = tile_s[srow * 4 + sq];
    }
}

// The routed sum of down + sum over the f32 workspace y [T * A, N]: one thread per four consecutive outputs of a token, the slots in
// their order from +0.0, one fmaf each, one rounding.  A slot whose id is outside [0, E) is skipped, its routing weight and its
// workspace row unread.  Rows of y are 16-byte aligned when N % 4 == 0 (float4 loads); otherwise every load is scalar.
constexpr int kSlotSumThreads = 256;
template <typename TOUT>
__global__ __launch_bounds__(kSlotSumThreads) void k_scaled_slot_sum(const float *__restrict__ y, const int32_t *__restrict__ ids,
                                                                     const void *__restrict__ rw, int rw_dtype, int64_t T, int A, int E,
                                                                     int64_t N, TOUT *__restrict__ out) {
    const int64_t quads = (N + 3) / 4, i = (int64_t)blockIdx.x * kSlotSumThreads + threadIdx.x;
    if (i >= T * quads) return;
    const int64_t t = i / quads, n = (i - t * quads) * 4;
    const int live = N - n < 4 ? (int)(N - n) : 4;
    const bool vec = N % 4 == 0;                             // uniform
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int a = 0; a < A; ++a) {
        const int64_t p = t * A + a;
        const int id = ids[p];
        if (id < 0 || id >= E) continue;
        const float w = load_bias(rw, rw_dtype, p);
        const float *row = y + p * N + n;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec) {
            const float4 q = *(const float4 *)row;
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < live) v[c] = row[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(w, v[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < live) out[t * N + n + c] = (TOUT)acc[c];
}

// ---------------------------------------------------------------- host side
// One launch of k_mx_experts_scaled.  HELEM == kPlainEpi: out [P, N] of out_dtype.  Else GluQ: out is h_codes, out_dtype unread.
template <int AELEM, int HELEM>
int launch_scaled(const void *X, const void *Xs, const void *W, const void *Ws, const void *plan, int64_t P, int64_t x_div, int64_t E, int64_t N,
                  int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, void *h_scales, float alpha, float limit, hipStream_t s) {
    const int64_t col_tiles = (N + kColTile - 1) / kColTile, max_tiles = max_tiles_of(P, E);
    const auto launch = [&](auto tag) {
        using TOUT = decltype(tag);
        hipLaunchKernelGGL((k_mx_experts_scaled<AELEM, TOUT, HELEM>), dim3((unsigned)(col_tiles * max_tiles)), dim3(kThreads), 0, s, (const uint8_t *)X,
                           (const uint8_t *)Xs, (const uint8_t *)W, (const uint8_t *)Ws, (const int32_t *)plan, (int)P, (int)x_div, (int)E, N, K, bias,
                           bias_dtype, (TOUT *)out, (int)col_tiles, (int)max_tiles, (uint8_t *)h_scales, alpha, limit);
        return mbnb::launch_status("k_mx_experts_scaled");
    };
    if constexpr (HELEM == kPlainEpi) return mbnb::with_dtype(out_dtype, launch);
    else return launch(uint8_t{});
}

int launch_plain(int act_elem, const void *X, const void *Xs, const void *W, const void *Ws, const void *plan, int64_t P, int64_t x_div, int64_t E,
                 int64_t N, int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, hipStream_t s) {
    return act_elem == MBNB_MOEMX_FP8
               ? launch_scaled<MBNB_MOEMX_FP8, kPlainEpi>(X, Xs, W, Ws, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, nullptr, 0.0f, 0.0f, s)
               : launch_scaled<MBNB_MOEMX_FP4, kPlainEpi>(X, Xs, W, Ws, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, nullptr, 0.0f, 0.0f, s);
}

int launch_slot_sum(const void *y, const int32_t *ids, const void *rw, int rw_dtype, int64_t T, int64_t A, int64_t E, int64_t N, void *out,
                    int out_dtype, hipStream_t s) {
    const int64_t threads = T * ((N + 3) / 4);
    return mbnb::with_dtype(out_dtype, [&](auto tag) {
        using TOUT = decltype(tag);
        hipLaunchKernelGGL((k_scaled_slot_sum<TOUT>), dim3((unsigned)((threads + kSlotSumThreads - 1) / kSlotSumThreads)), dim3(kSlotSumThreads), 0, s,
                           (const float *)y, ids, rw, rw_dtype, T, (int)A, (int)E, N, (TOUT *)out);
        return mbnb::launch_status("k_scaled_slot_sum");
    });
}

const char *elem_name(int elem) { return elem == MBNB_MOEMX_FP8 ? "fp8" : "fp4"; }
bool known_elem(int elem) { return elem == MBNB_MOEMX_FP4 || elem == MBNB_MOEMX_FP8; }
int64_t slot_workspace_bytes(int64_t P, int64_t N) { return (P * N * 4 + 255) & ~(int64_t)255; }     // f32 [P, N], in whole 256 bytes

// The checks of the three entry points, in one order (mbnb_moemx_experts'): the formats, mx_plan.h's shape checks (the rows are
// codes here, asked as 16-bit), the entry point's own refusals that need no pointer (`own`: a status or 0), the empty call
// (*work = false), the pointers, the plan (a NULL plan was refused among the pointers), the workspace of down + sum
// (workspace_bytes < 0: the call has none), the alignments.
template <typename OWN>
int check_call(const char *what, int act_elem, int64_t T, int64_t A, int64_t K, int64_t E, int64_t N, int bias_dtype, bool has_bias, int out_dtype,
               OWN &&own, std::initializer_list<mbnb::mx::Operand> operands, const void *plan, int64_t plan_bytes, const void *workspace,
               int64_t workspace_bytes, bool *work) {
    *work = false;
    if (!known_elem(act_elem)) return fail(MBNB_MOEMX_ERR_ARG, "%s: unknown act_elem %d", what, act_elem);
    if (const int st = check_grouped_call(what, T, A, K, MBNB_MOEMX_BF16, E, N, bias_dtype, has_bias, out_dtype, kColTile)) return st;
    if (const int st = own()) return st;
    const int64_t P = T * A;
    if (P == 0) return 0;
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (const int st = check_plan(what, plan, plan_bytes, P, E, "holds")) return st;
    if (workspace_bytes >= 0 && (!workspace || workspace_bytes < slot_workspace_bytes(P, N)))
        return fail(MBNB_MOEMX_ERR_WORKSPACE, "%s: the f32 workspace is missing or short: %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)slot_workspace_bytes(P, N));
    if (const int st = check_expert_alignment(what, operands)) return st;
    *work = true;
    return 0;
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
    bool work;
    if (const int st = check_call(what, act_elem, T, A, K, E, N, bias_dtype, bias != nullptr, out_dtype, [] { return 0; },
                                  {{"x_codes", x_codes, 16}, {"x_scales", x_scales, 1}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1},
                                   {"ids", ids, 4}, {"out", out, mbnb::esize(out_dtype)}, {"bias", bias, mbnb::esize(bias_dtype), true}, {"plan", plan, 16}},
                                  plan, plan_bytes, nullptr, -1, &work))
        return st;
    if (!work) return 0;
    const int64_t P = T * A;
    const int st = launch_plain(act_elem, x_codes, x_scales, w_codes, w_scales, plan, P, x_per_slot ? 1 : A, E, N, K, bias, bias_dtype, out, out_dtype,
                                (hipStream_t)stream);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_scaled %s %s E%lld P%lld %dx%d", elem_name(act_elem),
                 x_per_slot ? "slot" : "shared", (long long)E, (long long)P, kRowTile, kColTile);
    return st;
}

int mbnb_moemx_gate_up_glu(const void *x_codes, const void *x_scales, int act_elem, int64_t T, int64_t A, int64_t K, const void *w_codes,
                           const void *w_scales, int64_t E, int64_t I, const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit,
                           void *h_codes, void *h_scales, int h_elem, const void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moemx_gate_up_glu";
    const int64_t N = 2 * (I < mbnb::kMaxElems ? I : mbnb::kMaxElems);       // an I beyond every limit is refused as its N, without overflow
    const auto own = [&] {
        if (!known_elem(h_elem)) return fail(MBNB_MOEMX_ERR_ARG, "%s: unknown h_elem %d", what, h_elem);
        if (h_elem != act_elem)
            return fail(MBNB_MOEMX_ERR_ARG, "%s: act_elem %s with h_elem %s: the two formats of a call are the same", what, elem_name(act_elem), elem_name(h_elem));
        if (I % 32) return fail(MBNB_MOEMX_ERR_SHAPE, "%s: I = %lld is not a multiple of the MX block, 32: an activated row is quantised in whole blocks", what, (long long)I);
        if (!(alpha - alpha == 0.0f)) return fail(MBNB_MOEMX_ERR_ARG, "%s: alpha (%g) must be finite", what, (double)alpha);
        if (!(limit > 0.0f)) return fail(MBNB_MOEMX_ERR_ARG, "%s: limit (%g) must be above 0 (+Inf: no clamp)", what, (double)limit);
        return 0;
    };
    bool work;
    if (const int st = check_call(what, act_elem, T, A, K, E, N, bias_dtype, bias != nullptr, MBNB_MOEMX_F32, own,
                                  {{"x_codes", x_codes, 16}, {"x_scales", x_scales, 1}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1},
                                   {"ids", ids, 4}, {"h_codes", h_codes, 16}, {"h_scales", h_scales, 1}, {"bias", bias, mbnb::esize(bias_dtype), true},
                                   {"plan", plan, 16}},
                                  plan, plan_bytes, nullptr, -1, &work))
        return st;
    if (!work) return 0;
    const int64_t P = T * A;
    hipStream_t s = (hipStream_t)stream;
    const int st = h_elem == MBNB_MOEMX_FP8 ? launch_scaled<MBNB_MOEMX_FP8, MBNB_MOEMX_FP8>(x_codes, x_scales, w_codes, w_scales, plan, P, A, E, N, K, bias,
                                                                                            bias_dtype, h_codes, 0, h_scales, alpha, limit, s)
                                            : launch_scaled<MBNB_MOEMX_FP4, MBNB_MOEMX_FP4>(x_codes, x_scales, w_codes, w_scales, plan, P, A, E, N, K, bias,
                                                                                            bias_dtype, h_codes, 0, h_scales, alpha, limit, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_scaled_glu %s>%s E%lld P%lld %dx%d", elem_name(act_elem), elem_name(h_elem),
                 (long long)E, (long long)P, kRowTile, kColTile);
    return st;
}

int64_t mbnb_moemx_workspace_bytes(int64_t P, int64_t N) {
    const char *const what = "mbnb_moemx_workspace_bytes";
    if (P < 0 || N <= 0) return fail(MBNB_MOEMX_ERR_SHAPE, "%s: P = %lld, N = %lld", what, (long long)P, (long long)N);
    if (P > MBNB_MOEMX_MAX_PAIRS) return fail(MBNB_MOEMX_ERR_SHAPE, "%s: P = %lld pairs, at most %d in one call", what, (long long)P, MBNB_MOEMX_MAX_PAIRS);
    if (P > 0 && N > mbnb::kMaxElems / P) return fail(MBNB_MOEMX_ERR_SHAPE, "%s: %lld x %lld outputs exceed one launch", what, (long long)P, (long long)N);
    return slot_workspace_bytes(P, N);
}

int mbnb_moemx_down_sum(const void *h_codes, const void *h_scales, int act_elem, int64_t T, int64_t A, int64_t K, const void *w_codes,
                        const void *w_scales, int64_t E, int64_t N, const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype,
                        void *out, int out_dtype, void *workspace, int64_t workspace_bytes, const void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moemx_down_sum";
    const auto own = [&] {
        if (rw_dtype < MBNB_MOEMX_F16 || rw_dtype > MBNB_MOEMX_F32) return fail(MBNB_MOEMX_ERR_ARG, "%s: unknown dtype (rw %d)", what, rw_dtype);
        return 0;
    };
    bool work;
    if (const int st = check_call(what, act_elem, T, A, K, E, N, bias_dtype, bias != nullptr, out_dtype, own,
                                  {{"h_codes", h_codes, 16}, {"h_scales", h_scales, 1}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1},
                                   {"ids", ids, 4}, {"rw", rw, mbnb::esize(rw_dtype)}, {"out", out, mbnb::esize(out_dtype)},
                                   {"bias", bias, mbnb::esize(bias_dtype), true}, {"workspace", workspace, 16, true}, {"plan", plan, 16}},
                                  plan, plan_bytes, workspace, workspace_bytes < 0 ? 0 : workspace_bytes, &work))
        return st;
    if (!work) return 0;
    const int64_t P = T * A;
    hipStream_t s = (hipStream_t)stream;
    int st = launch_plain(act_elem, h_codes, h_scales, w_codes, w_scales, plan, P, 1, E, N, K, bias, bias_dtype, workspace, MBNB_MOEMX_F32, s);
    if (st != 0) return st;
    st = launch_slot_sum(workspace, ids, rw, rw_dtype, T, A, E, N, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_scaled_down_sum %s E%lld P%lld %dx%d A%lld", elem_name(act_elem), (long long)E,
                 (long long)P, kRowTile, kColTile, (long long)A);
    return st;
}

}  // extern "C"
