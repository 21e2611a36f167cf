// moegemm_kernels.hip — the prefill-sized grouped GEMM over MXFP4 experts, and the C ABI of libmbnb_moegemm.so
// (include/mbnb_moegemm.h).
//
//   k_plan_count, k_plan_fill   the plan of a call, a function of the ids alone: counts[E], the stable list of pair indices
//                               grouped by expert (the out-of-range pairs last) and the tile table, (expert, first, rows <= R)
//                               per entry.  Workgroup e counts / lists its own expert with ballots; no workgroup waits for
//                               another, the second launch reads what the first wrote.
//   k_mx_experts_grouped        a workgroup serves one tile-table entry (up to R = 16 MT listed pairs of one expert) against
//                               C = 16 NT weight rows and ALL of K: the K walk of mx_decode.h's tile_walk with MT A fragments
//                               per block and NT B fragments per k-step in registers, every decoded B fragment reused by MT
//                               MFMAs.  A result's bits are those of k_mx_experts for its row: the same blocks in the same
//                               order on the same wave, one FMA by the scale per block, the eight partial sums added from
//                               +0.0 in wave order.  Three epilogues: Plain (bias, one rounding, zeros for the out-of-range
//                               pairs), Glu (moemlp_kernels.hip's gated activation) and PlainF32 (into the workspace).
//   k_routed_sum                moemlp_kernels.hip's: the fmaf chain over the slots of a token, in slot order.
#include "../../include/mbnb_moegemm.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MOEGEMM_F16 == mbnb::kF16 && MBNB_MOEGEMM_BF16 == mbnb::kBF16 && MBNB_MOEGEMM_F32 == mbnb::kF32, "host.h's dtype codes");
static_assert(MBNB_MOEGEMM_ERR_ARG == mbnb::mx::kErrArg && MBNB_MOEGEMM_ERR_SHAPE == mbnb::mx::kErrShape, "mx_decode.h's statuses");
static_assert(MBNB_MOEGEMM_ROW_TILE % 16 == 0 && MBNB_MOEGEMM_ROW_TILE % 32 == 0, "whole A fragments, and 8 waves share the 4 R / 16 sums of a round");
static_assert(MBNB_MOEGEMM_MAX_PAIRS >= 65536 && (int64_t)MBNB_MOEGEMM_MAX_PAIRS * 4 < INT32_MAX, "a pair index and a list offset are an int");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;
using mbnb::mx::v4f;
using mbnb::mx::v4i;
using mbnb::mx::kMfmaWaves;
using mbnb::mx::kNaNScale;
using mbnb::mx::kOneScale;
using mbnb::mx::decode8_16;
using mbnb::mx::mfma16;
using mbnb::mx::scale_value;
using mbnb::mx::load_bias;
using mbnb::mx::store_out;
using mbnb::mx::lane_rank;
using mbnb::mx::check_expert_call;
using mbnb::mx::check_expert_nulls;
using mbnb::mx::check_expert_alignment;

constexpr int kMaxExperts = MBNB_MOEGEMM_MAX_EXPERTS;
constexpr int kMaxGroupedPairs = MBNB_MOEGEMM_MAX_PAIRS;
constexpr int kRowTile = MBNB_MOEGEMM_ROW_TILE;          // R: listed pairs of a workgroup
constexpr int kMT = kRowTile / 16;                       // A fragments per block
constexpr int kNT = 3;                                   // B fragments per k-step: C = 16 NT weight rows of a workgroup
constexpr int kColTile = 16 * kNT;
constexpr int kThreads = 64 * kMfmaWaves;
constexpr int kPlanThreads = 256, kPlanWaves = kPlanThreads / 64;
constexpr int kPlanUnroll = 4;                           // id chunks of 256 whose loads are requested before the first ballot
constexpr int kSumThreads = 256;

struct Plain { static constexpr bool kGlu = false, kZeros = true; };
struct Glu { static constexpr bool kGlu = true, kZeros = true; };
struct PlainF32 { static constexpr bool kGlu = false, kZeros = false; };

// ---------------------------------------------------------------- the plan
// int32 words: counts[E], n_tiles, n_listed, tiles[max_tiles][3], sorted[P]
__host__ __device__ inline int64_t max_tiles_of(int64_t P, int64_t E) { return (E < P ? E : P) + P / kRowTile; }
int64_t plan_words(int64_t P, int64_t E) { return E + 2 + 3 * max_tiles_of(P, E) + P; }

// workgroup e: counts[e]
__global__ __launch_bounds__(kPlanThreads) void k_plan_count(const int32_t *__restrict__ ids, int P, int32_t *__restrict__ plan) {
    __shared__ int part[kPlanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = blockIdx.x;
    int count = 0;
    for (int p0 = 0; p0 < P; p0 += kPlanThreads) {
        const int p = p0 + tid;
        bool mine = false;
        if (p < P) mine = ids[p] == e;
        count += __popcll(__ballot(mine));
    }
    if (lane == 0) part[wave] = count;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < kPlanWaves; ++w) total += part[w];
        plan[e] = total;
    }
}

// workgroup b < E: the tile entries and the stable list of expert b; workgroup E: the out-of-range list, n_tiles and n_listed.
// Both start at the sums over counts[0 .. b), and scan the ids 1024 per step in index order.
__global__ __launch_bounds__(kPlanThreads) void k_plan_fill(const int32_t *__restrict__ ids, int P, int E, int32_t *__restrict__ plan,
                                                            int max_tiles) {
    __shared__ int sums[2][kPlanWaves];
    __shared__ int cnt[2][kPlanUnroll * kPlanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    int off = 0, toff = 0;
    for (int j = tid; j < b; j += kPlanThreads) {
        const int c = plan[j];
        off += c;
        toff += (c + kRowTile - 1) / kRowTile;
    }
    for (int m = 32; m; m >>= 1) {
        off += __shfl_xor(off, m);
        toff += __shfl_xor(toff, m);
    }
    if (lane == 0) {
        sums[0][wave] = off;
        sums[1][wave] = toff;
    }
    __syncthreads();
    off = toff = 0;
    for (int w = 0; w < kPlanWaves; ++w) {
        off += sums[0][w];
        toff += sums[1][w];
    }
    int32_t *tiles = plan + E + 2, *sorted = tiles + 3 * (int64_t)max_tiles;
    if (b == E) {
        if (tid == 0) {
            plan[E] = toff;
            plan[E + 1] = off;
        }
    } else {
        const int count = plan[b];
        for (int t = tid; t * kRowTile < count; t += kPlanThreads) {
            const int left = count - t * kRowTile;
            tiles[3 * (toff + t)] = b;
            tiles[3 * (toff + t) + 1] = off + t * kRowTile;
            tiles[3 * (toff + t) + 2] = left < kRowTile ? left : kRowTile;
        }
    }
    int base = off;
    for (int p0 = 0, it = 0; p0 < P; p0 += kPlanUnroll * kPlanThreads, ++it) {
        int id[kPlanUnroll];
        bool in[kPlanUnroll];
#pragma unroll
        for (int u = 0; u < kPlanUnroll; ++u) {
            const int p = p0 + u * kPlanThreads + tid;
            in[u] = p < P;
            id[u] = 0;
            if (in[u]) id[u] = ids[p];
        }
        uint64_t bm[kPlanUnroll];
        bool mine[kPlanUnroll];
#pragma unroll
        for (int u = 0; u < kPlanUnroll; ++u) {
            mine[u] = in[u] && (b < E ? id[u] == b : (id[u] < 0 || id[u] >= E));
            bm[u] = __ballot(mine[u]);
            if (lane == 0) cnt[it & 1][u * kPlanWaves + wave] = __popcll(bm[u]);
        }
        __syncthreads();                                     // the buffer written two steps on is read before the barrier of the next
        int before = 0;
#pragma unroll
        for (int u = 0; u < kPlanUnroll; ++u) {
#pragma unroll
            for (int w = 0; w < kPlanWaves; ++w) {
                if (w == wave && mine[u]) sorted[base + before + lane_rank(bm[u])] = p0 + u * kPlanThreads + tid;
                before += cnt[it & 1][u * kPlanWaves + w];
            }
        }
        base += before;
    }
}

// ---------------------------------------------------------------- the grouped GEMM
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

struct GroupedLds {                    // one round of the reduction: the 4 MT sums of one B fragment, of every wave
    float red[kMfmaWaves][4 * kMT][64];
    int red_ff[kMfmaWaves][64];
};

// Workgroup (tile, column tile).  Lane (fr = l & 15, g = l >> 4) of every wave holds, per A fragment m, listed pair 16 m + fr of
// the tile (its row advanced by 8 g elements) and, per B fragment j, weight row n0 + 16 j + fr.  Wave w takes the k-steps w,
// w + 8, ... of four blocks: per k-step the lane fetches the 16 bytes of block 4 c + g of each of its NT weight rows, the
// 4 x 4 transpose across the lane groups leaves dword g of block q in register q, and the decoded fragment of block q meets
// the MT A fragments of that block.  Every load is unconditional, from a clamped (valid) address; rows past the tile's count,
// columns past N and k past K become zeros in registers, and nothing past an edge is stored.
template <typename T, typename EPI>
__global__ __launch_bounds__(kThreads) void k_mx_experts_grouped(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                 const uint8_t *__restrict__ Ws, const int32_t *__restrict__ plan, int P,
                                                                 int x_div, int E, int64_t N, int64_t K, const void *__restrict__ bias,
                                                                 int bias_dtype, void *__restrict__ out, int out_dtype, int col_tiles,
                                                                 int max_tiles, float alpha, float limit) {
    static_assert(sizeof(T) == 2, "16-bit activations");
    __shared__ GroupedLds lds;
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x / col_tiles;
    const int64_t n0 = (int64_t)(blockIdx.x % col_tiles) * kColTile;
    const int32_t *tiles = plan + E + 2, *sorted = tiles + 3 * (int64_t)max_tiles;
    const int n_tiles = plan[E], n_listed = plan[E + 1];
    const int64_t width = EPI::kGlu ? N / 2 : N;            // of a row of out

    if (EPI::kZeros) {                                      // the rows of +0.0 of the out-of-range pairs, this column tile's outputs
        constexpr int kCols = EPI::kGlu ? kColTile / 2 : kColTile, kRows = kThreads / kCols;     // kRows rows per pass; the threads left over rest
        const int64_t col = (EPI::kGlu ? n0 / 2 : n0) + tid % kCols;
        for (int i = n_listed + tile * kRows + tid / kCols; i < P && tid < kRows * kCols; i += max_tiles * kRows)
            if (col < width) store_out(out, out_dtype, (int64_t)sorted[i] * width + col, 0.0f);
    }
    if (tile >= n_tiles) return;                            // uniform: no weight byte is touched, no barrier was met
    const int e = tiles[3 * tile], first = tiles[3 * tile + 1], rows = tiles[3 * tile + 2];

    const int64_t KB = K / 32, ldw = K / 2, last = KB - 1, steps = (KB + 3) / 4;
    const uint8_t *w_row[kNT], *s_row[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) {                          // a column past N reads the last weight row and stores nothing
        const int64_t n = n0 + 16 * j + fr < N ? n0 + 16 * j + fr : N - 1;
        w_row[j] = W + ((int64_t)e * N + n) * ldw;
        s_row[j] = Ws + ((int64_t)e * N + n) * KB;
    }
    const T *x_row[kMT];
    bool x_live[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) {                          // an entry past the count reads row 0 of x and is a zero fragment
        x_live[m] = 16 * m + fr < rows;
        const int pair = x_live[m] ? sorted[first + 16 * m + fr] : 0;
        x_row[m] = x + (int64_t)(x_div == 1 ? pair : pair / x_div) * K + 8 * g;
    }

    v4f acc[kMT][kNT];
    bool ff[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
        ff[j] = false;
#pragma unroll
        for (int m = 0; m < kMT; ++m) acc[m][j] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
    for (int64_t c = wave; c < steps; c += kMfmaWaves) {
        v4i wq[kNT], xa[4][kMT];
        uint32_t sb[kNT];                                    // the scale bytes of blocks 4 c .. 4 c + 3, block q in byte q
        const int64_t blk = 4 * c + g;
#pragma unroll
        for (int j = 0; j < kNT; ++j) {
            wq[j] = *(const v4i *)(w_row[j] + (blk < KB ? blk : last) * 16);
            if (blk >= KB) wq[j] = v4i{0, 0, 0, 0};
            sb[j] = 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = 4 * c + q < KB;
            const int64_t b = in ? 4 * c + q : last;
#pragma unroll
            for (int j = 0; j < kNT; ++j) {
                uint32_t byte = s_row[j][b];
                if (!in) byte = (uint32_t)kOneScale;
                sb[j] |= byte << (8 * q);
            }
#pragma unroll
            for (int m = 0; m < kMT; ++m) {
                xa[q][m] = *(const v4i *)(x_row[m] + b * 32);
                if (!(in && x_live[m])) xa[q][m] = v4i{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int j = 0; j < kNT; ++j) {
            // register q of lane group g holds dword q of block g; after the transpose, dword g of block q
            typedef unsigned v2u __attribute__((ext_vector_type(2)));
            const v2u s02 = __builtin_amdgcn_permlane32_swap((unsigned)wq[j][0], (unsigned)wq[j][2], false, false);
            const v2u s13 = __builtin_amdgcn_permlane32_swap((unsigned)wq[j][1], (unsigned)wq[j][3], false, false);
            const v2u t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
            const v2u t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
            const uint32_t wb[4] = {t01[0], t01[1], t23[0], t23[1]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4i bq = decode8_16<T>(wb[q]);
                const uint32_t byte = (sb[j] >> (8 * q)) & 0xFFu;
                ff[j] |= byte == (uint32_t)kNaNScale;
                const float sv = scale_value(byte == (uint32_t)kNaNScale ? (uint32_t)kOneScale : byte);
#pragma unroll
                for (int m = 0; m < kMT; ++m) {
                    const v4f d = mfma16(xa[q][m], bq, T{});
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[m][j][r] = __builtin_fmaf(d[r], sv, acc[m][j][r]);
                }
                __builtin_amdgcn_sched_barrier(0);           // the MT results of one block are consumed before the next block's are made
            }
        }
    }

    // The reduction, one round per B fragment: sum v = 4 m + r of the round is added by wave v % 8, from +0.0 in wave order;
    // there lane (fr, g) holds column n0 + 16 j + fr of listed pair 16 m + 4 g + r.
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
        const int64_t col = n0 + 16 * j + fr, n = col < N ? col : N - 1;
        const float b = bias ? load_bias(bias, bias_dtype, (int64_t)e * N + n) : 0.0f;   // requested before the round's barrier
        if (j) __syncthreads();                              // the sums of the round before are read
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds.red[wave][4 * m + r][lane] = acc[m][j][r];
        lds.red_ff[wave][lane] = ff[j];
        __syncthreads();
        bool col_nan = false;
#pragma unroll
        for (int w = 0; w < kMfmaWaves; ++w) col_nan |= lds.red_ff[w][lane] != 0;
#pragma unroll
        for (int v0 = 0; v0 < 4 * kMT; v0 += kMfmaWaves) {
            const int v = v0 + wave;
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < kMfmaWaves; ++w) s += lds.red[w][v][lane];
            const int i = 16 * (v >> 2) + 4 * g + (v & 3);
            const bool live = i < rows;
            const int64_t pair = sorted[first + (live ? i : 0)];
            const float pre = col_nan ? __uint_as_float(0x7FC00000u) : s + b;
            if (EPI::kGlu) {
                // N = 2I: lanes fr, fr ^ 1 hold (gate, up) of one output, both inside N or both outside; all 64 lanes exchange
                const float other = __shfl_xor(pre, 1);
                if (!(fr & 1) && col < N && live) store_out(out, out_dtype, pair * width + col / 2, glu(pre, other, alpha, limit));
            } else if (col < N && live) {
                store_out(out, out_dtype, pair * width + n, pre);
            }
        }
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
bool known_dtype(int d) { return d >= MBNB_MOEGEMM_F16 && d <= MBNB_MOEGEMM_F32; }
const char *name16(int d) { return d == MBNB_MOEGEMM_BF16 ? "bf16" : "f16"; }
int64_t ws_bytes(int64_t P, int64_t N) { return mbnb::round256(P * N * 4); }
int64_t plan_bytes_of(int64_t P, int64_t E) { return mbnb::round256(plan_words(P, E) * 4); }

// The shape checks of a projection call: mx_decode.h's for everything but the pairs (asked with none, its limit being the decode
// launches'), then the pairs of this library, the outputs and the grid.
int check_grouped_call(const char *what, int64_t T, int64_t A, int64_t K, int row_dtype, int64_t E, int64_t N, int bias_dtype, bool has_bias,
                       int out_dtype) {
    if (const int st = check_expert_call(what, 0, 0, K, row_dtype, E, N, bias_dtype, has_bias, out_dtype, kMaxExperts, true)) return st;
    if (T < 0 || A < 0) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: T = %lld, A = %lld", what, (long long)T, (long long)A);
    if (T > 0 && A > kMaxGroupedPairs / T)
        return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: T x A = %lld x %lld pairs, at most %d in one launch", what, (long long)T, (long long)A,
                    kMaxGroupedPairs);
    const int64_t P = T * A;
    if (P > 0 && N > mbnb::kMaxElems / P)
        return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: %lld x %lld outputs exceed one launch", what, (long long)P, (long long)N);
    const int64_t col_tiles = (N + kColTile - 1) / kColTile;   // under the limits above the grid stays below 2^31: the guard of the launch's cast
    if (P > 0 && col_tiles > INT32_MAX / max_tiles_of(P, E))
        return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: %lld x %lld workgroups exceed one launch", what, (long long)col_tiles,
                    (long long)max_tiles_of(P, E));
    return 0;
}

int check_plan(const char *what, const void *plan, int64_t plan_bytes, int64_t P, int64_t E) {
    if (!plan || plan_bytes < plan_bytes_of(P, E))
        return fail(MBNB_MOEGEMM_ERR_WORKSPACE, "%s: the plan is NULL or holds %lld bytes, %lld needed", what, (long long)plan_bytes,
                    (long long)plan_bytes_of(P, E));
    return 0;
}

template <typename T, typename EPI>
int launch_grouped(const void *x, const void *W, const void *Ws, const void *plan, int64_t P, int64_t x_div, int64_t E, int64_t N, int64_t K,
                   const void *bias, int bias_dtype, void *out, int out_dtype, float alpha, float limit, hipStream_t s) {
    const int64_t col_tiles = (N + kColTile - 1) / kColTile, max_tiles = max_tiles_of(P, E);
    hipLaunchKernelGGL((k_mx_experts_grouped<T, EPI>), dim3((unsigned)(col_tiles * max_tiles)), dim3(kThreads), 0, s, (const T *)x,
                       (const uint8_t *)W, (const uint8_t *)Ws, (const int32_t *)plan, (int)P, (int)x_div, (int)E, N, K, bias, bias_dtype, out,
                       out_dtype, (int)col_tiles, (int)max_tiles, alpha, limit);
    return mbnb::launch_status("k_mx_experts_grouped");
}

template <typename EPI>
int launch_by_dtype(int x_dtype, const void *x, const void *W, const void *Ws, const void *plan, int64_t P, int64_t x_div, int64_t E, int64_t N,
                    int64_t K, const void *bias, int bias_dtype, void *out, int out_dtype, float alpha, float limit, hipStream_t s) {
    return x_dtype == MBNB_MOEGEMM_BF16 ? launch_grouped<bf16_t, EPI>(x, W, Ws, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, alpha, limit, s)
                                        : launch_grouped<f16_t, EPI>(x, W, Ws, plan, P, x_div, E, N, K, bias, bias_dtype, out, out_dtype, alpha, limit, s);
}

}  // namespace

extern "C" {

int mbnb_moegemm_abi_version(void) { return MBNB_MOEGEMM_ABI_VERSION; }

const char *mbnb_moegemm_last_error(void) { return mbnb::last_error(); }

const char *mbnb_moegemm_last_launch(void) { return mbnb::last_launch(); }

int64_t mbnb_moegemm_plan_bytes(int64_t P, int64_t E) {
    const char *const what = "mbnb_moegemm_plan_bytes";
    if (P < 0 || P > kMaxGroupedPairs) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: P = %lld pairs, at most %d", what, (long long)P, kMaxGroupedPairs);
    if (E <= 0 || E > kMaxExperts) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: E = %lld experts, at most %d", what, (long long)E, kMaxExperts);
    return plan_bytes_of(P, E);
}

int mbnb_moegemm_plan(const int32_t *ids, int64_t P, int64_t E, void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moegemm_plan";
    if (P < 0 || P > kMaxGroupedPairs) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: P = %lld pairs, at most %d", what, (long long)P, kMaxGroupedPairs);
    if (E <= 0 || E > kMaxExperts) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: E = %lld experts, at most %d", what, (long long)E, kMaxExperts);
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"ids", ids, 4}, {"plan", plan, 16, true}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (const int st = check_plan(what, plan, plan_bytes, P, E)) return st;
    if (const int st = check_expert_alignment(what, operands)) return st;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_plan_count, dim3((unsigned)E), dim3(kPlanThreads), 0, s, ids, (int)P, (int32_t *)plan);
    int st = mbnb::launch_status("k_plan_count");
    if (st != 0) return st;
    hipLaunchKernelGGL(k_plan_fill, dim3((unsigned)E + 1), dim3(kPlanThreads), 0, s, ids, (int)P, (int)E, (int32_t *)plan, (int)max_tiles_of(P, E));
    st = mbnb::launch_status("k_plan_fill");
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_plan E%lld P%lld R%d", (long long)E, (long long)P, kRowTile);
    return st;
}

int mbnb_moegemm_experts(const void *x, int64_t T, int64_t A, int x_per_slot, int64_t K, int x_dtype, const void *w_codes, const void *w_scales,
                         int64_t E, int64_t N, const int32_t *ids, const void *bias, int bias_dtype, void *out, int out_dtype, const void *plan,
                         int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moegemm_experts";
    if (const int st = check_grouped_call(what, T, A, K, x_dtype, E, N, bias_dtype, bias != nullptr, out_dtype)) return st;
    const int64_t P = T * A;
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"x", x, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                               {"out", out, mbnb::esize(out_dtype)}, {"bias", bias, mbnb::esize(bias_dtype), true},
                                                               {"plan", plan, 16, true}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (const int st = check_plan(what, plan, plan_bytes, P, E)) return st;
    if (const int st = check_expert_alignment(what, operands)) return st;
    const int st = launch_by_dtype<Plain>(x_dtype, x, w_codes, w_scales, plan, P, x_per_slot ? 1 : A, E, N, K, bias, bias_dtype, out, out_dtype, 0.0f,
                                          0.0f, (hipStream_t)stream);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped %s %s E%lld P%lld R%d", name16(x_dtype), x_per_slot ? "slot" : "shared",
                 (long long)E, (long long)P, kRowTile);
    return st;
}

int mbnb_moegemm_gate_up_glu(const void *x, int64_t T, int64_t A, int64_t K, int x_dtype, const void *w_codes, const void *w_scales, int64_t E,
                             int64_t I, const int32_t *ids, const void *bias, int bias_dtype, float alpha, float limit, void *out, int out_dtype,
                             const void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moegemm_gate_up_glu";
    if (I <= 0 || I > mbnb::kMaxElems / 2) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: I = %lld", what, (long long)I);
    const int64_t N = 2 * I;
    if (const int st = check_grouped_call(what, T, A, K, x_dtype, E, N, bias_dtype, bias != nullptr, out_dtype)) return st;
    if (!(alpha - alpha == 0.0f)) return fail(MBNB_MOEGEMM_ERR_ARG, "%s: alpha = %g is not finite", what, (double)alpha);
    if (!(limit > 0.0f)) return fail(MBNB_MOEGEMM_ERR_ARG, "%s: limit = %g is not positive (+Inf: no clamp)", what, (double)limit);
    const int64_t P = T * A;
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"x", x, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                               {"out", out, mbnb::esize(out_dtype)}, {"bias", bias, mbnb::esize(bias_dtype), true},
                                                               {"plan", plan, 16, true}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (const int st = check_plan(what, plan, plan_bytes, P, E)) return st;
    if (const int st = check_expert_alignment(what, operands)) return st;
    const int st = launch_by_dtype<Glu>(x_dtype, x, w_codes, w_scales, plan, P, A, E, N, K, bias, bias_dtype, out, out_dtype, alpha, limit,
                                        (hipStream_t)stream);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_glu %s E%lld P%lld R%d", name16(x_dtype), (long long)E, (long long)P, kRowTile);
    return st;
}

int64_t mbnb_moegemm_workspace_bytes(int64_t P, int64_t N) {
    const char *const what = "mbnb_moegemm_workspace_bytes";
    if (P < 0 || N <= 0) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: P = %lld, N = %lld", what, (long long)P, (long long)N);
    if (P > kMaxGroupedPairs) return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: P = %lld pairs, at most %d in one call", what, (long long)P, kMaxGroupedPairs);
    if (P > 0 && N > mbnb::kMaxElems / P)
        return fail(MBNB_MOEGEMM_ERR_SHAPE, "%s: %lld x %lld outputs exceed one launch", what, (long long)P, (long long)N);
    return ws_bytes(P, N);
}

int mbnb_moegemm_down_sum(const void *h, int64_t T, int64_t A, int64_t K, int h_dtype, const void *w_codes, const void *w_scales, int64_t E,
                          int64_t N, const int32_t *ids, const void *bias, int bias_dtype, const void *rw, int rw_dtype, void *out, int out_dtype,
                          void *workspace, int64_t workspace_bytes, const void *plan, int64_t plan_bytes, void *stream) {
    const char *const what = "mbnb_moegemm_down_sum";
    if (const int st = check_grouped_call(what, T, A, K, h_dtype, E, N, bias_dtype, bias != nullptr, out_dtype)) return st;
    if (!known_dtype(rw_dtype)) return fail(MBNB_MOEGEMM_ERR_ARG, "%s: unknown dtype (rw %d)", what, rw_dtype);
    const int64_t P = T * A;
    if (P == 0) return 0;
    const std::initializer_list<mbnb::mx::Operand> operands = {{"h", h, 16}, {"w_codes", w_codes, 16}, {"w_scales", w_scales, 1}, {"ids", ids, 4},
                                                               {"rw", rw, mbnb::esize(rw_dtype)}, {"out", out, mbnb::esize(out_dtype)},
                                                               {"bias", bias, mbnb::esize(bias_dtype), true}, {"workspace", workspace, 16, true},
                                                               {"plan", plan, 16, true}};
    if (const int st = check_expert_nulls(what, operands)) return st;
    if (!workspace || workspace_bytes < ws_bytes(P, N))
        return fail(MBNB_MOEGEMM_ERR_WORKSPACE, "%s: the workspace is NULL or holds %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)ws_bytes(P, N));
    if (const int st = check_plan(what, plan, plan_bytes, P, E)) return st;
    if (const int st = check_expert_alignment(what, operands)) return st;
    hipStream_t s = (hipStream_t)stream;
    int st = launch_by_dtype<PlainF32>(h_dtype, h, w_codes, w_scales, plan, P, 1, E, N, K, bias, bias_dtype, workspace, MBNB_MOEGEMM_F32, 0.0f, 0.0f, s);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_routed_sum, dim3((unsigned)((T * N + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads), 0, s, (const float *)workspace,
                       ids, rw, rw_dtype, T, (int)A, (int)E, N, out, out_dtype);
    st = mbnb::launch_status("k_routed_sum");
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_grouped_down_sum %s E%lld P%lld R%d A%lld", name16(h_dtype), (long long)E,
                 (long long)P, kRowTile, (long long)A);
    return st;
}

}  // extern "C"
