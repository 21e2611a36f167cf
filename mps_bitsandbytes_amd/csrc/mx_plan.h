// mx_plan.h — the plan of a grouped expert call, once: moegemm_kernels.hip builds it (k_plan_count, k_plan_fill)
// and reads it (k_mx_experts_grouped), moemx_kernels.hip reads it (k_mx_experts_scaled).  Two libraries agree on a binary format
// through this header: the word layout, its size, the accessor every kernel goes through, and the shape checks of a grouped call.
#pragma once

#include "mx_decode.h"

namespace mbnb {
namespace mx {

// R, the listed pairs of one tile entry, and the limits of a grouped call: MBNB_MOEGEMM_* == MBNB_MOEMX_*, each library asserts its own
constexpr int kPlanRowTile = 64;
constexpr int kPlanMaxPairs = 1048576;
constexpr int kPlanMaxExperts = 1024;
constexpr int kErrPlan = -3;           // a short plan is a short workspace: the ERR_WORKSPACE of both libraries

// int32 words: counts[E], n_tiles, n_listed, tiles[max_tiles][3], sorted[P]
__host__ __device__ inline int64_t max_tiles_of(int64_t P, int64_t E) { return (E < P ? E : P) + P / kPlanRowTile; }
static inline int64_t plan_words(int64_t P, int64_t E) { return E + 2 + 3 * max_tiles_of(P, E) + P; }
static inline int64_t plan_bytes_of(int64_t P, int64_t E) { return round256(plan_words(P, E) * 4); }

struct PlanTile { int e, first, rows; };                     // one entry of the tile table: rows <= R listed pairs of expert e from sorted[first]

// The parts of a plan of E experts and max_tiles entries; WORD is int32_t where the plan is written, const int32_t where it is
// read (counts[e] is plan[e] itself).  Entry t of the tile table is the words tiles[3 t .. 3 t + 2], in PlanTile's order.
template <typename WORD> struct Plan {
    WORD *n_tiles, *n_listed, *tiles, *sorted;
    __device__ __forceinline__ PlanTile tile(int t) const { return PlanTile{tiles[3 * t], tiles[3 * t + 1], tiles[3 * t + 2]}; }
};
template <typename WORD> __device__ __forceinline__ Plan<WORD> plan_of(WORD *plan, int E, int max_tiles) {
    WORD *tiles = plan + E + 2;
    return Plan<WORD>{plan + E, plan + E + 1, tiles, tiles + 3 * (int64_t)max_tiles};
}

// ---------------------------------------------------------------- host: the checks of a grouped call
// The shape checks of a projection over T x A pairs: mx_decode.h's for everything but the pairs (asked with none, its limit being
// the decode launches'), then the pairs of a plan, the outputs, and the grid of ceil(N / col_tile) x max_tiles workgroups.
static inline int check_grouped_call(const char *what, int64_t T, int64_t A, int64_t K, int row_dtype, int64_t E, int64_t N, int bias_dtype,
                                     bool has_bias, int out_dtype, int col_tile) {
    if (const int st = check_expert_call(what, 0, 0, K, row_dtype, E, N, bias_dtype, has_bias, out_dtype, kPlanMaxExperts, true)) return st;
    if (T < 0 || A < 0) return fail(kErrShape, "%s: T = %lld, A = %lld", what, (long long)T, (long long)A);
    if (T > 0 && A > kPlanMaxPairs / T)
        return fail(kErrShape, "%s: T x A = %lld x %lld pairs, at most %d in one launch", what, (long long)T, (long long)A, kPlanMaxPairs);
    const int64_t P = T * A;
    if (P > 0 && N > kMaxElems / P) return fail(kErrShape, "%s: %lld x %lld outputs exceed one launch", what, (long long)P, (long long)N);
    const int64_t col_tiles = (N + col_tile - 1) / col_tile;   // under the limits above the grid stays below 2^31: the guard of the launch's cast
    if (P > 0 && col_tiles > INT32_MAX / max_tiles_of(P, E))
        return fail(kErrShape, "%s: %lld x %lld workgroups exceed one launch", what, (long long)col_tiles, (long long)max_tiles_of(P, E));
    return 0;
}

// The plan of a call with P > 0 pairs holds its bytes.  `holds`: the caller's words for what it refuses ("holds", or "is NULL or
// holds" where a NULL plan is refused here and not among the pointers).
static inline int check_plan(const char *what, const void *plan, int64_t plan_bytes, int64_t P, int64_t E, const char *holds) {
    if (!plan || plan_bytes < plan_bytes_of(P, E))
        return fail(kErrPlan, "%s: the plan %s %lld bytes, %lld needed", what, holds, (long long)plan_bytes, (long long)plan_bytes_of(P, E));
    return 0;
}

}  // namespace mx
}  // namespace mbnb
