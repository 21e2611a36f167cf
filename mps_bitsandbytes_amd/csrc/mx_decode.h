// mx_decode.h — what the three MXFP4 decode libraries share: mx_kernels.hip (k_mx_decode, k_mx_decode_mfma),
// moe_kernels.hip (k_mx_experts) and moemlp_kernels.hip (k_mx_experts_rt).
//
//   device   the E8M0 scale, the byte-table decode of 8 E2M1 codes to 8 values of the activation's 16-bit type, the MFMA of one MX
//            block, the bias load and output store by dtype code; and the ONE text of the 16 x 16 decode tile on
//            v_mfma_f32_16x16x32: tile_walk (a wave's share of the K walk) and tile_reduce (the eight partial sums, in wave order),
//            which fix a result's bits, and list_pairs (the id scan of the two expert kernels).  All of it forced inline.
//   host     check_expert_call / check_expert_pointers: the argument checks the three expert entry points share.
// The dtype codes are host.h's, which every public header restates.
#pragma once

#include <initializer_list>

#include "host.h"

namespace mbnb {
namespace mx {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kNaNScale = 0xFF;        // E8M0: the block is NaN
constexpr int kOneScale = 127;         // E8M0: 2^0
constexpr int kMfmaWaves = 8;          // the waves of an MFMA decode workgroup: wave w takes the k-steps w, w + 8, ...

// 2^(byte - 127) for byte 0..254; byte 0 is the f32 subnormal 2^-127
__device__ __forceinline__ float scale_value(uint32_t byte) { return __uint_as_float(byte ? byte << 23 : 0x00400000u); }

__device__ __forceinline__ float load_bias(const void *bias, int dtype, int64_t col) {
    if (dtype == kF32) return ((const float *)bias)[col];
    if (dtype == kBF16) return (float)((const bf16_t *)bias)[col];
    return (float)((const f16_t *)bias)[col];
}

__device__ __forceinline__ void store_out(void *out, int dtype, int64_t i, float v) {
    if (dtype == kF32) ((float *)out)[i] = v;
    else if (dtype == kBF16) ((bf16_t *)out)[i] = (bf16_t)v;
    else ((f16_t *)out)[i] = (f16_t)v;
}

template <typename T> struct E2M1Bytes;      // the 16-bit patterns of 0, .5, 1, 1.5, 2, 3, 4, 6 as byte tables: {codes 4..7, codes 0..3}
template <> struct E2M1Bytes<bf16_t> { static constexpr uint32_t hi[2] = {0x40404040u, 0x3F3F3F00u}, lo[2] = {0xC0804000u, 0xC0800000u}; };
template <> struct E2M1Bytes<f16_t> { static constexpr uint32_t hi[2] = {0x46444240u, 0x3E3C3800u}, lo[2] = {0u, 0u}; };

// the 8 codes of w (k = 0 .. 7, the lower k in the lower nibble) -> 8 values of T, k ascending
template <typename T> __device__ __forceinline__ v4i decode8_16(uint32_t w) {
    const uint32_t sel_e = w & 0x07070707u, sel_o = (w >> 4) & 0x07070707u;                       // k = 0, 2, 4, 6 and 1, 3, 5, 7
    const uint32_t hi_e = __builtin_amdgcn_perm(E2M1Bytes<T>::hi[0], E2M1Bytes<T>::hi[1], sel_e) | ((w << 4) & 0x80808080u);
    const uint32_t hi_o = __builtin_amdgcn_perm(E2M1Bytes<T>::hi[0], E2M1Bytes<T>::hi[1], sel_o) | (w & 0x80808080u);
    const uint32_t lo_e = __builtin_amdgcn_perm(E2M1Bytes<T>::lo[0], E2M1Bytes<T>::lo[1], sel_e);
    const uint32_t lo_o = __builtin_amdgcn_perm(E2M1Bytes<T>::lo[0], E2M1Bytes<T>::lo[1], sel_o);
    const uint32_t e01 = __builtin_amdgcn_perm(hi_e, lo_e, 0x05010400u), e23 = __builtin_amdgcn_perm(hi_e, lo_e, 0x07030602u);   // k 0, 2 | 4, 6
    const uint32_t o01 = __builtin_amdgcn_perm(hi_o, lo_o, 0x05010400u), o23 = __builtin_amdgcn_perm(hi_o, lo_o, 0x07030602u);   // k 1, 3 | 5, 7
    return v4i{(int)__builtin_amdgcn_perm(o01, e01, 0x05040100u), (int)__builtin_amdgcn_perm(o01, e01, 0x07060302u),
               (int)__builtin_amdgcn_perm(o23, e23, 0x05040100u), (int)__builtin_amdgcn_perm(o23, e23, 0x07060302u)};
}

__device__ __forceinline__ v4f mfma16(v4i a, v4i b, bf16_t) {
    typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), v4f{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
}
__device__ __forceinline__ v4f mfma16(v4i a, v4i b, f16_t) {
    typedef _Float16 v8h __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), v4f{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
}

// ---------------------------------------------------------------- the 16 x 16 decode tile of an 8-wave workgroup
// A workgroup owns 16 weight rows and ALL of K against up to 16 activation rows.  Lane (fr = l & 15, g = l >> 4) of every wave
// holds weight row fr (w_row, s_row: its codes and scale bytes) and activation row fr (x_row, already advanced by 8 g elements;
// x_live: the row exists).  What fixes a result's bits is here and nowhere else: the order of the blocks, one FMA by the scale
// per block, and the order of the eight partial sums.
struct TileSums {
    v4f acc;                           // column fr, rows 4 g + r: this wave's partial sums
    bool ff;                           // a 0xFF scale byte among this wave's blocks of weight row fr
};

struct TileLds {                       // 10 KiB: a workgroup declares one
    float red[kMfmaWaves][4][64];
    int red_ff[kMfmaWaves][64];
};

// Wave `wave` takes the k-steps wave, wave + 8, ... of 4 blocks (128 k) each; the loads of U = 2 k-steps are requested before the
// first is used.  Per k-step the lane fetches the 16 bytes of block 4 c + g of its weight row, and a 4 x 4 transpose across the
// four lane groups leaves in register q the dword g of block 4 c + q: the B fragment of the MFMA of block q.  Every load is
// unconditional, from a clamped (valid) address; what lies past K or the live rows becomes zeros in registers.
template <typename T>
__device__ __forceinline__ TileSums tile_walk(const T *x_row, bool x_live, const uint8_t *w_row, const uint8_t *s_row, int64_t KB, int wave,
                                              int g) {
    static_assert(sizeof(T) == 2, "16-bit activations");
    constexpr int U = 2;                                     // k-steps whose loads are requested before the first of them is used
    const int64_t last = KB - 1, steps = (KB + 3) / 4;
    v4f acc = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    bool ff = false;
    for (int64_t c0 = wave; c0 < steps; c0 += kMfmaWaves * U) {
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
    return TileSums{acc, ff};
}

// The eight partial sums, added on wave 0 in wave order: there `s` is column fr, rows 4 g + r, and the result says whether
// weight row fr met a 0xFF byte; the other waves get nothing.  It holds a barrier: every wave of the workgroup calls it.
__device__ __forceinline__ bool tile_reduce(TileLds &lds, const TileSums &part, int wave, int lane, v4f &s) {
#pragma unroll
    for (int r = 0; r < 4; ++r) lds.red[wave][r][lane] = part.acc[r];
    lds.red_ff[wave][lane] = part.ff;
    __syncthreads();
    bool col_nan = false;
    s = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < kMfmaWaves; ++w) {
            col_nan |= lds.red_ff[w][lane] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] += lds.red[w][r][lane];
        }
    }
    return col_nan;
}

// ---------------------------------------------------------------- the pair list of the expert kernels
constexpr int kMaxPairs = 1024;        // MBNB_MOE_MAX_PAIRS == MBNB_MOEMLP_MAX_PAIRS: each library asserts its own
constexpr int kPairRows = 16;          // listed pairs per pass of the decode tile: the rows of the MFMA's A fragment
static_assert(kMaxPairs <= 65536 && kMaxPairs % 64 == 0, "a pair index is 2 bytes in LDS");

__device__ __forceinline__ int lane_rank(uint64_t bm) {     // the set bits of bm below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
}

struct PairCounts { int count, zeros; };

// The id scan.  Every wave scans ALL P ids, 64 per step (a lane past P reads nothing), so every wave knows the counts without a
// barrier and an empty workgroup can leave uniformly before the first one; the list entries of step s are written by wave s % 8.
// The pairs routed to `e` (-1: none) fill list[0 .. count) in ascending pair order; with lists_zeros the pairs whose id is outside
// [0, E) fill list[kMaxPairs - zeros .. kMaxPairs) from the top down (count + zeros <= P <= kMaxPairs: they never meet).
__device__ __forceinline__ PairCounts list_pairs(const int32_t *ids, int P, int e, int E, bool lists_zeros, int wave, int lane, uint16_t *list) {
    int count = 0, zeros = 0;
    for (int s = 0; s * 64 < P; ++s) {
        const int p = s * 64 + lane;
        const bool in = p < P;
        int id = -1;
        if (in) id = ids[p];
        const bool writer = (s % kMfmaWaves) == wave;        // wave-uniform
        const bool mine = in && e >= 0 && id == e;           // e is -1 or inside [0, E): a -1 among the ids is nobody's
        const uint64_t bm = __ballot(mine);
        if (writer && mine) list[count + lane_rank(bm)] = (uint16_t)p;
        count += __popcll(bm);
        if (lists_zeros) {
            const bool oob = in && (id < 0 || id >= E);
            const uint64_t bz = __ballot(oob);
            if (writer && oob) list[kMaxPairs - 1 - zeros - lane_rank(bz)] = (uint16_t)p;
            zeros += __popcll(bz);
        }
    }
    return PairCounts{count, zeros};
}

// ---------------------------------------------------------------- host: the checks of an expert call
// The statuses of mbnb_moe.h and mbnb_moemlp.h, which agree: each library asserts its own against these.
constexpr int kErrArg = -1, kErrShape = -2;

// Rows [., K] of `row_dtype` against [E, N, K] weights for T x A pairs: 0, or the status recorded under the entry point's name.
// max_experts: the library's limit on E, 0 for none.  routed_grid: the launch has ceil(N / 16) x min(E, P) workgroups, else
// ceil(N / 16) x E.
static inline int check_expert_call(const char *what, int64_t T, int64_t A, int64_t K, int row_dtype, int64_t E, int64_t N, int bias_dtype,
                                    bool has_bias, int out_dtype, int64_t max_experts, bool routed_grid) {
    const auto known = [](int d) { return d >= kF16 && d <= kF32; };
    if (!known(row_dtype) || !known(out_dtype) || (has_bias && !known(bias_dtype)))
        return fail(kErrArg, "%s: unknown dtype (rows %d, bias %d, out %d)", what, row_dtype, bias_dtype, out_dtype);
    if (!is16(row_dtype)) return fail(kErrArg, "%s: 16-bit activations only (f16 or bf16 rows)", what);
    if (K <= 0 || K % 32) return fail(kErrShape, "%s: K = %lld is not a positive multiple of the MX block, 32", what, (long long)K);
    if (E <= 0 || N <= 0) return fail(kErrShape, "%s: E = %lld, N = %lld", what, (long long)E, (long long)N);
    if (max_experts && E > max_experts) return fail(kErrShape, "%s: E = %lld experts, at most %lld", what, (long long)E, (long long)max_experts);
    if (T < 0 || A < 0) return fail(kErrShape, "%s: T = %lld, A = %lld", what, (long long)T, (long long)A);
    if (T > 0 && A > kMaxPairs / T)
        return fail(kErrShape, "%s: T x A = %lld x %lld pairs, at most %d in one launch", what, (long long)T, (long long)A, kMaxPairs);
    const int64_t P = T * A;
    if (N > kMaxElems / K || E > kMaxElems / (N * K) || (P > 0 && N > kMaxElems / P))
        return fail(kErrShape, "%s: E x N x K = %lld x %lld x %lld or %lld x N outputs exceed one launch", what, (long long)E, (long long)N,
                    (long long)K, (long long)P);
    const int64_t tiles = (N + 15) / 16, rows = routed_grid && P < E ? P : E;
    if (P > 0 && tiles > INT32_MAX / rows)
        return fail(kErrShape, "%s: %lld x %lld workgroups exceed one launch", what, (long long)tiles, (long long)rows);
    return 0;
}

// The pointers of a call with work to do: none but an optional one is NULL (check_expert_nulls), and each lies on its alignment
// (check_expert_alignment).  Two functions, so that an entry point can put a check of its own between them; `inline`, because
// mx_kernels.hip includes this header and calls neither.
struct Operand {
    const char *name;
    const void *p;
    int align;
    bool optional = false;
};
static inline int check_expert_nulls(const char *what, std::initializer_list<Operand> operands) {
    for (const Operand &o : operands)
        if (!o.p && !o.optional) return fail(kErrArg, "%s: NULL %s", what, o.name);
    return 0;
}
static inline int check_expert_alignment(const char *what, std::initializer_list<Operand> operands) {
    for (const Operand &o : operands)
        if (o.p && !aligned(o.p, (uintptr_t)o.align)) return fail(kErrArg, "%s: misaligned %s (%d bytes)", what, o.name, o.align);
    return 0;
}
static inline int check_expert_pointers(const char *what, std::initializer_list<Operand> operands) {
    const int st = check_expert_nulls(what, operands);
    return st ? st : check_expert_alignment(what, operands);
}

}  // namespace mx
}  // namespace mbnb
