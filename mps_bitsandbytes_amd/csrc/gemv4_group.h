// gemv4_group.h — what k_gemv4_group (group_kernels.hip, libmbnb_group.so) and k_gemv4_group_lora (lora_kernels.hip, libmbnb_lora.so)
// share: the member table in the kernel arguments, the workgroup body (the search for the member, the activation DMA, one weight
// row) and the host checks of a member table.  The rank-R adapter epilogue sits behind `if constexpr (LORA)`: with LORA = false the
// body is k_gemv4_group's, instruction for instruction (DESIGN.md 17 holds the comparison).
//
// Host part: include host.h first (fail / vfail / aligned / is16), as the one source file of a library does.  It also serves the 2 to
// 16 row libraries (skinny4_group.h): the form and KU dispatch and the checks of an adapter table are written here once.
#pragma once
#include "../../include/mbnb_lora.h"      // mbnb_group.h, and the adapter table
#include "gemv4_lean.h"

#include <math.h>
#include <type_traits>

namespace mbnb {

constexpr int kGroupMax = MBNB_GROUP_MAX_MEMBERS;

struct GroupArgs {
    const void *x;                        // the activation row, K elements of the call's dtype
    int64_t K;
    int32_t first_block[kGroupMax + 1];   // cumulative workgroup counts: member i owns [first_block[i], first_block[i+1]); entries past n hold the total
    int32_t n;
    mbnb_group_member m[kGroupMax];
};
static_assert(sizeof(GroupArgs) <= 4096, "the member table must fit the kernel-argument segment");

// a member's adapter as the row body sees it: row n of B is R elements of the call's dtype at b + n R, t the R down-projected
// values in f32.  R == 0: the member has none, and its rows run the body without the epilogue.
struct LoraRow {
    const void *b;
    const float *t;
    int32_t R;
    float scaling;
};
constexpr int kLoraMaxR = 256;     // four wave-wide slices of a row of B

// One weight row, after the activation row has been requested into `xs`: the row's descriptors, every weight / absmax request, the code
// table, the barrier, decode, reduction and the bias add with its double rounding.
//
// THIS IS A COPY of the body of k_gemv4_lean (gemv4_lean.h, everything after its activation DMA, with OutT = T), kept in step BY HAND.
// Sharing one __forceinline__ function between the two kernels was tried and given up: with it k_gemv4_lean kept its instruction
// count, VGPRs, LDS and scratch in all 48 instantiations but not its scalar schedule or SGPR count (1 to 3 fewer, whichever way the
// function was cut), and that kernel must not change.  tests/test_gpu_group.py holds the two equal bit for bit in every KU form.
// `n` (clamped to a row of the weight by the caller; `live` = the row exists) is wave-uniform; `packed`, `am`, `bias`, `out` belong to
// the weight that owns the row.  Every thread of the workgroup must call it (the barrier).
//
// LORA: `lr` is the owning member's adapter (wave-uniform).  With lr.R > 0 the wave requests, before the barrier, its slice of t and
// of row n of B -- lane l takes j = 64 c + l for c < ceil(R / 64), range-checked, so j >= R reads zeros -- and after the main wave sum
// a second one over f32(B[n, j]) * t[j] (a rounded product, then adds) gives u; lane 63 forms (s + scaling * u) + bias and rounds
// as before.  With lr.R == 0 nothing is added: the stored bits are those of LORA = false, a negative zero included.
template <typename T, int QT, bool NESTED, int KU, bool LORA>
__device__ __forceinline__ void group_row(float *lut, const char *xs, const uint8_t *__restrict__ packed, const AbsmaxView &am,
                                          const T *__restrict__ bias, T *__restrict__ out, int64_t n, bool live, int64_t K, int tid,
                                          int lane, const LoraRow *lr) {
    const int64_t nblk = K >> 6, row_bytes = K >> 1;
    // per-wave buffer descriptors: the row's packed bytes, its absmax (NESTED: its codes, and the absmax2 array); n is wave-uniform
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(packed + n * row_bytes), 0, (int)row_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_m = NESTED ? __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(am.i8 + n * nblk), 0, (int)nblk, 0x00020000)
                                               : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(am.f32 + n * nblk), 0, (int)(nblk * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_m2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(NESTED ? am.am2 : am.f32), 0, 0x7FFFFFFC, 0x00020000);
    const int bs2_shift = NESTED ? __builtin_ctz((unsigned)am.bs2) : 0;
    u32x4 wq[KU];
    float a[KU];
    int aq[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) {
        // lane l: packed bytes 16 l .. + 15 of chunk u (k = 2048 u + 32 l .. + 31), one absmax (block 32 u + l / 2)
        wq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, u * 1024, 2));    // aux 2: nt
        if constexpr (!NESTED) {
            a[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_m, (lane >> 1) * 4, u * 128, 0));
        } else {
            const int bi = 32 * u + (lane >> 1);
            aq[u] = __builtin_amdgcn_raw_buffer_load_b32(rs_m, bi & ~3, 0, 0);        // the aligned dword that holds code bi
            const int64_t gi = n * nblk + (bi < (int)nblk ? bi : (int)nblk - 1);     // blocks past the row: code 0 (range check), any valid absmax2
            a[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_m2, (int)((gi >> bs2_shift) << 2), 0, 0));
        }
    }
    // LORA: the wave's slices of row n of B (16-bit loads in the range 2 R bytes) and of t (32-bit loads in the range 4 R bytes)
    constexpr int kSlices = kLoraMaxR / 64;
    int R = 0;
    uint16_t lb[kSlices] = {};
    float lt[kSlices] = {};
    if constexpr (LORA) {
        R = lr->R;
        if (R > 0) {
            const char *brow = static_cast<const char *>(lr->b) + n * (int64_t)R * 2;
            const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(brow), 0, R * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lr->t), 0, R * 4, 0x00020000);
#pragma unroll
            for (int c = 0; c < kSlices; c++) {
                if (64 * c < R) {          // wave-uniform
                    lb[c] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs_b, lane * 2, c * 128, 0);
                    lt[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, lane * 4, c * 256, 0));
                }
            }
        }
    }
    if (tid < 16) lut[tid] = (QT == MBNB_NF4 ? g_nf4_tab : g_fp4_tab)[tid];
    if constexpr (NESTED) {
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int bi = 32 * u + (lane >> 1);
            const float q = (float)(int)(int8_t)(aq[u] >> (8 * (bi & 3)));
            a[u] = q * (a[u] / 127.0f);          // dequantize_blockwise's arithmetic (functional.py:592-594)
        }
    }
    __syncthreads();     // table and activations in LDS (the barrier's fence waits for this wave's loads: all of them are needed now anyway)

    float acc = 0.0f;
    const char *lutb = reinterpret_cast<const char *>(lut);
#pragma unroll
    for (int u = 0; u < KU; u++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t w = wq[u][c];
            const u32x4 xq = *reinterpret_cast<const u32x4 *>(xs + (2048 * u + 32 * lane + 8 * c) * 2);
            const uint32_t wo = w & 0xF0F0F0F0u;
            const uint32_t we = (w << 2) & 0x3C3C3C3Cu;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float lo = *reinterpret_cast<const float *>(lutb + bfe_u32(we, 8 * j, 8));
                const float hi = *reinterpret_cast<const float *>(lutb + bfe_u32(wo, 8 * j + 2, 6));
                const f32x2 pr = f32x2{lo, hi} * f32x2{a[u], a[u]};      // two IEEE f32 products
                acc = Dot2<T>::run(pack2<T>(pr[0], pr[1]), xq[j], acc);
            }
        }
    }
    float s = dpp_wave_sum(acc);
    if constexpr (LORA) {
        if (R > 0) {
            float p = 0.0f;
#pragma unroll
            for (int c = 0; c < kSlices; c++)
                if (64 * c < R) p += to_f32(__builtin_bit_cast(T, lb[c])) * lt[c];      // a rounded product, then the add (-ffp-contract=off)
            const float up = dpp_wave_sum(p);
            s += lr->scaling * up;
        }
    }
    if (lane == 63 && live) {
        const float v = s + (bias ? to_f32(bias[n]) : 0.0f);
        out[n] = from_f32<T>(to_f32(from_f32<T>(v)));
    }
}

// The workgroup of both kernels: four rows of ONE member.  `lut` is the kernel's 16-float table, `xs` its dynamic LDS (K * 2 bytes,
// KU * 4096 allocated); `rows` is the adapter table of the LORA kernel, indexed like a.m (unused otherwise).
template <typename T, int QT, bool NESTED, int KU, bool LORA>
__device__ __forceinline__ void group_workgroup(const GroupArgs &a, const LoraRow *rows, float *lut, char *xs) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the member that owns this workgroup: a compare chain over the prefix array (kernel arguments and blockIdx only: scalar), so the
    // table is never indexed by a register the compiler could take for divergent
    const int blk = (int)blockIdx.x;
    int g = 0, first = 0;
#pragma unroll
    for (int i = 1; i < kGroupMax; i++) {
        const int fb = a.first_block[i];     // nondecreasing; the total from member n on
        g = fb <= blk ? i : g;
        first = fb <= blk ? fb : first;
    }
    g = __builtin_amdgcn_readfirstlane(g);
    const int64_t K = a.K;

    // ---- activations -> LDS, as in k_gemv4_lean (1 KiB per wave-instruction; bytes past the K activations read as zeros)
    {
        typedef int i32x4_t __attribute__((ext_vector_type(4)));
        const uint64_t px = reinterpret_cast<uint64_t>(a.x);
        i32x4_t rs_x = i32x4_t{(int)(uint32_t)px, (int)(uint32_t)(px >> 32), (int)(K * 2), 0x00020000};
#pragma unroll
        for (int e = 0; e < 4; e++) rs_x[e] = __builtin_amdgcn_readfirstlane(rs_x[e]);
        const uint32_t xs_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)xs;
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(xs_base + 4096u * u + 1024u * wave));
            const int vo = 4096 * u + tid * 16;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(dst), "v"(vo), "s"(rs_x) : "memory", "m0");
        }
    }
    // the member's own N (dead-row clamp) and its own absmax arrays (the nested index of group_row starts at the member's row 0)
    const mbnb_group_member &m = a.m[g];
    const int64_t N = m.N;
    int64_t n = (int64_t)(blk - first) * 4 + wave;
    const bool live = n < N;
    n = live ? n : N - 1;
    const AbsmaxView am{m.absmax_f32, m.absmax_i8, m.absmax2, m.blocksize2};
    group_row<T, QT, NESTED, KU, LORA>(lut, xs, static_cast<const uint8_t *>(m.packed), am, static_cast<const T *>(m.bias), static_cast<T *>(m.out), n,
                                       live, K, tid, lane, LORA ? rows + g : nullptr);
}

// KU of the instantiation that serves ceil(K / 2048) = ku chunks (the lean launcher's choice)
static int group_ku_form(int ku) { return ku <= 4 ? ku : ku <= 6 ? 6 : 8; }

// f(KU as a compile-time constant) for a KU that group_ku_form gave: the launches of every kernel that has a KU form
template <typename F> void with_ku(int KU, F &&f) {
    switch (KU) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
}

// FN<T, QT, NESTED>(...) for the call's form: {f16, bf16} x {NF4, FP4} x {plain, double-quantised absmax}
#define MBNB_GROUP_FORMS(DTYPE, QUANT, NESTED, FN, ...)                                                                             \
    ((DTYPE) == MBNB_GROUP_F16                                                                                                      \
         ? ((QUANT) == MBNB_GROUP_NF4                                                                                               \
                ? ((NESTED) ? FN<mbnb::f16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<mbnb::f16_t, MBNB_NF4, false>(__VA_ARGS__))         \
                : ((NESTED) ? FN<mbnb::f16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<mbnb::f16_t, MBNB_FP4, false>(__VA_ARGS__)))        \
         : ((QUANT) == MBNB_GROUP_NF4                                                                                               \
                ? ((NESTED) ? FN<mbnb::bf16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<mbnb::bf16_t, MBNB_NF4, false>(__VA_ARGS__))       \
                : ((NESTED) ? FN<mbnb::bf16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<mbnb::bf16_t, MBNB_FP4, false>(__VA_ARGS__))))

// ---------------------------------------------------------------- host side: the checks of a member table, for both libraries
// `who` is the entry point's name in the error texts.  group_argument_errors: 0, or the negative code of an argument error (n == 0 is
// the caller's no-op and never comes here).  group_conditions: 0 with `a` filled and `nested` set, or `not_applicable` after recording
// the reason: the conditions of the fused launch (those of k_gemv4_lean, matmul4_kernels.hip) live here and nowhere else.
static int group_argument_errors(const char *who, const void *x, int64_t K, int quant_type, int dtype, int blocksize,
                                 const mbnb_group_member *members, int n, int flags) {
    if (n < 0 || n > kGroupMax) return fail(MBNB_GROUP_ERR_ARG, "%s: n = %d members, 0..%d per call", who, n, kGroupMax);
    if (!members) return fail(MBNB_GROUP_ERR_ARG, "%s: NULL member table", who);
    if (!x) return fail(MBNB_GROUP_ERR_ARG, "%s: NULL x", who);
    if (dtype < MBNB_GROUP_F16 || dtype > MBNB_GROUP_F32) return fail(MBNB_GROUP_ERR_ARG, "%s: unknown dtype %d", who, dtype);
    if (quant_type != MBNB_GROUP_NF4 && quant_type != MBNB_GROUP_FP4) return fail(MBNB_GROUP_ERR_ARG, "%s: unknown quant type %d", who, quant_type);
    if (flags) return fail(MBNB_GROUP_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    if (K <= 0 || blocksize <= 0) return fail(MBNB_GROUP_ERR_SHAPE, "%s: K = %lld, blocksize = %d", who, (long long)K, blocksize);
    for (int i = 0; i < n; ++i) {
        const mbnb_group_member &m = members[i];
        if (!m.packed || !m.out) return fail(MBNB_GROUP_ERR_ARG, "%s: member %d has a NULL packed or out pointer", who, i);
        if (!m.absmax_f32 && !m.absmax_i8) return fail(MBNB_GROUP_ERR_ARG, "%s: member %d has no absmax", who, i);
        if (m.absmax_i8 && !m.absmax2) return fail(MBNB_GROUP_ERR_ARG, "%s: member %d has int8 absmax codes without absmax2", who, i);
        if (m.N <= 0) return fail(MBNB_GROUP_ERR_SHAPE, "%s: member %d has N = %lld", who, i, (long long)m.N);
    }
    return 0;
}

static int group_conditions(const char *who, int not_applicable, const void *x, int64_t K, int dtype, int blocksize,
                            const mbnb_group_member *members, int n, GroupArgs &a, bool &nested) {
    if (!is16(dtype)) return fail(not_applicable, "%s: a 16-bit dtype is needed, got dtype %d", who, dtype);
    if (blocksize != 64) return fail(not_applicable, "%s: blocksize 64 is needed, got %d", who, blocksize);
    if (K % 64 != 0 || K < 1024 || K > 16384)
        return fail(not_applicable, "%s: K %% 64 == 0 and 1024 <= K <= 16384 are needed, got K = %lld", who, (long long)K);
    if (!aligned(x, 16)) return fail(not_applicable, "%s: x is not 16-byte aligned", who);
    nested = members[0].absmax_i8 != nullptr;
    a.x = x;
    a.K = K;
    a.n = n;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const mbnb_group_member &m = members[i];
        if (!aligned(m.packed, 16)) return fail(not_applicable, "%s: member %d's packed weight is not 16-byte aligned", who, i);
        if (m.N >= ((int64_t)1 << 40) || m.N * (K / 2) >= ((int64_t)1 << 40))
            return fail(not_applicable, "%s: member %d's packed weight has 2^40 bytes or more", who, i);
        if ((m.absmax_i8 != nullptr) != nested)
            return fail(not_applicable, "%s: plain and double-quantised absmax in one group (member %d differs from member 0)", who, i);
        if (nested) {
            if (m.blocksize2 <= 0 || (m.blocksize2 & (m.blocksize2 - 1)) != 0)
                return fail(not_applicable, "%s: member %d's blocksize2 %d is no power of two", who, i, m.blocksize2);
            if (!aligned(m.absmax_i8, 4)) return fail(not_applicable, "%s: member %d's absmax codes are not 4-byte aligned", who, i);
            if ((K / 64) % 4 != 0)
                return fail(not_applicable, "%s: double-quantised absmax needs (K / 64) %% 4 == 0, got K = %lld", who, (long long)K);
        }
        a.first_block[i] = (int32_t)blocks;
        blocks += (m.N + 3) / 4;
        if (blocks >= ((int64_t)1 << 31)) return fail(not_applicable, "%s: 2^31 workgroups or more", who);
        a.m[i] = m;
        a.m[i].pad_ = 0;
    }
    for (int i = n; i <= kGroupMax; ++i) a.first_block[i] = (int32_t)blocks;
    for (int i = n; i < kGroupMax; ++i) a.m[i] = mbnb_group_member{};
    return 0;
}

// ---------------------------------------------------------------- host side: the checks of an adapter table, one adapter per member
// adapter_argument_errors: 0, or the negative code of an argument error.  adapter_conditions: 0 with rows[kGroupMax] filled and, in
// the down-projection table `d` (a library's own DownArgs), first_row[kGroupMax + 1] and every m[i].a / m[i].t, or `not_applicable`
// after recording the reason; `plain` names the entry point that serves a table without any adapter.
static_assert(MBNB_LORA_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_LORA_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "one set of argument-error codes");
static int adapter_argument_errors(const char *who, const mbnb_lora_adapter *adapters, int n) {
    if (!adapters) return fail(MBNB_LORA_ERR_ARG, "%s: NULL adapter table", who);
    for (int i = 0; i < n; ++i) {
        const mbnb_lora_adapter &ad = adapters[i];
        if (ad.R < 0) return fail(MBNB_LORA_ERR_SHAPE, "%s: member %d has R = %d", who, i, ad.R);
        if (ad.R > 0 && (!ad.a || !ad.b)) return fail(MBNB_LORA_ERR_ARG, "%s: member %d has R = %d with a NULL a or b", who, i, ad.R);
    }
    return 0;
}

template <typename Down>
int adapter_conditions(const char *who, int not_applicable, const char *plain, const mbnb_lora_adapter *adapters, int n, Down &d, LoraRow *rows) {
    const int na = not_applicable;
    int total = 0;
    for (int i = 0; i < kGroupMax; ++i) {
        d.first_row[i] = total;
        d.m[i].a = nullptr;
        d.m[i].t = nullptr;
        rows[i] = LoraRow{nullptr, nullptr, 0, 0.0f};
        if (i >= n || adapters[i].R == 0) continue;
        const mbnb_lora_adapter &ad = adapters[i];
        if (ad.R > MBNB_LORA_MAX_R) return fail(na, "%s: member %d has R = %d, 1 <= R <= %d is needed", who, i, ad.R, MBNB_LORA_MAX_R);
        if (!aligned(ad.a, 16)) return fail(na, "%s: member %d's a is not 16-byte aligned", who, i);
        if (!aligned(ad.b, 2)) return fail(na, "%s: member %d's b is not 2-byte aligned", who, i);
        if (!ad.t || !aligned(ad.t, 4)) return fail(na, "%s: member %d's t is NULL or not 4-byte aligned", who, i);
        if (!isfinite(ad.scaling)) return fail(na, "%s: member %d's scaling is not finite", who, i);
        d.m[i].a = ad.a;
        d.m[i].t = ad.t;
        rows[i] = LoraRow{ad.b, ad.t, ad.R, ad.scaling};
        total += ad.R;
    }
    d.first_row[kGroupMax] = total;
    if (total == 0) return fail(na, "%s: no member has an adapter (R > 0): the call is %s's", who, plain);
    return 0;
}

}  // namespace mbnb
