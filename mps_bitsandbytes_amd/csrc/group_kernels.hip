// group_kernels.hip — the grouped M = 1 decode GEMV and the C ABI of libmbnb_group.so (include/mbnb_group.h).
//
// k_gemv4_lean (gemv4_lean.h) spends about 2 of its 5 us per 4096^2 layer on what does not depend on the weight: the launch, staging
// the activation row into LDS, the code table, the barrier.  A decoder block hands the same row to q / k / v and
// again to gate / up; k_gemv4_group serves the rows of all those weights from ONE launch.  A workgroup still owns four rows of one
// weight and runs the arithmetic of k_gemv4_lean on them (group_row below), so each output equals mbnb_matmul_4bit's bit for bit; what
// is new is the member table in the kernel arguments and the search that tells a workgroup whose rows it has.
#include "../../include/mbnb_group.h"
#include "gemv4_lean.h"
#include "host.h"

static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");
static_assert(MBNB_GROUP_F16 == MBNB_F16 && MBNB_GROUP_BF16 == MBNB_BF16 && MBNB_GROUP_F32 == MBNB_F32, "dtype codes of mbnb_hip.h");
static_assert(MBNB_GROUP_NF4 == MBNB_NF4 && MBNB_GROUP_FP4 == MBNB_FP4, "code tables of mbnb_hip.h");

namespace {

using mbnb::AbsmaxView;
using mbnb::aligned;
using mbnb::bf16_t;
using mbnb::bfe_u32;
using mbnb::Dot2;
using mbnb::dpp_wave_sum;
using mbnb::f16_t;
using mbnb::f32x2;
using mbnb::fail;
using mbnb::from_f32;
using mbnb::g_fp4_tab;
using mbnb::g_nf4_tab;
using mbnb::pack2;
using mbnb::to_f32;
using mbnb::u32x4;

constexpr int kMax = MBNB_GROUP_MAX_MEMBERS;

struct GroupArgs {
    const void *x;                   // the activation row, K elements of the call's dtype
    int64_t K;
    int32_t first_block[kMax + 1];   // cumulative workgroup counts: member i owns [first_block[i], first_block[i+1]); entries past n hold the total
    int32_t n;
    mbnb_group_member m[kMax];
};
static_assert(sizeof(GroupArgs) <= 4096, "the member table must fit the kernel-argument segment");

// One weight row, after the activation row has been requested into `xs`: the row's descriptors, every weight / absmax request, the code
// table, the barrier, decode, reduction and the bias add with its double rounding.
//
// THIS IS A COPY of the body of k_gemv4_lean (gemv4_lean.h, everything after its activation DMA, with OutT = T), kept in step BY HAND.
// Sharing one __forceinline__ function between the two kernels was tried and given up: with it k_gemv4_lean kept its instruction
// count, VGPRs, LDS and scratch in all 48 instantiations but not its scalar schedule or SGPR count (1 to 3 fewer, whichever way the
// function was cut), and that kernel must not change.  tests/test_gpu_group.py holds the two equal bit for bit in every KU form.
// `n` (clamped to a row of the weight by the caller; `live` = the row exists) is wave-uniform; `packed`, `am`, `bias`, `out` belong to
// the weight that owns the row.  Every thread of the workgroup must call it (the barrier).
template <typename T, int QT, bool NESTED, int KU>
__device__ __forceinline__ void group_row(float *lut, const char *xs, const uint8_t *__restrict__ packed, const AbsmaxView &am,
                                          const T *__restrict__ bias, T *__restrict__ out, int64_t n, bool live, int64_t K, int tid,
                                          int lane) {
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
    const float s = dpp_wave_sum(acc);
    if (lane == 63 && live) {
        const float v = s + (bias ? to_f32(bias[n]) : 0.0f);
        out[n] = from_f32<T>(to_f32(from_f32<T>(v)));
    }
}

template <typename T, int QT, bool NESTED, int KU>
__global__ __launch_bounds__(256) void k_gemv4_group(const GroupArgs a) {
    __shared__ float lut[16];
    extern __shared__ __attribute__((aligned(16))) char xs[];      // the activation row: K * 2 bytes
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the member that owns this workgroup: a compare chain over the prefix array (kernel arguments and blockIdx only: scalar), so the
    // table is never indexed by a register the compiler could take for divergent
    const int blk = (int)blockIdx.x;
    int g = 0, first = 0;
#pragma unroll
    for (int i = 1; i < kMax; i++) {
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
    group_row<T, QT, NESTED, KU>(lut, xs, static_cast<const uint8_t *>(m.packed), am, static_cast<const T *>(m.bias), static_cast<T *>(m.out), n,
                                 live, K, tid, lane);
}

// ---------------------------------------------------------------- host side
char *last_launch() {
    static thread_local char text[64] = "";
    return text;
}

template <typename T, int QT, bool NESTED>
int launch(const GroupArgs &a, hipStream_t stream) {
    const int ku = (int)((a.K + 2047) / 2048);
    const dim3 grid((unsigned)a.first_block[a.n]);
    int KU;
#define MBNB_GROUP(KU_)                                                                                               \
    do {                                                                                                              \
        hipLaunchKernelGGL((k_gemv4_group<T, QT, NESTED, KU_>), grid, dim3(256), (size_t)KU_ * 4096, stream, a);      \
        KU = KU_;                                                                                                     \
    } while (0)
    if (ku == 1) MBNB_GROUP(1);
    else if (ku == 2) MBNB_GROUP(2);
    else if (ku == 3) MBNB_GROUP(3);
    else if (ku == 4) MBNB_GROUP(4);
    else if (ku <= 6) MBNB_GROUP(6);
    else MBNB_GROUP(8);
#undef MBNB_GROUP
    const int rc = mbnb::launch_status("mbnb_group_gemv4");
    if (rc == 0) snprintf(last_launch(), 64, "gemv_group G%d ku%d/KU%d", a.n, ku, KU);
    return rc;
}

template <typename T>
int dispatch_form(int qt, bool nested, const GroupArgs &a, hipStream_t stream) {
    if (qt == MBNB_GROUP_NF4) return nested ? launch<T, MBNB_NF4, true>(a, stream) : launch<T, MBNB_NF4, false>(a, stream);
    return nested ? launch<T, MBNB_FP4, true>(a, stream) : launch<T, MBNB_FP4, false>(a, stream);
}

int not_applicable(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int not_applicable(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = mbnb::vfail(MBNB_GROUP_NOT_APPLICABLE, fmt, ap);
    va_end(ap);
    return rc;
}

}  // namespace

extern "C" {

int mbnb_group_abi_version(void) { return MBNB_GROUP_ABI_VERSION; }

const char *mbnb_group_last_error(void) { return mbnb::last_error(); }

const char *mbnb_group_last_launch(void) { return last_launch(); }

int mbnb_group_gemv4(const void *x, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members, int n,
                     int flags, void *stream) {
    // ---- argument errors
    if (n < 0 || n > kMax) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: n = %d members, 0..%d per call", n, kMax);
    if (n == 0) return 0;
    if (!members) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: NULL member table");
    if (!x) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: NULL x");
    if (dtype < MBNB_GROUP_F16 || dtype > MBNB_GROUP_F32) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: unknown dtype %d", dtype);
    if (quant_type != MBNB_GROUP_NF4 && quant_type != MBNB_GROUP_FP4)
        return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: unknown quant type %d", quant_type);
    if (flags) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: unknown flags 0x%x", flags);
    if (K <= 0 || blocksize <= 0)
        return fail(MBNB_GROUP_ERR_SHAPE, "mbnb_group_gemv4: K = %lld, blocksize = %d", (long long)K, blocksize);
    for (int i = 0; i < n; ++i) {
        const mbnb_group_member &m = members[i];
        if (!m.packed || !m.out) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: member %d has a NULL packed or out pointer", i);
        if (!m.absmax_f32 && !m.absmax_i8) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: member %d has no absmax", i);
        if (m.absmax_i8 && !m.absmax2) return fail(MBNB_GROUP_ERR_ARG, "mbnb_group_gemv4: member %d has int8 absmax codes without absmax2", i);
        if (m.N <= 0) return fail(MBNB_GROUP_ERR_SHAPE, "mbnb_group_gemv4: member %d has N = %lld", i, (long long)m.N);
    }
    // ---- the conditions of the fused launch (those of k_gemv4_lean, matmul4_kernels.hip); this is the one place they live
    if (!mbnb::is16(dtype)) return not_applicable("mbnb_group_gemv4: a 16-bit dtype is needed, got dtype %d", dtype);
    if (blocksize != 64) return not_applicable("mbnb_group_gemv4: blocksize 64 is needed, got %d", blocksize);
    if (K % 64 != 0 || K < 1024 || K > 16384)
        return not_applicable("mbnb_group_gemv4: K %% 64 == 0 and 1024 <= K <= 16384 are needed, got K = %lld", (long long)K);
    if (!aligned(x, 16)) return not_applicable("mbnb_group_gemv4: x is not 16-byte aligned");
    const bool nested = members[0].absmax_i8 != nullptr;
    GroupArgs a;
    a.x = x;
    a.K = K;
    a.n = n;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const mbnb_group_member &m = members[i];
        if (!aligned(m.packed, 16)) return not_applicable("mbnb_group_gemv4: member %d's packed weight is not 16-byte aligned", i);
        if (m.N >= ((int64_t)1 << 40) || m.N * (K / 2) >= ((int64_t)1 << 40))
            return not_applicable("mbnb_group_gemv4: member %d's packed weight has 2^40 bytes or more", i);
        if ((m.absmax_i8 != nullptr) != nested)
            return not_applicable("mbnb_group_gemv4: plain and double-quantised absmax in one group (member %d differs from member 0)", i);
        if (nested) {
            if (m.blocksize2 <= 0 || (m.blocksize2 & (m.blocksize2 - 1)) != 0)
                return not_applicable("mbnb_group_gemv4: member %d's blocksize2 %d is no power of two", i, m.blocksize2);
            if (!aligned(m.absmax_i8, 4)) return not_applicable("mbnb_group_gemv4: member %d's absmax codes are not 4-byte aligned", i);
            if ((K / 64) % 4 != 0)
                return not_applicable("mbnb_group_gemv4: double-quantised absmax needs (K / 64) %% 4 == 0, got K = %lld", (long long)K);
        }
        a.first_block[i] = (int32_t)blocks;
        blocks += (m.N + 3) / 4;
        if (blocks >= ((int64_t)1 << 31)) return not_applicable("mbnb_group_gemv4: 2^31 workgroups or more");
        a.m[i] = m;
        a.m[i].pad_ = 0;
    }
    for (int i = n; i <= kMax; ++i) a.first_block[i] = (int32_t)blocks;
    for (int i = n; i < kMax; ++i) a.m[i] = mbnb_group_member{};
    hipStream_t s = (hipStream_t)stream;
    return dtype == MBNB_GROUP_F16 ? dispatch_form<f16_t>(quant_type, nested, a, s) : dispatch_form<bf16_t>(quant_type, nested, a, s);
}

}  // extern "C"
