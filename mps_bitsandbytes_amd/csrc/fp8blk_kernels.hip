// fp8blk_kernels.hip — the block-scaled FP8 linear (128 x 128 weight blocks, 1 x 128 activation groups, f32 scales): two
// quantisers to OCP E4M3 and a GEMM with two-level accumulation on gfx950's FP8 MFMA, and the C ABI of libmbnb_fp8blk.so
// (include/mbnb_fp8blk.h; the semantics, the design and the figures: DESIGN.md §38).
//
//   k_fp8_quantize_groups  x [M, K] of f16 / bf16 / f32 -> codes uint8 [M, K] and one f32 scale per row and 128-wide k group.  A
//                          thread owns one chunk of 16 elements, the eight lanes of a group reduce their maximum by three lane
//                          exchanges: every element is read once, no LDS; a workgroup serves 32 groups.
//   k_fp8_quantize_blocks  w [N, K] -> codes uint8 [N, K] and one f32 scale per 128 x 128 block.  One workgroup per block, a
//                          thread holds four chunks of 16 in registers between the maximum and the encoding: one read.
//   k_gemm_fp8_block       out[m, n] = sum_t (sA[m, t] * sW[n / 128, t]) * (A_t . W_t^T)[m, n] + bias[n]: one K-step of
//                          v_mfma_scale_f32_16x16x128_f8f6f4 (unit scale bytes) per scale group into a fresh partial, folded into
//                          the running sum on the vector ALU under the MFMAs that follow (see the kernel).
#include "../../include/mbnb_fp8blk.h"
#include "host.h"

#include <atomic>

static_assert(MBNB_FP8BLK_F16 == mbnb::kF16 && MBNB_FP8BLK_BF16 == mbnb::kBF16 && MBNB_FP8BLK_F32 == mbnb::kF32, "host.h's dtype codes");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;              // every launch: 4 waves
constexpr int kBlock = MBNB_FP8BLK_BLOCK;  // the scale block's edge
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// ---------------------------------------------------------------- the quantisers
// The operation chain of fp8_kernels.hip's fp8_enc_e4m3 (mx_scaled.h's enc_e4m3), restated: this library links to no other and a
// host test closes that header's includers.  The bits of |a| -> E4M3 code 0..0x7E, round to nearest even, saturating at 448
// (an Inf saturates with it)
__device__ __forceinline__ uint32_t blk_enc_e4m3(uint32_t a) {
    if (a >= 0x3C800000u) {                                  // 2^-6 and up: the normal codes
        a += 0x7FFFFu + ((a >> 20) & 1u);                    // RNE at mantissa bit 20; a carry moves into the exponent
        const uint32_t code = (a >> 20) - (120u << 3);       // exponent bias 127 -> 7
        return code < 0x7Eu ? code : 0x7Eu;
    }
    return (uint32_t)rintf(__uint_as_float(a) * 512.0f);     // multiples of 2^-9: 0..8, and 8 is the first normal code
}

// 16 consecutive elements as f32: 16-byte loads
template <typename T> __device__ __forceinline__ void load16(const T *p, float v[16]) {
    typedef T tvec __attribute__((ext_vector_type(8)));
    const tvec a = ((const tvec *)p)[0], b = ((const tvec *)p)[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j], v[8 + j] = (float)b[j];
}
template <> __device__ __forceinline__ void load16<float>(const float *p, float v[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 t = ((const f32x4 *)p)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * q + j] = t[j];
    }
}

__device__ __forceinline__ uint32_t max_abs_bits(const float v[16], uint32_t m) {
#pragma unroll
    for (int j = 0; j < 16; ++j) m = max(m, __float_as_uint(v[j]) & 0x7FFFFFFFu);
    return m;
}

// the 16 codes of v under the multiplier r, as one 16-byte store; `live` false: codes 0
__device__ __forceinline__ void store_codes(uint8_t *q, const float v[16], float r, bool live) {
    i32x4 w = i32x4{0, 0, 0, 0};
    if (live) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t a = __float_as_uint(v[j] * r) & 0x7FFFFFFFu;
            if (a > 0x7F800000u) a = 0;                      // 0 x an overflowed r: the element was a zero
            w[j >> 2] |= (int)((blk_enc_e4m3(a) | ((__float_as_uint(v[j]) >> 24) & 0x80u)) << (8 * (j & 3)));   // the sign of x
        }
    }
    *(i32x4 *)q = w;
}

// the scale of a group whose maximum has the bits m
__device__ __forceinline__ float scale_of(uint32_t m) { return m >= 0x7F800000u ? __uint_as_float(kQuietNaN) : __uint_as_float(m) / 448.0f; }

// Group G = row * KB + t of the activation: lanes 8 q .. 8 q + 7 of a wave hold its eight chunks (fewer in a row's last group),
// so the maximum is three exchanges away and sA is written in the order of the groups.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp8_quantize_groups(const T *__restrict__ x, int64_t M, int64_t K, int64_t KB,
                                                                  uint8_t *__restrict__ q, float *__restrict__ sA) {
    const int tid = threadIdx.x, c8 = tid & 7;
    const int64_t G = (int64_t)blockIdx.x * (kThreads / 8) + (tid >> 3);
    const int64_t row = G / KB, k = (G % KB) * kBlock + 16 * c8;
    const bool mine = row < M && k < K;                      // a chunk past K of a partial group, a group past the last row: idle

    float v[16];
    uint32_t m = 0;
    if (mine) {
        load16<T>(x + row * K + k, v);
        m = max_abs_bits(v, 0);
    }
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));

    const bool live = m != 0u && m < 0x7F800000u;            // not an all-zero group, no Inf or NaN in it
    const float r = 448.0f / __uint_as_float(m);
    if (c8 == 0 && row < M) sA[G] = scale_of(m);
    if (mine) store_codes(q + row * K + k, v, r, live);
}

// Block (nb, kb) of the weight: chunk c = 256 i + tid of its 128 rows x 8 chunks, so a thread's four chunks are rows
// 32 i + (tid >> 3) at the k of chunk tid & 7.  Rows past N and chunks past K are idle.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp8_quantize_blocks(const T *__restrict__ w, int64_t N, int64_t K, int64_t KB,
                                                                  uint8_t *__restrict__ q, float *__restrict__ sW) {
    __shared__ uint32_t wave_max[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)(blockIdx.x / KB) * kBlock, k = (int64_t)(blockIdx.x % KB) * kBlock + 16 * (tid & 7);

    float held[4][16];
    bool mine[4];
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = n0 + 32 * i + (tid >> 3);
        mine[i] = row < N && k < K;
        if (mine[i]) {
            load16<T>(w + row * K + k, held[i]);
            m = max_abs_bits(held[i], m);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if ((tid & 63) == 0) wave_max[tid >> 6] = m;
    __syncthreads();
    m = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));

    const bool live = m != 0u && m < 0x7F800000u;
    const float r = 448.0f / __uint_as_float(m);
    if (tid == 0) sW[blockIdx.x] = scale_of(m);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (mine[i]) store_codes(q + (n0 + 32 * i + (tid >> 3)) * K + k, held[i], r, live);
}

// ---------------------------------------------------------------- the GEMM
// One workgroup = four waves = one 128 x 128 output tile, n0 a multiple of 128: its columns lie in ONE block row nb of sW, so
// sW[nb, t] is one uniform value per K-step.  Wave (wm = w & 1, wn = w >> 1) owns rows 64 wm .. + 64 and columns 64 wn .. + 64 as
// 4 x 4 accumulators of 16 x 16.
//
// The instruction, the LDS image and the LDS-DMA are k_gemm_fp8's (fp8_kernels.hip): lane l = (g = l >> 4,
// fr = l & 15) holds row fr of its operand, registers 0..3 the 16 k from 16 g, 4..7 the 16 k from 64 + 16 g; the WEIGHT is the
// first operand, so D holds four consecutive n (4 g + r) of output row fr; two LDS stages of a K-step, each the activation tile
// then the weight tile in chunk order [half][row][g]; NPS = 8 LDS-DMA instructions per wave and stage.
//
// What is new is the two-level sum.  A K-step is one scale group of both operands, so the MFMA of K-step t may not add to the
// running sum: it writes a FRESH partial (source C is the constant 0), and the vector ALU folds it in,
//     acc = fmaf(partial, sA[m, t] * sW[nb, t], acc),
// four fmaf per lane and MFMA with one scale product sp[j] per activation fragment j.  The fold of MFMA (i, j) stands behind MFMA
// (i + 1, j): the NJ MFMAs (8 passes each) between the two are far more than the 11 wait states the matrix pipe needs before a
// VALU may read its result, and the VALU runs beside the matrix pipe, not after it.  The fold of the last MFMA row of K-step t
// stands in the first row of K-step t + 1 (with the products of t, which are replaced only behind that row); the first K-step
// folds a zero partial with a zero product, the last row of the last K-step is folded behind the loop, behind explicit nops.
// The order of the MFMAs and folds is pinned by statements without an instruction through which the partial and the sum pass
// (and sched_barriers): the compiler does not know the latency of an MFMA in assembly and would move the folds behind the last one.
//
// The register plan.  The VALU writes the running sums, so they are architectural VGPRs, unlike k_gemm_fp8's accumulators.  A
// 256 x 128 tile with the 96 fragment registers of a K-step in AGPRs assembles, but the allocator loads the fragments into VGPRs
// and copies them in front of every MFMA (profiles/fp8blk_resource_usage.txt), so the tile is 128 x 128 and everything is
// architectural: 4 x 4 x 4 = 64 running sums, 8 x 8 = 64 fragment registers, about 5 partials in flight x 4, the 4 scale products
// (one tuple), the 4 activation scales of the next K-step and the addresses: 220 VGPRs, no AGPR, no scratch, two workgroups per CU.
//
// The pipeline, with every wait (vector-memory operations retire in order: the count is what was issued AFTER what is awaited):
//
//   before the loop: sA of K-step 0 (NJ loads), DMA of K-step 0, DMA of K-step 1; vmcnt(NPS): sA(0) and K-step 0 are there,
//                    DMA(1) is in flight; barrier; the fragments of K-step 0
//   K-step t:   MFMA row 0 (+ folds of row 3 of t - 1)
//               lgkmcnt(0), barrier B1       every wave holds the fragments of t: stage t & 1 is free
//               vmcnt(NPS)                   sA(t) is there (issued a K-step ago); DMA(t + 1) is in flight (the compiler's wait
//                                            pass, which sees sA(t) used, strengthens this one to vmcnt(0): stricter, no race)
//               sp[j] = sA(t)[j] * sW(t); loads of sA(t + 1) (NJ), then the LDS-DMA of K-step t + 2 -> stage t & 1 (NPS)
//               MFMA row 1 (+ folds of row 0)
//               vmcnt(NPS + NJ), barrier B2  DMA(t + 1) has landed for every wave; sA(t + 1) and DMA(t + 2) stay in flight
//               fragment reads of t + 1 from stage (t + 1) & 1 into the registers of MFMA rows that are done
//               MFMA rows 2, 3 (+ folds of rows 1, 2)
//
// Edges (k_gemm_fp8's rules): chunks of rows past M / N and of k past K are fetched from the operand's first 16 bytes, so every
// K-step issues the same instructions and the counts hold; on the last step of a K % 128 != 0 problem the k past K are zeroed
// in registers in both operands; the sA of rows past M are those of row M - 1, the scales of the K-step past the end those of the
// last; nothing past the edge is stored; row and byte offsets are 64-bit.
constexpr int TM = MBNB_FP8BLK_TILE_M, TN = MBNB_FP8BLK_TILE_N, KS = MBNB_FP8BLK_K_STEP;
static_assert(TM == 128 && TN == kBlock && KS == kBlock && MBNB_FP8BLK_STEPS_IN_FLIGHT == 2, "the wave grid, the chunk maps and the waits below");

constexpr int X_BYTES = TM * KS, W_BYTES = TN * KS, STAGE = X_BYTES + W_BYTES, LDS_BYTES = 2 * STAGE;
constexpr int NX = X_BYTES / 16 / kThreads, NW = W_BYTES / 16 / kThreads, NPS = NX + NW;   // LDS-DMA instructions per thread and stage
constexpr int NI = TN / 32, NJ = TM / 32;                    // weight / activation fragments of a wave
constexpr int XQ = NX / 2, WQ = NW / 2;                      // row groups of 64 per half of an image

__device__ __forceinline__ void lds_dma16(const uint8_t *src, uint8_t *wave_dst) {   // 64 lanes x 16 bytes, lane l to wave_dst + 16 l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)wave_dst, 16, 0,
                                     0);
}

// s_waitcnt vmcnt(n) alone, the other counters left at their maxima (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
constexpr int vmcnt_only(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

__device__ __forceinline__ float bias_at(const void *bias, int dtype, int64_t n) {
    return dtype == mbnb::kF32 ? ((const float *)bias)[n] : dtype == mbnb::kBF16 ? (float)((const bf16_t *)bias)[n] : (float)((const f16_t *)bias)[n];
}

template <typename TO>
__global__ __launch_bounds__(kThreads, 1) void k_gemm_fp8_block(const uint8_t *__restrict__ A, const float *sA, const uint8_t *__restrict__ W,
                                                                const float *__restrict__ sW, int64_t M, int64_t N, int64_t K,
                                                                const void *__restrict__ bias, int bias_dtype, TO *__restrict__ out, int tiles_m) {
#if defined(__HIP_DEVICE_COMPILE__)                           // the host pass keeps the stub alone: the assembly below is gfx950's
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)(blockIdx.x % tiles_m) * TM, n0 = (int64_t)(blockIdx.x / tiles_m) * TN;
    const int nk = (int)((K + KS - 1) / KS);                 // = KB: a K-step is a scale group
    const int last_partial = K % KS ? nk - 1 : -1;           // the K-step whose k past K are zeroed in registers

    // the chunks this thread stages: chunk c = i * 256 + tid of an image [half][row][g], so g = tid & 3 and the rows are
    // 64 q + (tid >> 2); half h of the chunk begins at k 64 h + 16 g of the K-step
    const int cg = tid & 3, crow = tid >> 2;
    const uint8_t *x_src[XQ], *w_src[WQ];
#pragma unroll
    for (int q = 0; q < XQ; ++q) x_src[q] = m0 + 64 * q + crow < M ? A + (m0 + 64 * q + crow) * K + 16 * cg : nullptr;
#pragma unroll
    for (int q = 0; q < WQ; ++q) w_src[q] = n0 + 64 * q + crow < N ? W + (n0 + 64 * q + crow) * K + 16 * cg : nullptr;
    auto stage = [&](int s, int64_t k0) {
        uint8_t *dst = smem + s * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int h = i / XQ, q = i % XQ;
            const uint8_t *p = x_src[q] && k0 + 64 * h + 16 * cg < K ? x_src[q] + k0 + 64 * h : A;
            lds_dma16(p, dst + i * 4096);
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int h = i / WQ, q = i % WQ;
            const uint8_t *p = w_src[q] && k0 + 64 * h + 16 * cg < K ? w_src[q] + k0 + 64 * h : W;
            lds_dma16(p, dst + X_BYTES + i * 4096);
        }
    };

    // fragment reads: operand row `row0 + fr` of an image of `rows` rows at `img`, K-step `step`
    const int frag_off = (fr * 4 + g) * 16;
    auto read_frag = [&](const uint8_t *img, int rows, int row0, int step) {
        const i32x4 lo = *(const i32x4 *)(img + row0 * 64 + frag_off);
        const i32x4 hi = *(const i32x4 *)(img + rows * 64 + row0 * 64 + frag_off);
        i32x8 f = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if (step == last_partial) {                          // the k past K count as zeros
            const int64_t k0 = (int64_t)step * KS;
            if (k0 + 16 * g >= K) f[0] = f[1] = f[2] = f[3] = 0;
            if (k0 + 64 + 16 * g >= K) f[4] = f[5] = f[6] = f[7] = 0;
        }
        return f;
    };
    i32x8 wf[NI], xf[NJ];
    auto read_w = [&](int i, int step) { wf[i] = read_frag(smem + (step & 1) * STAGE + X_BYTES, TN, wn * (TN / 2) + 16 * i, step); };
    auto read_x = [&](int j, int step) { xf[j] = read_frag(smem + (step & 1) * STAGE, TM, wm * (TM / 2) + 16 * j, step); };

    // the scales: row j of this lane's activation fragments (clamped to M - 1), and this workgroup's block row of sW
    const float *sa_row[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t m = m0 + wm * (TM / 2) + 16 * j + fr;
        sa_row[j] = sA + (m < M ? m : M - 1) * nk;
    }
    const float *sw_row = sW + (n0 / kBlock) * nk;
    float sa_next[NJ];                                       // sA of the K-step whose products are formed next
    f32x4 sp = f32x4{0.0f, 0.0f, 0.0f, 0.0f};                // the products in use, one per activation fragment: ONE register tuple,
    static_assert(NJ == 4, "sp");                            // so that a packed fma that reads a pair of them never touches a load's target
    float sw_next = sw_row[0];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sa_next[j] = sa_row[j][0];

    f32x4 acc[NI][NJ], part[2][NJ];                          // the running sums; the partials of MFMA rows i & 1
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        part[(NI - 1) & 1][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};   // "the last row of K-step -1": folded with sp = 0 into +0
    }
    const int one = 127;                                     // both scale bytes: 2^0

    __builtin_amdgcn_sched_barrier(0);                       // the loads of sA(0) stand in front of the DMA: the count below
    stage(0, 0);
    stage(1, KS);
    __builtin_amdgcn_s_waitcnt(vmcnt_only(NPS));             // sA(0) and K-step 0 have landed; DMA(1), NPS instructions, is in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NI; ++i) read_w(i, 0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) read_x(j, 0);

    constexpr int R1 = 1, R2 = 2;                            // B1 behind MFMA row R1 - 1, B2 behind row R2 - 1
    for (int t = 0; t < nk; ++t) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i == R1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the fragment reads of t (and sW(t)): nothing of LDS in flight
                __builtin_amdgcn_s_barrier();                // B1: stage t & 1 is free
                asm volatile("" ::: "memory");
                __builtin_amdgcn_s_waitcnt(vmcnt_only(NPS)); // sA(t) has landed; DMA(t + 1), NPS instructions, is in flight
                const int tn = t + 1 < nk ? t + 1 : nk - 1;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    asm volatile("" : "+v"(sa_next[j]));     // (no instruction: the product stands behind the wait above)
                    sp[j] = sa_next[j] * sw_next;            // one f32 rounding; the folds of K-step t - 1 stand in front of B1
                }
                asm volatile("" : "+v"(sp));                 // (no instruction: the products are formed HERE, in front of the loads)
#pragma unroll
                for (int j = 0; j < NJ; ++j) sa_next[j] = sa_row[j][tn];   // NJ vector-memory loads, IN FRONT of the DMA below
                sw_next = sw_row[tn];                        // uniform: a scalar load
                __builtin_amdgcn_sched_barrier(0);
                stage(t & 1, (int64_t)(t + 2) * KS);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (i == R2) {
                // DMA(t + 1) has landed; behind it sA(t + 1), NJ loads, and DMA(t + 2), NPS instructions, stay in flight
                __builtin_amdgcn_s_waitcnt(vmcnt_only(NPS + NJ));
                __builtin_amdgcn_s_barrier();                // B2: K-step t + 1 is in LDS
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 0; d < R2; ++d) read_w(d, t + 1);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %3 op_sel_hi:[0,0,0]"
                             : "=&v"(part[i & 1][j])
                             : "v"(wf[i]), "v"(xf[j]), "v"(one));
                // the fold of the MFMA NJ back: row i - 1 of this K-step, or (i == 0) the last row of the K-step before.  The two
                // statements without an instruction pin it between this MFMA and the next: the partial passes through the first,
                // the sum through the second
                {
                    f32x4 &c = acc[(i + NI - 1) % NI][j], &p = part[(i + 1) & 1][j];
                    asm volatile("" : "+v"(p));
#pragma unroll
                    for (int r = 0; r < 4; ++r) c[r] = fmaf(p[r], sp[j], c[r]);
                    asm volatile("" : "+v"(c));
                }
                // a fragment's registers are loaded again right behind the MFMA that reads them (k_gemm_fp8's reasoning)
                if (i == NI - 1) read_x(j, t + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (i >= R2) read_w(i, t + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the two K-steps past the end are still landing in LDS; nothing reads them, the workgroup must not end under them.  The
    // nops also keep the VALU off the last MFMAs' results: the partials pass through the statement, so no fold moves above it
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15"
                 : "+v"(part[(NI - 1) & 1][0]), "+v"(part[(NI - 1) & 1][1]), "+v"(part[(NI - 1) & 1][2]), "+v"(part[(NI - 1) & 1][3])
                 :
                 : "memory");
    static_assert(NJ == 4, "the operands of the statement above");
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[NI - 1][j][r] = fmaf(part[(NI - 1) & 1][j][r], sp[j], acc[NI - 1][j][r]);

    // epilogue: acc + bias[n] in f32, one rounding to TO; bias read once per lane
    const bool vec = N % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (4 * sizeof(TO) - 1)) == 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int64_t n = n0 + wn * (TN / 2) + 16 * i + 4 * g;
        float b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) b[r] = bias ? bias_at(bias, bias_dtype, n + r < N ? n + r : N - 1) : 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t m = m0 + wm * (TM / 2) + 16 * j + fr;
            TO v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float f = acc[i][j][r];
                if (bias) f = f + b[r];
                v[r] = (TO)f;
            }
            if (m >= M || n >= N) continue;
            TO *o = out + m * N + n;
            if (vec) {                                       // N % 4 == 0: the four columns are inside the row
                typedef TO tvec __attribute__((ext_vector_type(4)));
                *(tvec *)o = tvec{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < N) o[r] = v[r];
            }
        }
    }
#endif
}

// ---------------------------------------------------------------- host side
bool known_dtype(int d) { return d >= MBNB_FP8BLK_F16 && d <= MBNB_FP8BLK_F32; }
const char *dtype_name(int d) { return d == MBNB_FP8BLK_F16 ? "f16" : d == MBNB_FP8BLK_BF16 ? "bf16" : "f32"; }
int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// the checks every entry point shares, on the rows R (M or N) and K of one operand; 0 or the status
int check_shape(const char *what, const char *rows, int64_t R, int64_t K) {
    if (R < 0 || K <= 0) return fail(MBNB_FP8BLK_ERR_SHAPE, "%s: %s = %lld, K = %lld", what, rows, (long long)R, (long long)K);
    if (K % 16) return fail(MBNB_FP8BLK_ERR_SHAPE, "%s: K = %lld is not a multiple of 16", what, (long long)K);
    if (R > INT32_MAX || (R > 0 && R > mbnb::kMaxElems / K))
        return fail(MBNB_FP8BLK_ERR_SHAPE, "%s: %lld x %lld elements exceed one launch", what, (long long)R, (long long)K);
    return 0;
}

int64_t tiles_of(int64_t M, int64_t N) { return ((M + TM - 1) / TM) * ((N + TN - 1) / TN); }

int check_gemm(const char *what, int64_t M, int64_t K, int64_t N, const void *bias, int bias_dtype, int out_dtype) {
    if (!known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_FP8BLK_ERR_ARG, "%s: unknown dtype (bias %d, out %d)", what, bias_dtype, out_dtype);
    if (const int st = check_shape(what, "M", M, K)) return st;
    if (N <= 0 || N > INT32_MAX || N > mbnb::kMaxElems / K || (M > 0 && N > mbnb::kMaxElems / M))
        return fail(MBNB_FP8BLK_ERR_SHAPE, "%s: N = %lld", what, (long long)N);
    if (M > 0 && tiles_of(M, N) > INT32_MAX) return fail(MBNB_FP8BLK_ERR_SHAPE, "%s: %lld workgroups exceed one launch", what, (long long)tiles_of(M, N));
    return 0;
}

int check_gemm_pointers(const char *what, const void *w, const void *sW, const void *bias, int bias_dtype, const void *out, int out_dtype) {
    if (!w || !sW || !out) return fail(MBNB_FP8BLK_ERR_ARG, "%s: NULL w, sW or out", what);
    if (!mbnb::aligned(w, 16)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned w (16 bytes)", what);
    if (!mbnb::aligned(sW, 4) || !mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned sW, out or bias (the element size each)", what);
    return 0;
}

// the checks of a quantiser call on x [R, K]: 0, the status, or 1 for the empty call
int check_quantize(const char *what, const char *rows, const void *x, int x_dtype, int64_t R, int64_t K, const void *q, const void *s) {
    if (!known_dtype(x_dtype)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: unknown dtype %d", what, x_dtype);
    if (const int st = check_shape(what, rows, R, K)) return st;
    if (R == 0) return 1;
    if (!x || !q || !s) return fail(MBNB_FP8BLK_ERR_ARG, "%s: NULL input, q or scales", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(q, 16)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned input or q (16 bytes each)", what);
    if (!mbnb::aligned(s, 4)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned scales (4 bytes)", what);
    return 0;
}

int launch_quantize_groups(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, hipStream_t s) {
    const int64_t KB = blocks_of(K), grid = (M * KB + kThreads / 8 - 1) / (kThreads / 8);
    return mbnb::with_dtype(x_dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_fp8_quantize_groups<T>), dim3((unsigned)grid), dim3(kThreads), 0, s, (const T *)x, M, K, KB, (uint8_t *)q, (float *)sA);
        return mbnb::launch_status("k_fp8_quantize_groups");
    });
}

int launch_quantize_blocks(const void *w, int w_dtype, int64_t N, int64_t K, void *q, void *sW, hipStream_t s) {
    const int64_t KB = blocks_of(K), grid = blocks_of(N) * KB;
    return mbnb::with_dtype(w_dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_fp8_quantize_blocks<T>), dim3((unsigned)grid), dim3(kThreads), 0, s, (const T *)w, N, K, KB, (uint8_t *)q, (float *)sW);
        return mbnb::launch_status("k_fp8_quantize_blocks");
    });
}

// The dynamic-LDS limit of ALL three instantiations is raised by the first GEMM call on a device (the attribute belongs to the
// device's copy of a function), so which dtype a later call takes -- one inside a stream capture, say -- never decides whether
// hipFuncSetAttribute runs.  include/mbnb_fp8blk.h asks for that first call outside a capture.
template <typename TO> hipError_t raise_one() {
    return hipFuncSetAttribute((const void *)&k_gemm_fp8_block<TO>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
}
int raise_lds_limits() {
    constexpr int kDevices = 64;
    static std::atomic<bool> done[kDevices];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    const bool known = dev >= 0 && dev < kDevices;
    if (e == hipSuccess && known && done[dev].load(std::memory_order_acquire)) return 0;
    hipError_t (*const all[])() = {raise_one<f16_t>, raise_one<bf16_t>, raise_one<float>};
    for (auto raise : all)
        if (e == hipSuccess) e = raise();
    if (e != hipSuccess) return fail((int)e, "k_gemm_fp8_block: raising the dynamic LDS limit failed: %s", hipGetErrorString(e));
    if (known) done[dev].store(true, std::memory_order_release);
    return 0;
}

int launch_gemm(const void *a, const void *sA, const void *w, const void *sW, int64_t M, int64_t N, int64_t K, const void *bias, int bias_dtype,
                void *out, int out_dtype, hipStream_t s) {
    if (const int st = raise_lds_limits()) return st;
    const int64_t tiles_m = (M + TM - 1) / TM;
    return mbnb::with_dtype(out_dtype, [&](auto t) {
        using TO = decltype(t);
        hipLaunchKernelGGL((k_gemm_fp8_block<TO>), dim3((unsigned)tiles_of(M, N)), dim3(kThreads), LDS_BYTES, s, (const uint8_t *)a, (const float *)sA,
                           (const uint8_t *)w, (const float *)sW, M, N, K, bias, bias_dtype, (TO *)out, (int)tiles_m);
        return mbnb::launch_status("k_gemm_fp8_block");
    });
}

}  // namespace

extern "C" {

int mbnb_fp8blk_abi_version(void) { return MBNB_FP8BLK_ABI_VERSION; }

const char *mbnb_fp8blk_last_error(void) { return mbnb::last_error(); }

const char *mbnb_fp8blk_last_launch(void) { return mbnb::last_launch(); }

int mbnb_fp8blk_quantize_groups(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, void *stream) {
    const int c = check_quantize("mbnb_fp8blk_quantize_groups", "M", x, x_dtype, M, K, q, sA);
    if (c) return c < 0 ? c : 0;
    const int st = launch_quantize_groups(x, x_dtype, M, K, q, sA, (hipStream_t)stream);
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_quant_groups %s %lldx%lld", dtype_name(x_dtype), (long long)M, (long long)K);
    return st;
}

int mbnb_fp8blk_quantize_blocks(const void *w, int w_dtype, int64_t N, int64_t K, void *q, void *sW, void *stream) {
    const int c = check_quantize("mbnb_fp8blk_quantize_blocks", "N", w, w_dtype, N, K, q, sW);
    if (c) return c < 0 ? c : 0;
    const int st = launch_quantize_blocks(w, w_dtype, N, K, q, sW, (hipStream_t)stream);
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_quant_blocks %s %lldx%lld", dtype_name(w_dtype), (long long)N, (long long)K);
    return st;
}

int mbnb_fp8blk_matmul(const void *a, const void *sA, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias,
                       int bias_dtype, void *out, int out_dtype, void *stream) {
    const char *what = "mbnb_fp8blk_matmul";
    if (const int st = check_gemm(what, M, K, N, bias, bias_dtype, out_dtype)) return st;
    if (M == 0) return 0;
    if (!a || !sA) return fail(MBNB_FP8BLK_ERR_ARG, "%s: NULL a or sA", what);
    if (!mbnb::aligned(a, 16)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned a (16 bytes)", what);
    if (!mbnb::aligned(sA, 4)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned sA (4 bytes)", what);
    if (const int st = check_gemm_pointers(what, w, sW, bias, bias_dtype, out, out_dtype)) return st;
    const int st = launch_gemm(a, sA, w, sW, M, N, K, bias, bias_dtype, out, out_dtype, (hipStream_t)stream);
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "gemm_fp8_block %dx%d %lldx%lldx%lld", TM, TN, (long long)M, (long long)N, (long long)K);
    return st;
}

int64_t mbnb_fp8blk_workspace_bytes(int64_t M, int64_t K) {
    if (const int st = check_shape("mbnb_fp8blk_workspace_bytes", "M", M, K)) return st;
    return mbnb::round256(M * K) + mbnb::round256(M * blocks_of(K) * 4);
}

int mbnb_fp8blk_linear(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias,
                       int bias_dtype, void *out, int out_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "mbnb_fp8blk_linear";
    if (!known_dtype(x_dtype)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: unknown dtype %d", what, x_dtype);
    if (const int st = check_gemm(what, M, K, N, bias, bias_dtype, out_dtype)) return st;
    if (M == 0) return 0;
    if (!x) return fail(MBNB_FP8BLK_ERR_ARG, "%s: NULL x", what);
    if (!mbnb::aligned(x, 16)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned x (16 bytes)", what);
    if (const int st = check_gemm_pointers(what, w, sW, bias, bias_dtype, out, out_dtype)) return st;
    const int64_t cbytes = mbnb::round256(M * K), need = cbytes + mbnb::round256(M * blocks_of(K) * 4);
    if (!workspace || workspace_bytes < need)
        return fail(MBNB_FP8BLK_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", what, (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!mbnb::aligned(workspace, 16)) return fail(MBNB_FP8BLK_ERR_ARG, "%s: misaligned workspace (16 bytes)", what);
    uint8_t *q = (uint8_t *)workspace;
    float *sA = (float *)(q + cbytes);
    hipStream_t s = (hipStream_t)stream;
    if (const int st = launch_quantize_groups(x, x_dtype, M, K, q, sA, s)) return st;
    const int st = launch_gemm(q, sA, w, sW, M, N, K, bias, bias_dtype, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_quant_groups %s + gemm_fp8_block %dx%d %lldx%lldx%lld", dtype_name(x_dtype), TM, TN,
                 (long long)M, (long long)N, (long long)K);
    return st;
}

}  // extern "C"
