// fp8_kernels.hip — the W8A8 FP8 linear: a row quantiser to OCP E4M3 and a GEMM over two E4M3 operands on gfx950's FP8 MFMA,
// and the C ABI of libmbnb_fp8.so (include/mbnb_fp8.h; the semantics, the design and the figures: DESIGN.md §37).
//
//   k_fp8_quantize_rows  x [M, K] of f16 / bf16 / f32 -> codes uint8 [M, K] and one f32 scale per row.  One workgroup per row, a
//                        thread owns chunks of 16 elements: the first 4096 k of a row stay in registers between the maximum and
//                        the encoding, the rest is read a second time.  The maximum is taken over the |bits| as unsigned integers.
//   k_gemm_fp8           out[M, N] = ((A . W^T) * sA[m]) * sW[n] + bias[n] over the codes of both operands as they lie in
//                        memory: v_mfma_scale_f32_16x16x128_f8f6f4 with both scale bytes 127.  256 x 256 (or 256 x 128)
//                        output tile, four waves of 128 x 128 (128 x 64), K-step 128, two LDS stages filled by 16-byte LDS-DMA
//                        with two K-steps in flight, the fragments of a whole K-step in registers (see the kernel).
#include "../../include/mbnb_fp8.h"
#include "host.h"

#include <atomic>

static_assert(MBNB_FP8_F16 == mbnb::kF16 && MBNB_FP8_BF16 == mbnb::kBF16 && MBNB_FP8_F32 == mbnb::kF32, "host.h's dtype codes");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;              // every launch: 4 waves
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// ---------------------------------------------------------------- the row quantiser
// The operation chain of mx_scaled.h's enc_e4m3, restated (a host test closes that header's includers): the bits of |a| -> E4M3
// code 0..0x7E, round to nearest even, saturating at 448 (an Inf saturates with it)
__device__ __forceinline__ uint32_t fp8_enc_e4m3(uint32_t a) {
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
            w[j >> 2] |= (int)((fp8_enc_e4m3(a) | ((__float_as_uint(v[j]) >> 24) & 0x80u)) << (8 * (j & 3)));   // the sign of x
        }
    }
    *(i32x4 *)q = w;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp8_quantize_rows(const T *__restrict__ x, int64_t K, uint8_t *__restrict__ q,
                                                                float *__restrict__ sA) {
    __shared__ uint32_t wave_max[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t chunks = K / 16;
    const T *row = x + (int64_t)blockIdx.x * K;
    uint8_t *qrow = q + (int64_t)blockIdx.x * K;

    float held[16];                                          // chunk tid of the row, kept for the second pass
    uint32_t m = 0;
    if (tid < chunks) {
        load16<T>(row + (int64_t)tid * 16, held);
        m = max_abs_bits(held, 0);
    }
    for (int64_t c = tid + kThreads; c < chunks; c += kThreads) {
        float v[16];
        load16<T>(row + c * 16, v);
        m = max_abs_bits(v, m);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if ((tid & 63) == 0) wave_max[tid >> 6] = m;
    __syncthreads();
    m = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));

    const bool live = m != 0u && m < 0x7F800000u;            // not an all-zero row, no Inf or NaN in it
    const float amax = __uint_as_float(m);
    const float r = 448.0f / amax;
    if (tid == 0) sA[blockIdx.x] = m >= 0x7F800000u ? __uint_as_float(kQuietNaN) : amax / 448.0f;
    if (tid < chunks) store_codes(qrow + (int64_t)tid * 16, held, r, live);
    for (int64_t c = tid + kThreads; c < chunks; c += kThreads) {
        float v[16];
        if (live) load16<T>(row + c * 16, v);
        store_codes(qrow + c * 16, v, r, live);
    }
}

// ---------------------------------------------------------------- the GEMM
// One workgroup = four waves = one 256 x TN output tile (TN 256, or 128 where the wide grid would not fill the chip); wave
// (wm = w & 1, wn = w >> 1) owns rows 128 wm .. + 128 and columns (TN / 2) wn .. + TN / 2 as 8 x (TN / 32) accumulators of 16 x 16.
//
// The instruction (lane map: DESIGN.md §25): lane l = (g = l >> 4, fr = l & 15) holds row fr of its operand, registers 0..3 the
// 16 k from 16 g, registers 4..7 the 16 k from 64 + 16 g; D: column fr, rows 4 g + r.  The WEIGHT is the first operand and the
// activation the second, so a lane's four sums are four consecutive n of one output row: one 8- or 16-byte store.
//
// LDS: two stages of a K-step (128 k), each the activation tile then the weight tile, both in §25's chunk order
// [half][row][g] (16-byte chunk [h][row][g] = the 16 k from 64 h + 16 g of that row): a wave's fragment read -- lane l takes chunk
// [h][row0 + fr][g] -- is 1 KiB of consecutive LDS, and a wave's LDS-DMA instruction, which writes 64 consecutive chunks,
// reads 16 rows x 64 bytes of the operand.
//
// The pipeline.  The fragments of a WHOLE K-step live in registers (8 + TN / 32 fragments of 8 registers), so a stage is free
// again as soon as every wave has read it, a K-step before its MFMAs end:
//
//   K-step t:   MFMA row 0
//               lgkmcnt(0), barrier B1       every wave holds the fragments of t: stage t & 1 is free
//               LDS-DMA of K-step t + 2  ->  stage t & 1        (NPS instructions per wave; t + 1 is still in flight: two K-steps)
//               MFMA rows 1, 2
//               vmcnt(NPS), barrier B2       the DMA of t + 1 has landed for every wave, that of t + 2 stays in flight
//               fragment reads of t + 1 from stage (t + 1) & 1, each into the registers of an MFMA row that is done:
//               the weight fragments 0..2 now, fragment i behind MFMA row i, the activation fragments inside the last row
//
// One MFMA row = one weight fragment against the 8 activation fragments.  The MFMAs are issued from assembly with the accumulator
// pinned to its AGPR tuple, as in gemm_i8_inplace.h: 256 (128) accumulator registers do not survive the allocator otherwise.
//
// Edges (k_gemm_mx's rules): chunks of rows past M / N and of k past K are fetched from the operand's first 16 bytes, so every
// K-step issues the same NPS instructions and the vmcnt count holds, the two K-steps past the end included; on the last step of
// a K % 128 != 0 problem the k past K are zeroed in registers in both operands; rows and columns past the edge are never
// stored; row and byte offsets are 64-bit.
constexpr int TM = MBNB_FP8_TILE_M, KS = MBNB_FP8_K_STEP;
static_assert(TM == 256 && KS == 128 && MBNB_FP8_STEPS_IN_FLIGHT == 2, "the wave grid, the chunk maps and the waits below");

template <int TN> struct Fp8Tile {
    static constexpr int X_BYTES = TM * KS, W_BYTES = TN * KS, STAGE = X_BYTES + W_BYTES, LDS = 2 * STAGE;
    static constexpr int NX = X_BYTES / 16 / kThreads, NW = W_BYTES / 16 / kThreads, NPS = NX + NW;   // LDS-DMA instructions per thread and stage
    static constexpr int NI = TN / 32, NJ = TM / 32;         // weight / activation fragments of a wave
    static constexpr int XQ = NX / 2, WQ = NW / 2;           // row groups of 64 per half of an image
};

__device__ __forceinline__ void lds_dma16(const uint8_t *src, uint8_t *wave_dst) {   // 64 lanes x 16 bytes, lane l to wave_dst + 16 l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)wave_dst, 16, 0,
                                     0);
}

// s_waitcnt vmcnt(n) alone, the other counters left at their maxima (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
constexpr int vmcnt_only(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

__device__ __forceinline__ float bias_at(const void *bias, int dtype, int64_t n) {
    return dtype == mbnb::kF32 ? ((const float *)bias)[n] : dtype == mbnb::kBF16 ? (float)((const bf16_t *)bias)[n] : (float)((const f16_t *)bias)[n];
}

template <int TN, typename TO>
__global__ __launch_bounds__(kThreads, 1) void k_gemm_fp8(const uint8_t *__restrict__ A, const float *__restrict__ sA,
                                                          const uint8_t *__restrict__ W, const float *__restrict__ sW, int64_t M, int64_t N,
                                                          int64_t K, const void *__restrict__ bias, int bias_dtype, TO *__restrict__ out,
                                                          int tiles_m) {
#if defined(__HIP_DEVICE_COMPILE__)                           // the host pass keeps the stub alone: the assembly below is gfx950's
    using T = Fp8Tile<TN>;
    constexpr int X_BYTES = T::X_BYTES, STAGE = T::STAGE, NI = T::NI, NJ = T::NJ;
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)(blockIdx.x % tiles_m) * TM, n0 = (int64_t)(blockIdx.x / tiles_m) * TN;
    const int nk = (int)((K + KS - 1) / KS);
    const int last_partial = K % KS ? nk - 1 : -1;           // the K-step whose k past K are zeroed in registers

    // the chunks this thread stages: chunk c = i * 256 + tid of an image [half][row][g], so g = tid & 3 and the rows are
    // 64 q + (tid >> 2); half h of the chunk begins at k 64 h + 16 g of the K-step
    const int cg = tid & 3, crow = tid >> 2;
    const uint8_t *x_src[T::XQ], *w_src[T::WQ];
#pragma unroll
    for (int q = 0; q < T::XQ; ++q) x_src[q] = m0 + 64 * q + crow < M ? A + (m0 + 64 * q + crow) * K + 16 * cg : nullptr;
#pragma unroll
    for (int q = 0; q < T::WQ; ++q) w_src[q] = n0 + 64 * q + crow < N ? W + (n0 + 64 * q + crow) * K + 16 * cg : nullptr;
    auto stage = [&](int s, int64_t k0) {
        uint8_t *dst = smem + s * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < T::NX; ++i) {
            const int h = i / T::XQ, q = i % T::XQ;
            const uint8_t *p = x_src[q] && k0 + 64 * h + 16 * cg < K ? x_src[q] + k0 + 64 * h : A;
            lds_dma16(p, dst + i * 4096);
        }
#pragma unroll
        for (int i = 0; i < T::NW; ++i) {
            const int h = i / T::WQ, q = i % T::WQ;
            const uint8_t *p = w_src[q] && k0 + 64 * h + 16 * cg < K ? w_src[q] + k0 + 64 * h : W;
            lds_dma16(p, dst + X_BYTES + i * 4096);
        }
    };

    // fragment reads: operand row `row` of an image of ROWS rows at `img`, K-step `step`
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
    auto read_x = [&](int j, int step) { xf[j] = read_frag(smem + (step & 1) * STAGE, TM, wm * 128 + 16 * j, step); };

    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int one = 127;                                     // both scale bytes: 2^0

    stage(0, 0);
    stage(1, KS);
    __builtin_amdgcn_s_waitcnt(vmcnt_only(T::NPS));          // K-step 0 has landed, K-step 1 is in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NI; ++i) read_w(i, 0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) read_x(j, 0);

    constexpr int R1 = 1, R2 = NI > 4 ? 3 : 2;               // B1 behind MFMA row R1 - 1, B2 behind row R2 - 1
    for (int t = 0; t < nk; ++t) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i == R1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                // B1: stage t & 1 is free
                asm volatile("" ::: "memory");
                stage(t & 1, (int64_t)(t + 2) * KS);
            }
            if (i == R2) {
                __builtin_amdgcn_s_waitcnt(vmcnt_only(T::NPS));
                __builtin_amdgcn_s_barrier();                // B2: K-step t + 1 is in LDS
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 0; d < R2; ++d) read_w(d, t + 1);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %3 op_sel_hi:[0,0,0]"
                             : "+a"(acc[i][j])
                             : "v"(wf[i]), "v"(xf[j]), "v"(one));
                // a fragment's registers are loaded again right behind the MFMA that reads them, and no s_nop stands between: the
                // instruction reads SrcA / SrcB in its first passes, and the ds_read's data is an LDS latency (64 cycles and more) away
                if (i == NI - 1) read_x(j, t + 1);
            }
            if (i >= R2) read_w(i, t + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the two K-steps past the end are still landing in LDS; nothing reads them, the workgroup must not end under them
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");

    // epilogue: ((acc * sA[m]) * sW[n]) + bias[n], each one f32 rounding, one rounding to TO; sA / sW / bias read once per lane
    float sa[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t m = m0 + wm * 128 + 16 * j + fr;
        sa[j] = sA[m < M ? m : M - 1];
    }
    const bool vec = N % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (4 * sizeof(TO) - 1)) == 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int64_t n = n0 + wn * (TN / 2) + 16 * i + 4 * g;
        float sw[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t nr = n + r < N ? n + r : N - 1;
            sw[r] = sW[nr];
            b[r] = bias ? bias_at(bias, bias_dtype, nr) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t m = m0 + wm * 128 + 16 * j + fr;
            f32x4 a;
#pragma unroll
            for (int r = 0; r < 4; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(a[r]) : "a"(acc[i][j][r]));
            TO v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float f = (a[r] * sa[j]) * sw[r];
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
bool known_dtype(int d) { return d >= MBNB_FP8_F16 && d <= MBNB_FP8_F32; }
const char *dtype_name(int d) { return d == MBNB_FP8_F16 ? "f16" : d == MBNB_FP8_BF16 ? "bf16" : "f32"; }

// the checks every entry point shares; 0 or the status
int check_shape(const char *what, int64_t M, int64_t K) {
    if (M < 0 || K <= 0) return fail(MBNB_FP8_ERR_SHAPE, "%s: M = %lld, K = %lld", what, (long long)M, (long long)K);
    if (K % 16) return fail(MBNB_FP8_ERR_SHAPE, "%s: K = %lld is not a multiple of 16", what, (long long)K);
    if (M > INT32_MAX || (M > 0 && M > mbnb::kMaxElems / K))
        return fail(MBNB_FP8_ERR_SHAPE, "%s: %lld x %lld elements exceed one launch", what, (long long)M, (long long)K);
    return 0;
}

// the 256 x 256 tile from one tile per compute unit up, the 256 x 128 tile below
int tile_n(int64_t M, int64_t N) {
    const int64_t wide = ((M + TM - 1) / TM) * ((N + MBNB_FP8_TILE_N - 1) / MBNB_FP8_TILE_N);
    return wide >= MBNB_FP8_WIDE_TILES ? MBNB_FP8_TILE_N : MBNB_FP8_TILE_N_NARROW;
}
int64_t tiles_of(int64_t M, int64_t N, int tn) { return ((M + TM - 1) / TM) * ((N + tn - 1) / tn); }

int check_gemm(const char *what, int64_t M, int64_t K, int64_t N, const void *bias, int bias_dtype, int out_dtype) {
    if (!known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_FP8_ERR_ARG, "%s: unknown dtype (bias %d, out %d)", what, bias_dtype, out_dtype);
    if (const int st = check_shape(what, M, K)) return st;
    if (N <= 0 || N > mbnb::kMaxElems / K || (M > 0 && N > mbnb::kMaxElems / M)) return fail(MBNB_FP8_ERR_SHAPE, "%s: N = %lld", what, (long long)N);
    if (M > 0 && tiles_of(M, N, tile_n(M, N)) > INT32_MAX)
        return fail(MBNB_FP8_ERR_SHAPE, "%s: %lld workgroups exceed one launch", what, (long long)tiles_of(M, N, tile_n(M, N)));
    return 0;
}

int check_gemm_pointers(const char *what, const void *w, const void *sW, const void *bias, int bias_dtype, const void *out, int out_dtype) {
    if (!w || !sW || !out) return fail(MBNB_FP8_ERR_ARG, "%s: NULL w, sW or out", what);
    if (!mbnb::aligned(w, 16)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned w (16 bytes)", what);
    if (!mbnb::aligned(sW, 4) || !mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_FP8_ERR_ARG, "%s: misaligned sW, out or bias (the element size each)", what);
    return 0;
}

int launch_quantize(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, hipStream_t s) {
    return mbnb::with_dtype(x_dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_fp8_quantize_rows<T>), dim3((unsigned)M), dim3(kThreads), 0, s, (const T *)x, K, (uint8_t *)q, (float *)sA);
        return mbnb::launch_status("k_fp8_quantize_rows");
    });
}

template <int TN, typename TO>
int launch_gemm_tile(const void *a, const void *sA, const void *w, const void *sW, int64_t M, int64_t N, int64_t K, const void *bias,
                     int bias_dtype, void *out, hipStream_t s) {
    const int64_t tiles_m = (M + TM - 1) / TM;
    hipLaunchKernelGGL((k_gemm_fp8<TN, TO>), dim3((unsigned)tiles_of(M, N, TN)), dim3(kThreads), Fp8Tile<TN>::LDS, s, (const uint8_t *)a,
                       (const float *)sA, (const uint8_t *)w, (const float *)sW, M, N, K, bias, bias_dtype, (TO *)out, (int)tiles_m);
    return mbnb::launch_status("k_gemm_fp8");
}

// The dynamic-LDS limit of ALL six instantiations is raised by the first GEMM call on a device (the attribute belongs to the
// device's copy of a function), so which tile and dtype a later call takes -- one inside a stream capture, say -- never decides
// whether hipFuncSetAttribute runs.  include/mbnb_fp8.h asks for that first call outside a capture.
template <int TN, typename TO> hipError_t raise_one() {
    return hipFuncSetAttribute((const void *)&k_gemm_fp8<TN, TO>, hipFuncAttributeMaxDynamicSharedMemorySize, Fp8Tile<TN>::LDS);
}
int raise_lds_limits() {
    constexpr int kDevices = 64;
    static std::atomic<bool> done[kDevices];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    const bool known = dev >= 0 && dev < kDevices;
    if (e == hipSuccess && known && done[dev].load(std::memory_order_acquire)) return 0;
    hipError_t (*const all[])() = {raise_one<MBNB_FP8_TILE_N, f16_t>,        raise_one<MBNB_FP8_TILE_N, bf16_t>,        raise_one<MBNB_FP8_TILE_N, float>,
                                   raise_one<MBNB_FP8_TILE_N_NARROW, f16_t>, raise_one<MBNB_FP8_TILE_N_NARROW, bf16_t>, raise_one<MBNB_FP8_TILE_N_NARROW, float>};
    for (auto raise : all)
        if (e == hipSuccess) e = raise();
    if (e != hipSuccess) return fail((int)e, "k_gemm_fp8: raising the dynamic LDS limit failed: %s", hipGetErrorString(e));
    if (known) done[dev].store(true, std::memory_order_release);
    return 0;
}

int launch_gemm(const void *a, const void *sA, const void *w, const void *sW, int64_t M, int64_t N, int64_t K, const void *bias, int bias_dtype,
                void *out, int out_dtype, hipStream_t s) {
    if (const int st = raise_lds_limits()) return st;
    const bool wide = tile_n(M, N) == MBNB_FP8_TILE_N;
    return mbnb::with_dtype(out_dtype, [&](auto t) {
        using TO = decltype(t);
        return wide ? launch_gemm_tile<MBNB_FP8_TILE_N, TO>(a, sA, w, sW, M, N, K, bias, bias_dtype, out, s)
                    : launch_gemm_tile<MBNB_FP8_TILE_N_NARROW, TO>(a, sA, w, sW, M, N, K, bias, bias_dtype, out, s);
    });
}

}  // namespace

extern "C" {

int mbnb_fp8_abi_version(void) { return MBNB_FP8_ABI_VERSION; }

const char *mbnb_fp8_last_error(void) { return mbnb::last_error(); }

const char *mbnb_fp8_last_launch(void) { return mbnb::last_launch(); }

int mbnb_fp8_quantize_rows(const void *x, int x_dtype, int64_t M, int64_t K, void *q, void *sA, void *stream) {
    const char *what = "mbnb_fp8_quantize_rows";
    if (!known_dtype(x_dtype)) return fail(MBNB_FP8_ERR_ARG, "%s: unknown dtype %d", what, x_dtype);
    if (const int st = check_shape(what, M, K)) return st;
    if (M == 0) return 0;
    if (!x || !q || !sA) return fail(MBNB_FP8_ERR_ARG, "%s: NULL x, q or sA", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(q, 16)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned x or q (16 bytes each)", what);
    if (!mbnb::aligned(sA, 4)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned sA (4 bytes)", what);
    const int st = launch_quantize(x, x_dtype, M, K, q, sA, (hipStream_t)stream);
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_quant_rows %s %lldx%lld", dtype_name(x_dtype), (long long)M, (long long)K);
    return st;
}

int mbnb_fp8_matmul(const void *a, const void *sA, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias,
                    int bias_dtype, void *out, int out_dtype, void *stream) {
    const char *what = "mbnb_fp8_matmul";
    if (const int st = check_gemm(what, M, K, N, bias, bias_dtype, out_dtype)) return st;
    if (M == 0) return 0;
    if (!a || !sA) return fail(MBNB_FP8_ERR_ARG, "%s: NULL a or sA", what);
    if (!mbnb::aligned(a, 16)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned a (16 bytes)", what);
    if (!mbnb::aligned(sA, 4)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned sA (4 bytes)", what);
    if (const int st = check_gemm_pointers(what, w, sW, bias, bias_dtype, out, out_dtype)) return st;
    const int st = launch_gemm(a, sA, w, sW, M, N, K, bias, bias_dtype, out, out_dtype, (hipStream_t)stream);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "gemm_fp8 %dx%d %lldx%lldx%lld", TM, tile_n(M, N), (long long)M, (long long)N, (long long)K);
    return st;
}

int64_t mbnb_fp8_workspace_bytes(int64_t M, int64_t K) {
    if (const int st = check_shape("mbnb_fp8_workspace_bytes", M, K)) return st;
    return mbnb::round256(M * K) + mbnb::round256(M * 4);
}

int mbnb_fp8_linear(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias,
                    int bias_dtype, void *out, int out_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "mbnb_fp8_linear";
    if (!known_dtype(x_dtype)) return fail(MBNB_FP8_ERR_ARG, "%s: unknown dtype %d", what, x_dtype);
    if (const int st = check_gemm(what, M, K, N, bias, bias_dtype, out_dtype)) return st;
    if (M == 0) return 0;
    if (!x) return fail(MBNB_FP8_ERR_ARG, "%s: NULL x", what);
    if (!mbnb::aligned(x, 16)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned x (16 bytes)", what);
    if (const int st = check_gemm_pointers(what, w, sW, bias, bias_dtype, out, out_dtype)) return st;
    const int64_t cbytes = mbnb::round256(M * K), need = cbytes + mbnb::round256(M * 4);
    if (!workspace || workspace_bytes < need)
        return fail(MBNB_FP8_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", what, (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!mbnb::aligned(workspace, 16)) return fail(MBNB_FP8_ERR_ARG, "%s: misaligned workspace (16 bytes)", what);
    uint8_t *q = (uint8_t *)workspace;
    float *sA = (float *)(q + cbytes);
    hipStream_t s = (hipStream_t)stream;
    if (const int st = launch_quantize(x, x_dtype, M, K, q, sA, s)) return st;
    const int st = launch_gemm(q, sA, w, sW, M, N, K, bias, bias_dtype, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_quant_rows %s + gemm_fp8 %dx%d %lldx%lldx%lld", dtype_name(x_dtype), TM, tile_n(M, N),
                 (long long)M, (long long)N, (long long)K);
    return st;
}

}  // extern "C"
