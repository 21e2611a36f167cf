// fp8dec_kernels.hip — the weight-only decode linear over a block-scaled FP8 weight (E4M3 codes [N, K], one f32 scale per 128 x 128
// block): ONE launch for the 1 to 16 activation rows of a token-generation step, no quantiser, no workspace, the activation left
// in its own dtype, the weight streamed once and decoded in registers; and the C ABI of libmbnb_fp8dec.so
// (include/mbnb_fp8dec.h; the semantics, the design and the figures: DESIGN.md §39).
//
//   k_fp8_block_decode_mfma  16-bit x, 2 rows and more, on v_mfma_f32_16x16x32_{bf16,f16}.  A workgroup of eight waves owns 16
//                            weight rows and ALL of K against 16 activation rows; the waves take the 128-k scale blocks round-robin
//                            and their accumulators are added through LDS in wave order.
//   k_fp8_block_decode       one 16-bit row, and every f32 call: a wave owns 2 or 4 weight rows and all of K against 1 / 2 / 4
//                            activation rows, a lane 16 bytes of a weight row per pass of 1024 k; FMAs, then a DPP sum over the wave.
//
// Both fold a block's partial sum into the running sum with the block's scale, acc = fmaf(p, sW[n / 128, t], acc): the order inside
// a block and over the blocks is free (mbnb_fp8dec.h), which is what lets either kernel give a lane the bytes that are cheapest to load.
#include "../../include/mbnb_fp8dec.h"
#include "host.h"

static_assert(MBNB_FP8DEC_F16 == mbnb::kF16 && MBNB_FP8DEC_BF16 == mbnb::kBF16 && MBNB_FP8DEC_F32 == mbnb::kF32, "host.h's dtype codes");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef f16_t f16x2 __attribute__((ext_vector_type(2)));
typedef f16_t f16x8 __attribute__((ext_vector_type(8)));

constexpr int kBlock = MBNB_FP8DEC_BLOCK;  // the scale block's edge
constexpr int kRows = MBNB_FP8DEC_ROWS;    // weight rows, and activation rows, of an MFMA workgroup
static_assert(kBlock == 128 && kRows == 16 && kBlock % kRows == 0, "a workgroup's rows lie in ONE block row of sW; the lane maps below");

// ---------------------------------------------------------------- what both kernels share
__device__ __forceinline__ float bias_at(const void *bias, int dtype, int64_t n) {
    return dtype == mbnb::kF32 ? ((const float *)bias)[n] : dtype == mbnb::kBF16 ? (float)((const bf16_t *)bias)[n] : (float)((const f16_t *)bias)[n];
}

// acc (+ bias) in f32, then ONE rounding to TO; the value passes through a statement without an instruction, so that the addition
// is never fused into the conversion
template <typename TO> __device__ __forceinline__ TO round_once(float acc, bool has_bias, float b) {
    float f = has_bias ? acc + b : acc;
    asm("" : "+v"(f));
    return (TO)f;
}

__device__ __forceinline__ bool on_bytes(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 16 bytes of the weight.  A plain load: a non-temporal one measured 4 to 7 % slower on every row count, and the
// row chunks of a tile read the weight again
__device__ __forceinline__ i32x4 load_w16(const uint8_t *p) { return *(const i32x4 *)p; }

// ---------------------------------------------------------------- k_fp8_block_decode_mfma
// Workgroup b: activation rows m0 = 16 (b % row_chunks) .. + 16 and weight rows n0 = 16 (b / row_chunks) .. + 16, so the chunks of
// one weight tile run next to each other and the tile comes from HBM once.  16 divides 128: the tile's rows lie in one block row
// nb = n0 / 128 of sW, and sW[nb, t] is one wave-uniform value per block, a scalar load.
//
// The k permutation.  v_mfma_f32_16x16x32 wants, on lane l = (fr = l & 15, g = l >> 4), the eight k 8 g .. 8 g + 7 of row fr of
// each operand: for the byte-wide weight that is 8 bytes per lane and 32-byte runs per row, a quarter of a 128-byte line per
// instruction, or a transpose across lanes behind a wider load.  The sum inside a block may run in ANY order, so the k are permuted
// instead of the data: lane (fr, g) loads the 32 CONSECUTIVE bytes [32 g, 32 g + 32) of block t of weight row n0 + fr as two 16-byte
// loads (a wave touches sixteen whole lines per block), and MFMA j = 0..3 of the block takes bytes 8 j .. 8 j + 7 of them: slot
// (g, i) of MFMA j is k = 128 t + 32 g + 8 j + i.  The other operand follows the same map: 16 bytes of x, elements
// 32 g + 8 j .. + 7 of block t of row m0 + fr, the four of them 64 consecutive bytes per lane.  No lane exchange anywhere.
//
// The WEIGHT is the first operand: D[i][j] is weight row i against activation row j, and lane (fr, g) holds D[4 g + r][fr],
// r = 0..3: four consecutive n of output row m0 + fr, one 8- or 16-byte store.
//
// Decode: v_cvt_scalef32_pk_{bf16,f16}_fp8 with the scale 1.0 turns two codes (a 16-bit half of a dword) into a packed pair: four
// instructions per MFMA operand, exact for every finite code (4 significand bits into 8 or 11; 2^-9, the smallest subnormal, is a
// normal number of both formats).
//
// The fold: the four MFMAs of a block accumulate into a fresh partial (C = 0 on the first), then acc[r] = fmaf(p[r], sW[nb, t],
// acc[r]): four fmaf per lane and block.  The compiler places the MFMAs, the wait states behind them and every s_waitcnt: the kernel
// is plain HIP C++ and builtins.
//
// Bytes in flight: a wave holds a ring of kMfmaDepth = 4 blocks, each 2 x 16 bytes of the weight and 4 x 16 bytes of x per lane,
// all requested before the first is used and each slot requested again as soon as it is consumed: 4 x 32 bytes x 512 lanes = 64 KiB
// of weight per workgroup on its way, against §27's 16 KiB.  Every load is unconditional and its address clamped (a chunk past K,
// a block past the last one: the row's first 16 bytes; a row past M or N: the last row), so the loads of a ring slot issue back to
// back; what a clamped load returned is zeroed in registers (a chunk past K inside the last block, both operands: 0 x Inf would
// be a NaN) or never used (a block past the last one: the wave-uniform branch around the MFMAs; rows past M and N: columns and rows
// of D that are not stored, and a column of D depends on that activation row alone).
// The order of the requests is left to the compiler, which does NOT keep three blocks ahead of every use: it requests three slots in
// a burst of 18 loads and uses slot 0 of each round behind vmcnt(6), one block in flight.  Pinning the ring order with
// sched_barriers (every use at vmcnt(18)) measured 6 to 11 % slower, so it is not pinned (DESIGN.md §39 lists every wait).
//
// Edges: nothing past N or M is stored; row and element offsets are 64-bit.
constexpr int kMfmaWaves = 8, kMfmaDepth = 4;
static_assert(kMfmaDepth * 32 >= 128, "at least 4 x 32 bytes of the weight per lane on their way");

template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ frag decode(int lo, int hi) {              // the eight codes of two dwords, in byte order
        const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
        const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
        return frag{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ f32x4 mma(frag w, frag x, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, c, 0, 0, 0); }
};
template <> struct Mfma<f16_t> {
    typedef f16x8 frag;
    static __device__ __forceinline__ frag decode(int lo, int hi) {
        const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
        const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
        return frag{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ f32x4 mma(frag w, frag x, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, x, c, 0, 0, 0); }
};

template <typename TO>
__device__ __forceinline__ void store_row4(TO *o, f32x4 acc, const float b[4], bool has_bias, int64_t n, int64_t N, bool vec) {
    TO v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = round_once<TO>(acc[r], has_bias, b[r]);
    if (vec) {                                               // N % 4 == 0 and an aligned base: the four columns are inside the row
        typedef TO tvec __attribute__((ext_vector_type(4)));
        *(tvec *)o = tvec{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n + r < N) o[r] = v[r];
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_fp8_block_decode_mfma(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                           const float *__restrict__ sW, int64_t M, int64_t N, int64_t K,
                                                                           const void *__restrict__ bias, int bias_dtype, void *__restrict__ out,
                                                                           int out_dtype, int row_chunks) {
#if defined(__HIP_DEVICE_COMPILE__)                           // the host pass keeps the stub alone: the builtins below are gfx950's
    static_assert(sizeof(T) == 2, "16 bytes of x are one MFMA operand");
    using MF = Mfma<T>;
    __shared__ f32x4 red[kMfmaWaves][64];

    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)(blockIdx.x % row_chunks) * kRows, n0 = (int64_t)(blockIdx.x / row_chunks) * kRows;
    const int KB = (int)((K + kBlock - 1) / kBlock);
    const int last_partial = K % kBlock ? KB - 1 : -1;       // the block whose chunks past K are zeroed in registers

    const uint8_t *w_row = W + (n0 + fr < N ? n0 + fr : N - 1) * K;
    const uint8_t *x_row = (const uint8_t *)(x + (m0 + fr < M ? m0 + fr : M - 1) * K);
    const float *s_row = sW + (n0 / kBlock) * KB;

    struct Step {
        i32x4 w[2], x[4];                                    // bytes 16 c .. + 15 of the lane's 32; elements 8 j .. + 7 of its 32
    };
    auto fetch = [&](int t) {
        Step s;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t k = (int64_t)t * kBlock + 32 * g + 16 * c, kc = k < K ? k : 0;
            s.w[c] = load_w16(w_row + kc);
            s.x[2 * c] = *(const i32x4 *)(x_row + kc * 2);
            s.x[2 * c + 1] = *(const i32x4 *)(x_row + kc * 2 + 16);
        }
        return s;
    };

    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    auto consume = [&](Step &s, int t) {
        if (t == last_partial) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if ((int64_t)t * kBlock + 32 * g + 16 * c >= K) s.w[c] = s.x[2 * c] = s.x[2 * c + 1] = i32x4{0, 0, 0, 0};
        }
        f32x4 p = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            p = MF::mma(MF::decode(s.w[j >> 1][2 * (j & 1)], s.w[j >> 1][2 * (j & 1) + 1]), __builtin_bit_cast(typename MF::frag, s.x[j]), p);
        const float scale = s_row[t];                        // uniform: a scalar load
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = fmaf(p[r], scale, acc[r]);
    };

    Step ring[kMfmaDepth];
#pragma unroll
    for (int d = 0; d < kMfmaDepth; ++d) {
        ring[d] = fetch(wave + kMfmaWaves * d);
    }
    for (int t0 = wave; t0 < KB; t0 += kMfmaWaves * kMfmaDepth) {
#pragma unroll
        for (int d = 0; d < kMfmaDepth; ++d) {
            const int t = t0 + kMfmaWaves * d;
            if (t < KB) consume(ring[d], t);                 // uniform over the wave
            ring[d] = fetch(t + kMfmaWaves * kMfmaDepth);
        }
    }

    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    acc = red[0][lane];
#pragma unroll
    for (int w = 1; w < kMfmaWaves; ++w) acc += red[w][lane];

    const int64_t m = m0 + fr, n = n0 + 4 * g;
    if (m >= M || n >= N) return;
    float b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bias ? bias_at(bias, bias_dtype, n + r < N ? n + r : N - 1) : 0.0f;
    const int64_t at = m * N + n;
    const bool has_bias = bias != nullptr, four = N % 4 == 0;
    if (out_dtype == mbnb::kF32)
        store_row4((float *)out + at, acc, b, has_bias, n, N, four && on_bytes(out, 16));
    else if (out_dtype == mbnb::kBF16)
        store_row4((bf16_t *)out + at, acc, b, has_bias, n, N, four && on_bytes(out, 8));
    else
        store_row4((f16_t *)out + at, acc, b, has_bias, n, N, four && on_bytes(out, 8));
#endif
}

// ---------------------------------------------------------------- k_fp8_block_decode
// Workgroup b of four waves: activation rows m0 = MT (b % row_chunks) .. + MT; wave w owns the RW weight rows from
// n0 = 4 RW (b / row_chunks) + RW w and ALL of K.  RW divides 128 and n0 is a multiple of it: a wave's rows lie in one block row of sW.
// A pass is 1024 k: lane l takes the 16 bytes at k = 1024 p + 16 l of each of its weight rows, so a 128-k block is 8 lanes, and the
// same 16 k of each activation row (32 bytes of 16-bit x, 64 of f32), read ONCE for the RW weight rows.  v_cvt_pk_f32_fp8 decodes
// two codes an instruction; 16 FMAs make the lane's share of the block's partial, one fmaf by sW[nb, k / 128] (a load per lane and
// pass) folds it into the lane's running sum.  A lane past K computes on what its clamped loads returned and keeps its old sum.
// A ring of kDepth passes is in flight, as in the kernel above: 4 for 16-bit x (MT = 1: 4 x 4 x 16 bytes of weight per lane),
// 2 for f32 x, whose rows take the registers.
// The DPP sum leaves the wave's total on lane 63, which adds the bias, rounds once and stores.
constexpr int kThreads = 256;                                // four waves
constexpr int kPass = 64 * 16;                               // k of a pass
static_assert(kPass % kBlock == 0, "a lane's 16 k lie in one scale block");
constexpr int fma_rows(int MT) { return MT == 1 ? 4 : 2; }   // RW: weight rows of a wave

// lane 63 ends with the sum over the wave: row shifts inside the rows of 16, then the row broadcasts (mx_kernels.hip's)
__device__ __forceinline__ float wave_total(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));   // row_shr:1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xF, 0xF, true));   // row_shr:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xF, 0xF, true));   // row_shr:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xF, 0xF, true));   // row_shr:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, true));   // row_bcast:15
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, true));   // row_bcast:31
    return v;
}

// element e (0 .. 16 / sizeof(T) - 1) of 16 bytes of x, as f32
template <typename T> __device__ __forceinline__ float x_at(i32x4 q, int e) {
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(f32x4, q)[e];
    } else {
        typedef T tvec __attribute__((ext_vector_type(8)));
        return (float)__builtin_bit_cast(tvec, q)[e];
    }
}

__device__ __forceinline__ void put_out(void *out, int dtype, int64_t at, float acc, bool has_bias, float b) {
    if (dtype == mbnb::kF32)
        ((float *)out)[at] = round_once<float>(acc, has_bias, b);
    else if (dtype == mbnb::kBF16)
        ((bf16_t *)out)[at] = round_once<bf16_t>(acc, has_bias, b);
    else
        ((f16_t *)out)[at] = round_once<f16_t>(acc, has_bias, b);
}

template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void k_fp8_block_decode(const T *__restrict__ x, const uint8_t *__restrict__ W, const float *__restrict__ sW,
                                                               int64_t M, int64_t N, int64_t K, const void *__restrict__ bias, int bias_dtype,
                                                               void *__restrict__ out, int out_dtype, int row_chunks) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int RW = fma_rows(MT);
    constexpr int XQ = (int)sizeof(T);                       // 16-byte loads of a lane's 16 activations: 2 (16 bit) or 4 (f32)
    constexpr int PER = 16 / (int)sizeof(T);                 // activations of one of them
    constexpr int kDepth = sizeof(T) == 2 ? 4 : 2;
    static_assert(kBlock % RW == 0, "one block row of sW per wave");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t m0 = (int64_t)(blockIdx.x % row_chunks) * MT;
    const int64_t n0 = (int64_t)(blockIdx.x / row_chunks) * (4 * RW) + wave * RW;
    const int64_t KB = (K + kBlock - 1) / kBlock;
    const int passes = (int)((K + kPass - 1) / kPass);

    const uint8_t *w_row[RW], *x_row[MT];
#pragma unroll
    for (int r = 0; r < RW; ++r) w_row[r] = W + (n0 + r < N ? n0 + r : N - 1) * K;      // a row past N reads the last row and stores nothing
#pragma unroll
    for (int m = 0; m < MT; ++m) x_row[m] = (const uint8_t *)(x + (m0 + m < M ? m0 + m : M - 1) * K);
    const float *s_row = sW + ((n0 < N ? n0 : N - 1) / kBlock) * KB;

    struct Pass {
        i32x4 w[RW], x[MT][XQ];
        float scale;
    };
    auto fetch = [&](int p) {
        Pass s;
        const int64_t k = (int64_t)p * kPass + 16 * lane, kc = k < K ? k : 0;
#pragma unroll
        for (int r = 0; r < RW; ++r) s.w[r] = load_w16(w_row[r] + kc);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < XQ; ++q) s.x[m][q] = *(const i32x4 *)(x_row[m] + kc * sizeof(T) + 16 * q);
        s.scale = s_row[kc / kBlock];
        return s;
    };

    float acc[RW][MT];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.0f;

    auto consume = [&](const Pass &s, int p) {
        const bool live = (int64_t)p * kPass + 16 * lane < K;
        float part[RW][MT];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) part[r][m] = 0.0f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {                        // dword d of the codes: the lane's k 4 d .. 4 d + 3
            float wv[RW][4];
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(s.w[r][d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(s.w[r][d], true);
                wv[r][0] = lo[0], wv[r][1] = lo[1], wv[r][2] = hi[0], wv[r][3] = hi[1];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xv = x_at<T>(s.x[m][(4 * d + e) / PER], (4 * d + e) % PER);
#pragma unroll
                    for (int r = 0; r < RW; ++r) part[r][m] = fmaf(xv, wv[r][e], part[r][m]);
                }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[r][m] = live ? fmaf(part[r][m], s.scale, acc[r][m]) : acc[r][m];
    };

    Pass ring[kDepth];
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
        ring[d] = fetch(d);
    }
    for (int p0 = 0; p0 < passes; p0 += kDepth) {
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            if (p0 + d < passes) consume(ring[d], p0 + d);   // uniform over the workgroup
            ring[d] = fetch(p0 + d + kDepth);
        }
    }

#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t n = n0 + r;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float total = wave_total(acc[r][m]);
            if (lane == 63 && n < N && m0 + m < M) put_out(out, out_dtype, (m0 + m) * N + n, total, bias != nullptr, bias ? bias_at(bias, bias_dtype, n) : 0.0f);
        }
    }
#endif
}

// ---------------------------------------------------------------- host side
bool known_dtype(int d) { return d >= MBNB_FP8DEC_F16 && d <= MBNB_FP8DEC_F32; }
const char *dtype_name(int d) { return d == MBNB_FP8DEC_F16 ? "f16" : d == MBNB_FP8DEC_BF16 ? "bf16" : "f32"; }
int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }   // no a + b - 1: M is checked by the grid alone, up to INT64_MAX

// the form of a call: the kernel, the rows of a chunk and the grid
struct Plan {
    bool mfma;
    int mt;
    int64_t chunks, grid;
};
Plan plan_of(int x_dtype, int64_t M, int64_t N) {
    Plan p;
    p.mfma = mbnb::is16(x_dtype) && M >= 2;
    p.mt = p.mfma ? kRows : (M == 1 || mbnb::is16(x_dtype)) ? 1 : M == 2 ? 2 : 4;
    p.chunks = ceil_div(M, p.mt);
    const int64_t tiles = ceil_div(N, p.mfma ? kRows : 4 * fma_rows(p.mt));
    p.grid = tiles > INT64_MAX / p.chunks ? INT64_MAX : tiles * p.chunks;
    return p;
}

template <typename T, int MT>
int launch_fma(const Plan &p, const void *x, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias, int bias_dtype,
               void *out, int out_dtype, hipStream_t s) {
    hipLaunchKernelGGL((k_fp8_block_decode<T, MT>), dim3((unsigned)p.grid), dim3(kThreads), 0, s, (const T *)x, (const uint8_t *)w, (const float *)sW, M, N,
                       K, bias, bias_dtype, out, out_dtype, (int)p.chunks);
    return mbnb::launch_status("k_fp8_block_decode");
}

template <typename T>
int launch_mfma(const Plan &p, const void *x, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias, int bias_dtype,
                void *out, int out_dtype, hipStream_t s) {
    hipLaunchKernelGGL((k_fp8_block_decode_mfma<T>), dim3((unsigned)p.grid), dim3(64 * kMfmaWaves), 0, s, (const T *)x, (const uint8_t *)w,
                       (const float *)sW, M, N, K, bias, bias_dtype, out, out_dtype, (int)p.chunks);
    return mbnb::launch_status("k_fp8_block_decode_mfma");
}

}  // namespace

extern "C" {

int mbnb_fp8dec_abi_version(void) { return MBNB_FP8DEC_ABI_VERSION; }

const char *mbnb_fp8dec_last_error(void) { return mbnb::last_error(); }

const char *mbnb_fp8dec_last_launch(void) { return mbnb::last_launch(); }

int mbnb_fp8dec_linear_weight_only(const void *x, int x_dtype, int64_t M, int64_t K, const void *w, const void *sW, int64_t N, const void *bias,
                                   int bias_dtype, void *out, int out_dtype, void *stream) {
    const char *what = "mbnb_fp8dec_linear_weight_only";
    if (!known_dtype(x_dtype) || !known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_FP8DEC_ERR_ARG, "%s: unknown dtype (x %d, bias %d, out %d)", what, x_dtype, bias_dtype, out_dtype);
    if (M < 0 || K <= 0 || N <= 0) return fail(MBNB_FP8DEC_ERR_SHAPE, "%s: M = %lld, K = %lld, N = %lld", what, (long long)M, (long long)K, (long long)N);
    if (K % 16) return fail(MBNB_FP8DEC_ERR_SHAPE, "%s: K = %lld is not a multiple of 16", what, (long long)K);
    if (K > INT32_MAX || N > INT32_MAX) return fail(MBNB_FP8DEC_ERR_SHAPE, "%s: K = %lld or N = %lld exceeds 2^31 - 1", what, (long long)K, (long long)N);
    if (M == 0) return 0;
    if (!x || !w || !sW || !out) return fail(MBNB_FP8DEC_ERR_ARG, "%s: NULL x, w, sW or out", what);
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w, 16)) return fail(MBNB_FP8DEC_ERR_ARG, "%s: misaligned x or w (16 bytes each)", what);
    if (!mbnb::aligned(sW, 4) || !mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_FP8DEC_ERR_ARG, "%s: misaligned sW, out or bias (the element size each)", what);
    const Plan p = plan_of(x_dtype, M, N);
    if (p.grid > INT32_MAX) return fail(MBNB_FP8DEC_ERR_SHAPE, "%s: %lld workgroups exceed one launch", what, (long long)p.grid);

    hipStream_t s = (hipStream_t)stream;
    int st;
    if (p.mfma)
        st = x_dtype == MBNB_FP8DEC_BF16 ? launch_mfma<bf16_t>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s)
                                         : launch_mfma<f16_t>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s);
    else if (x_dtype == MBNB_FP8DEC_BF16)
        st = launch_fma<bf16_t, 1>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s);
    else if (x_dtype == MBNB_FP8DEC_F16)
        st = launch_fma<f16_t, 1>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s);
    else
        st = p.mt == 1   ? launch_fma<float, 1>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s)
             : p.mt == 2 ? launch_fma<float, 2>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s)
                         : launch_fma<float, 4>(p, x, M, K, w, sW, N, bias, bias_dtype, out, out_dtype, s);
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "fp8_block_decode%s %s MT%d %lldx%lldx%lld", p.mfma ? "_mfma" : "", dtype_name(x_dtype), p.mt,
                 (long long)M, (long long)N, (long long)K);
    return st;
}

}  // extern "C"
