// mx_kernels.hip — the OCP MX quantiser / decoder, the MXFP4 linear on gfx950's block-scaled MFMA, and the C ABI of
// libmbnb_mx.so (include/mbnb_mx.h; the format and the lane map: DESIGN.md §25).
//
//   k_mx_quantize    [rows, K] of f16 / bf16 / f32 -> fp4 or fp8 codes + one E8M0 byte per 32 elements.  Four lanes share a block
//                    (8 elements each); everything after the f32 read is integer work or an exact power-of-two scaling.
//   k_mx_dequantize  the inverse: value(code) * 2^(byte - 127), exact in f32, one rounding to the output dtype.
//   k_gemm_mx        out[M, N] = A . W^T + bias over the codes and scale bytes of both operands as they lie in memory:
//                    v_mfma_scale_f32_16x16x128_f8f6f4, whose lane holds the scale byte of one MX block (32 k of one row).
//                    128 x 128 output tile, 4 waves of 64 x 64, K-step 128, two LDS stages filled by 16-byte LDS-DMA.
//   k_mx_decode      the weight-only linear for decode steps: the activation stays in its dtype, the codes and
//                    scale bytes are streamed once and decoded in registers, one lane per MX block, f32 FMA (one 16-bit row, f32 rows);
//   k_mx_decode_mfma the same for 2 and more bf16 / f16 rows on v_mfma_f32_16x16x32, whose K is one MX block.
#include "../../include/mbnb_mx.h"
#include "host.h"
#include "mx_decode.h"

static_assert(MBNB_MX_F16 == mbnb::kF16 && MBNB_MX_BF16 == mbnb::kBF16 && MBNB_MX_F32 == mbnb::kF32, "host.h's dtype codes");

namespace {

using mbnb::bf16_t;
using mbnb::f16_t;
using mbnb::fail;
// the scale, the bias load, the output store and the 16 x 16 MFMA decode tile: mx_decode.h, shared with the two expert libraries
using mbnb::mx::v4i;
using mbnb::mx::v4f;
using mbnb::mx::kNaNScale;
using mbnb::mx::kOneScale;
using mbnb::mx::kMfmaWaves;
using mbnb::mx::scale_value;
using mbnb::mx::load_bias;
using mbnb::mx::store_out;
using mbnb::mx::TileLds;
using mbnb::mx::TileSums;
using mbnb::mx::tile_walk;
using mbnb::mx::tile_reduce;

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;          // every launch: 4 waves

// ---------------------------------------------------------------- the element formats
// |a| -> E2M1 code 0..7 (0, .5, 1, 1.5, 2, 3, 4, 6), nearest, ties to the even code, everything above 5 to 6
__device__ __forceinline__ uint32_t enc_e2m1(float a) {
    return (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) +
           (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
}

// the bits of |a| (finite) -> E4M3 code 0..0x7E, RNE, saturating at 448
__device__ __forceinline__ uint32_t enc_e4m3(uint32_t a) {
    if (a >= 0x3C800000u) {                                  // 2^-6 and up: the normal codes
        a += 0x7FFFFu + ((a >> 20) & 1u);                    // RNE at mantissa bit 20; a carry moves into the exponent
        const uint32_t code = (a >> 20) - (120u << 3);       // exponent bias 127 -> 7
        return code < 0x7Eu ? code : 0x7Eu;
    }
    return (uint32_t)rintf(__uint_as_float(a) * 512.0f);     // multiples of 2^-9: 0..8, and 8 is the first normal code
}

__device__ __forceinline__ float dec_e2m1(uint32_t c) {
    // magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6 as f32 bits: codes 2..7 are (1 + m/2) * 2^(e - 1)
    const uint32_t m = c & 7u;
    const uint32_t bits = m < 2u ? (m ? 0x3F000000u : 0u) : (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);
    return __uint_as_float(bits | ((c & 8u) << 28));
}

__device__ __forceinline__ float dec_e4m3(uint32_t c) {
    const uint32_t e = (c >> 3) & 15u, m = c & 7u, sign = (c & 0x80u) << 24;
    if ((c & 0x7Fu) == 0x7Fu) return __uint_as_float(0x7FC00000u);
    if (e == 0u) return __uint_as_float(__float_as_uint((float)m * 0.001953125f) | sign);    // m * 2^-9
    return __uint_as_float(((e + 120u) << 23) | (m << 20) | sign);
}

template <typename T> __device__ __forceinline__ void load8(const T *p, float v[8]) {
    typedef T tvec __attribute__((ext_vector_type(8)));
    const tvec t = *(const tvec *)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}
template <> __device__ __forceinline__ void load8<float>(const float *p, float v[8]) {
    const float4 a = ((const float4 *)p)[0], b = ((const float4 *)p)[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

template <typename T> __device__ __forceinline__ void store8(T *p, const float v[8]) {
    typedef T tvec __attribute__((ext_vector_type(8)));
    tvec t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (T)v[j];
    *(tvec *)p = t;
}
template <> __device__ __forceinline__ void store8<float>(float *p, const float v[8]) {
    ((float4 *)p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4 *)p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// ---------------------------------------------------------------- quantiser
// Thread i owns elements [8 i, 8 i + 8); the four threads of a block are consecutive lanes of one wave (K % 32 == 0, so a
// block never straddles a row or the end of the grid).
template <typename T, int ELEM>
__global__ __launch_bounds__(kThreads) void k_mx_quantize(const T *__restrict__ x, int64_t groups, uint8_t *__restrict__ codes,
                                                          uint8_t *__restrict__ scales) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= groups) return;
    float v[8];
    load8<T>(x + i * 8, v);
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, __float_as_uint(v[j]) & 0x7FFFFFFFu);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
    const uint32_t E = amax >> 23;                           // 255: the block holds an Inf or a NaN (their bits top every finite value's)
    constexpr uint32_t emax = ELEM == MBNB_MX_FP4 ? 2u : 8u;
    const uint32_t byte = E == 255u ? (uint32_t)kNaNScale : (E > emax ? E - emax : 0u);
    const float mult = __uint_as_float((254u - byte) << 23);  // 2^(127 - byte): 2^-125 .. 2^127 (unused for a NaN block)
    uint32_t c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = v[j] * mult;                         // exact, or an underflow far below half the smallest element value
        const uint32_t u = __float_as_uint(s), a = u & 0x7FFFFFFFu;
        if constexpr (ELEM == MBNB_MX_FP4)
            c[j] = E == 255u ? 0u : enc_e2m1(__uint_as_float(a)) | ((u >> 28) & 8u);
        else
            c[j] = E == 255u ? 0u : enc_e4m3(a) | ((u >> 24) & 0x80u);
    }
    if constexpr (ELEM == MBNB_MX_FP4) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) w |= c[j] << (4 * j);    // even k in the low nibble of its byte, bytes in k order
        *(uint32_t *)(codes + i * 4) = w;
    } else {
        uint2 w;
        w.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        w.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
        *(uint2 *)(codes + i * 8) = w;
    }
    if ((i & 3) == 0) scales[i >> 2] = (uint8_t)byte;
}

// ---------------------------------------------------------------- decoder
template <typename T, int ELEM>
__global__ __launch_bounds__(kThreads) void k_mx_dequantize(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ scales,
                                                            int64_t groups, T *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= groups) return;
    const uint32_t byte = scales[i >> 2];
    const float s = scale_value(byte);
    float v[8];
    if constexpr (ELEM == MBNB_MX_FP4) {
        const uint32_t w = *(const uint32_t *)(codes + i * 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = dec_e2m1((w >> (4 * j)) & 15u) * s;
    } else {
        const uint2 w = *(const uint2 *)(codes + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = dec_e4m3(((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 255u) * s;
    }
    if (byte == (uint32_t)kNaNScale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(0x7FC00000u);
    }
    store8<T>(out + i * 8, v);
}

// ---------------------------------------------------------------- the GEMM
// One workgroup = 4 waves = one TM x TN output tile, wave (wm, wn) owns 64 x 64 of it as 4 x 4 MFMA tiles of 16 x 16.
//
// v_mfma_scale_f32_16x16x128_f8f6f4, operands as measured with the identity test: lane l = (g = l >> 4, l & 15)
// holds row (A) / column (B) l & 15.  An fp4 operand: the 32 consecutive k from 32 g, one MX block, as 16 bytes in registers
// 0..3 (the lower k in the low nibble).  An fp8 operand: registers 0..3 hold the 16 k from 16 g, registers 4..7 the 16 k from
// 64 + 16 g (the instruction is two K = 64 passes), so a lane's bytes belong to two blocks.  The scales do not follow the data:
// whatever the format, byte 0 of lane l's scale register (opsel 0) is the scale of k block g of row / column l & 15.
// D: column l & 15, rows 4 g + r.  A is the activation (cbsz = its format), B the fp4 weight (blgp 4).
//
// LDS image of a stage, in 16-byte chunks: an operand's tile is [half][row][g]: for fp4 one half, chunk g = the k block g of
// the K-step; for fp8 chunk [h][row][g] = the 16 k from 64 h + 16 g.  So a wave's fragment read -- lane l takes chunk
// [h][row0 + (l & 15)][l >> 4] -- is 1 KiB of consecutive LDS (no bank conflict), and a wave's LDS-DMA, which writes 64
// consecutive chunks, reads 16 rows x 64 bytes of the operand.  Chunks of rows past the operand or of k blocks past K are fetched from the operand's first 16
// bytes instead; the k blocks past K are zeroed in registers on the last K-step, the rows past the operand are never stored.
constexpr int TM = MBNB_MX_TILE_M, TN = MBNB_MX_TILE_N, KS = MBNB_MX_K_STEP;
static_assert(TM == 128 && TN == 128 && KS == 128, "the wave grid and the chunk maps below are written for 128 x 128 x 128");

template <int AELEM, typename TO>
__global__ __launch_bounds__(kThreads) void k_gemm_mx(const uint8_t *__restrict__ A, const uint8_t *__restrict__ As,
                                                      const uint8_t *__restrict__ W, const uint8_t *__restrict__ Ws, int64_t M, int64_t N,
                                                      int64_t K, const void *__restrict__ bias, int bias_dtype, TO *__restrict__ out,
                                                      int tiles_m) {
    constexpr bool A8 = AELEM == MBNB_MX_FP8;
    constexpr int AH = A8 ? 2 : 1;                           // 16-byte halves of an activation block
    constexpr int A_BYTES = TM * 4 * AH * 16, B_BYTES = TN * 4 * 16, STAGE = A_BYTES + B_BYTES;
    constexpr int NA = A_BYTES / 16 / kThreads, NB = B_BYTES / 16 / kThreads;   // LDS-DMA instructions per thread and stage
    constexpr int CBSZ = A8 ? 0 : 4, BLGP = 4;
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * STAGE];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)(blockIdx.x % tiles_m) * TM, n0 = (int64_t)(blockIdx.x / tiles_m) * TN;
    const int64_t KB = K / 32;                               // blocks, and scale bytes, per row
    const int64_t lda = A8 ? K : K / 2, ldw = K / 2;         // bytes per row of codes
    const int nk = (int)((K + KS - 1) / KS);

    // the chunks this thread stages: chunk c = i * 256 + tid of an image = [half][row][g]
    const uint8_t *a_src[NA], *b_src[NB];
    int a_k[NA], b_k[NB];                                    // the chunk's first k inside the K-step
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int c = i * kThreads + tid, h = c / (TM * 4), row = (c % (TM * 4)) >> 2;
        a_k[i] = A8 ? h * 64 + (c & 3) * 16 : (c & 3) * 32;
        a_src[i] = m0 + row < M ? A + (m0 + row) * lda + (A8 ? a_k[i] : a_k[i] >> 1) : nullptr;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int c = i * kThreads + tid, row = c >> 2;
        b_k[i] = (c & 3) * 32;
        b_src[i] = n0 + row < N ? W + (n0 + row) * ldw + (b_k[i] >> 1) : nullptr;
    }
    auto stage = [&](int s, int64_t k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint8_t *p = a_src[i] && k0 + a_k[i] < K ? a_src[i] + (A8 ? k0 : k0 >> 1) : A;
            auto gp = (const __attribute__((address_space(1))) void *)p;
            auto lp = (__attribute__((address_space(3))) void *)(smem + s * STAGE + (i * kThreads + wave * 64) * 16);
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const uint8_t *p = b_src[i] && k0 + b_k[i] < K ? b_src[i] + (k0 >> 1) : W;
            auto gp = (const __attribute__((address_space(1))) void *)p;
            auto lp = (__attribute__((address_space(3))) void *)(smem + s * STAGE + A_BYTES + (i * kThreads + wave * 64) * 16);
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        }
    };

    // this lane's scale bytes of K-step t: rows wm * 64 + 16 i + fr of the activation, wn * 64 + 16 j + fr of the weight, k block g
    const uint8_t *as_row[4], *ws_row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t am = m0 + wm * 64 + i * 16 + fr, wr = n0 + wn * 64 + i * 16 + fr;
        as_row[i] = am < M ? As + am * KB : nullptr;
        ws_row[i] = wr < N ? Ws + wr * KB : nullptr;
    }
    auto load_scales = [&](int t, int sa[4], int sb[4]) {
        const int64_t kb = (int64_t)t * (KS / 32) + g;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sa[i] = as_row[i] && kb < KB ? (int)as_row[i][kb] : kOneScale;
            sb[i] = ws_row[i] && kb < KB ? (int)ws_row[i][kb] : kOneScale;
        }
    };
    // bit q of the mask: row / column q of the 16 x 16 tile has a NaN block (a lane holds row l & 15's scale, not its outputs' rows)
    auto fold16 = [](uint64_t b) { return (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xFFFFu); };

    v4f acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t a_nan[4] = {0, 0, 0, 0}, b_nan[4] = {0, 0, 0, 0};
    int sa[4], sb[4], sa_next[4], sb_next[4];

    stage(0, 0);
    load_scales(0, sa_next, sb_next);
    for (int t = 0; t < nk; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sa[i] = sa_next[i], sb[i] = sb_next[i];
        // stage t has landed for every wave, and every wave is done reading the other stage (K-step t - 1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nk) {
            stage((t + 1) & 1, (int64_t)(t + 1) * KS);
            load_scales(t + 1, sa_next, sb_next);
        }
        const uint8_t *sA = smem + (t & 1) * STAGE, *sB = sA + A_BYTES;
        v8i af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + fr;
            const v4i lo = *(const v4i *)(sA + (row * 4 + g) * 16);
            v4i hi = v4i{0, 0, 0, 0};
            if constexpr (A8) hi = *(const v4i *)(sA + (TM * 4 + row * 4 + g) * 16);
            af[i] = v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const v4i lo = *(const v4i *)(sB + ((wn * 64 + j * 16 + fr) * 4 + g) * 16);
            bf[j] = v8i{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
        }
        if (t == nk - 1 && K % KS) {                         // the k past K count as zeros, in both operands
            const int64_t k0 = (int64_t)t * KS;
            const bool lo_out = k0 + (A8 ? 16 : 32) * g >= K, hi_out = k0 + 64 + 16 * g >= K, b_out = k0 + 32 * g >= K;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (lo_out) af[i][q] = 0;
                    if (hi_out) af[i][4 + q] = 0;
                    if (b_out) bf[i][q] = 0;
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
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bf[j], acc[i][j], CBSZ, BLGP, 0, sa[i], 0, sb[j]);
    }

    // epilogue: + bias in f32, NaN rows and columns, one rounding, guarded stores
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = n0 + wn * 64 + j * 16 + fr;
        if (col >= N) continue;
        const float b = bias ? load_bias(bias, bias_dtype, col) : 0.0f;
        const bool col_nan = (b_nan[j] >> fr) & 1u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm * 64 + i * 16 + 4 * g + r;
                if (row >= M) continue;
                float v = acc[i][j][r] + b;
                if (col_nan || ((a_nan[i] >> (4 * g + r)) & 1u)) v = __uint_as_float(0x7FC00000u);
                out[row * N + col] = (TO)v;
            }
    }
}

// ---------------------------------------------------------------- the weight-only decode linear
// out[m, n] = sum_b 2^(s[n, b] - 127) * (sum_{k in block b} x[m, k] * v(code[n, k])) + bias[n]: the activation is NOT quantised.
// One lane owns one MX block of a weight row per pass: 16 bytes of codes (one dwordx4) and one scale byte, so a wave covers
// kDecodeChunk = 2048 k of a row, 1 KiB of codes, coalesced.  A wave runs RW weight rows against one read of the activations, a
// workgroup 4 RW rows against one staging of them: the workgroup copies its MT rows x 2048 k of x into LDS per pass (zeros for
// the rows past M and the k past K), lane l's 32 values of a row as S 16-byte slots at slot (row * 64 + l) * S + (j ^ swz(l)).
// The XOR spreads the 16 lanes of every ds_read_b128 lane group over the 16 slots of the 256-byte bank row, so the per-lane
// 64- / 128-byte reads are conflict-free.  The 32 products of a block go into one partial sum per activation row (f32 FMA; a
// product of a 16-bit x and an E2M1 value is exact), which is multiplied by the block's scale ONCE and added to the lane's
// accumulator: an element that alone is no f32 (code 6 under byte 254) never exists.  A 0xFF byte anywhere in the row makes the
// whole column NaN, whatever x holds.  DPP wave sums; lane 63 adds the bias and stores with one rounding.  This FMA form serves ONE
// 16-bit row (MT 1) and every call with f32 rows (MT 1, 2, 4, 8: 64 KiB of LDS at 8); 2 and more 16-bit rows take
// k_mx_decode_mfma below.
constexpr int kDecodeChunk = 2048;
constexpr int decode_rw(int mt) { return mt == 1 ? 1 : (mt <= 4 ? 2 : 4); }      // weight rows per wave
static_assert(MBNB_MX_DECODE_ROWS == 16, "the MFMA form's 16 x 16 tile and the MT dispatch below");

// nibble E of w -> the E2M1 value: the code's three magnitude bits placed at f32 bits 22..24 are 2^-126 times the value (codes 0
// and 1 as the subnormals 0 and 2^-127), so one exact multiplication by 2^126 finishes the decode
template <int E> __device__ __forceinline__ float dec_nibble(uint32_t w) {
    const uint32_t t = 4 * E <= 22 ? w << (22 - 4 * E > 0 ? 22 - 4 * E : 0) : w >> (4 * E - 22 > 0 ? 4 * E - 22 : 0);
    const uint32_t bits = (t & 0x01C00000u) | ((w << (28 - 4 * E)) & 0x80000000u);
    return __uint_as_float(bits) * 0x1p126f;
}

__device__ __forceinline__ void decode8(uint32_t w, float v[8]) {
    v[0] = dec_nibble<0>(w), v[1] = dec_nibble<1>(w), v[2] = dec_nibble<2>(w), v[3] = dec_nibble<3>(w);
    v[4] = dec_nibble<4>(w), v[5] = dec_nibble<5>(w), v[6] = dec_nibble<6>(w), v[7] = dec_nibble<7>(w);
}

// lane 63 ends with the sum over the wave: row shifts inside the rows of 16, then the row broadcasts
__device__ __forceinline__ float decode_wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));   // row_shr:1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xF, 0xF, true));   // row_shr:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xF, 0xF, true));   // row_shr:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xF, 0xF, true));   // row_shr:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, true));   // row_bcast:15
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, true));   // row_bcast:31
    return v;
}

template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void k_mx_decode(const T *__restrict__ x, const uint8_t *__restrict__ W, const uint8_t *__restrict__ Ws,
                                                        int64_t M, int64_t N, int64_t K, const void *__restrict__ bias, int bias_dtype,
                                                        void *__restrict__ out, int out_dtype, int row_chunks) {
    constexpr int RW = decode_rw(MT);
    constexpr int S = 32 * (int)sizeof(T) / 16;              // 16-byte slots of a lane's 32 activations: 4 (16 bit) or 8 (f32)
    constexpr int UNITS = 64 * S;                            // slots of one activation row of a pass
    constexpr int PER = 16 / (int)sizeof(T);                 // activations per slot
    static_assert(MT * UNITS * 16 <= 65536 && (MT * UNITS) % kThreads == 0, "the staged rows fit 64 KiB of LDS");
    __shared__ __attribute__((aligned(16))) uint8_t xs[MT * UNITS * 16];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)(blockIdx.x % row_chunks) * MT;
    const int64_t n0 = (int64_t)(blockIdx.x / row_chunks) * (4 * RW) + wave * RW;
    const int64_t KB = K / 32, ldw = K / 2;
    const int swz = (lane / (16 / S)) & (S - 1);

    const uint8_t *w_row[RW], *s_row[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t n = n0 + r < N ? n0 + r : N - 1;       // a row past N reads the last row and stores nothing
        w_row[r] = W + n * ldw;
        s_row[r] = Ws + n * KB;
    }
    float acc[RW][MT];
    bool ff[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        ff[r] = false;
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.0f;
    }

    for (int64_t k0 = 0; k0 < K; k0 += kDecodeChunk) {
        if (k0) __syncthreads();                             // every wave is done with the last pass's activations
        const int64_t blk = k0 / 32 + lane;
        const bool live = blk < KB;
        v4i wq[RW];
        uint32_t sb[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            wq[r] = live ? __builtin_nontemporal_load((const v4i *)(w_row[r] + blk * 16)) : v4i{0, 0, 0, 0};
            sb[r] = live ? (uint32_t)s_row[r][blk] : (uint32_t)kOneScale;
        }
#pragma unroll
        for (int it = 0; it < MT * UNITS / kThreads; ++it) {
            const int u = it * kThreads + tid, row = u / UNITS, c = u % UNITS;
            const int64_t k = k0 + (int64_t)c * PER;
            v4i v = v4i{0, 0, 0, 0};
            if (m0 + row < M && k < K) v = *(const v4i *)(x + (m0 + row) * K + k);
            const int l = c / S, j = c % S;
            *(v4i *)(xs + ((row * 64 + l) * S + (j ^ ((l / (16 / S)) & (S - 1)))) * 16) = v;
        }
        __syncthreads();

        float p[RW][MT];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) p[r][m] = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                        // dword q of the codes: the block's k 8 q .. 8 q + 7
            float wv[RW][8];
#pragma unroll
            for (int r = 0; r < RW; ++r) decode8((uint32_t)wq[r][q], wv[r]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float xv[8];
                const uint8_t *base = xs + (m * 64 + lane) * S * 16;
                if constexpr (sizeof(T) == 2) {
                    typedef T tvec __attribute__((ext_vector_type(8)));
                    const tvec t = *(const tvec *)(base + ((q ^ swz) * 16));
#pragma unroll
                    for (int e = 0; e < 8; ++e) xv[e] = (float)t[e];
                } else {
                    const float4 a = *(const float4 *)(base + (((2 * q) ^ swz) * 16)), b = *(const float4 *)(base + (((2 * q + 1) ^ swz) * 16));
                    xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w, xv[4] = b.x, xv[5] = b.y, xv[6] = b.z, xv[7] = b.w;
                }
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int e = 0; e < 8; ++e) p[r][m] = __builtin_fmaf(xv[e], wv[r][e], p[r][m]);
            }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            ff[r] |= sb[r] == (uint32_t)kNaNScale;
            const float sv = scale_value(sb[r] == (uint32_t)kNaNScale ? (uint32_t)kOneScale : sb[r]);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[r][m] = __builtin_fmaf(p[r][m], sv, acc[r][m]);
        }
    }

#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const bool col_nan = __ballot(ff[r]) != 0;           // a 0xFF byte anywhere in weight row n: the column is NaN
        const int64_t n = n0 + r;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float s = decode_wave_sum(acc[r][m]);
            if (lane == 63 && n < N && m0 + m < M) {
                const float v = s + (bias ? load_bias(bias, bias_dtype, n) : 0.0f);
                store_out(out, out_dtype, (m0 + m) * N + n, col_nan ? __uint_as_float(0x7FC00000u) : v);
            }
        }
    }
}

// k_mx_decode_mfma: 2 to 16 rows of 16-bit activations on v_mfma_f32_16x16x32_{bf16,f16}, whose K = 32 is one MX block.  A workgroup
// of 8 waves owns 16 weight rows and ALL of K against 16 activation rows: the decode tile of mx_decode.h.  tile_walk gives every
// wave its partial sums over the k-steps w, w + 8, ... of 4 blocks (128 k) each, tile_reduce adds the eight through LDS in wave
// order; the expert kernels (moe_kernels.hip, moemlp_kernels.hip) call the same two functions, so their bits are this kernel's.
// What is this kernel's own: where a workgroup finds its rows and columns, and the store.  The A fragment A[row m = l & 15]
// [k = 8 g + j] is 16 bytes of x straight from memory (rows past M and k past K count as zeros); D is column n = l & 15 on the lane,
// rows 4 g + r.  (Two tiles of 16 weight rows per workgroup, every x fragment feeding two MFMAs, measured slower at 11008 rows:
// DESIGN.md §27.)
template <typename T>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mx_decode_mfma(const T *__restrict__ x, const uint8_t *__restrict__ W,
                                                                     const uint8_t *__restrict__ Ws, int64_t M, int64_t N, int64_t K,
                                                                     const void *__restrict__ bias, int bias_dtype, void *__restrict__ out,
                                                                     int out_dtype, int row_chunks) {
    __shared__ TileLds lds;
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)(blockIdx.x % row_chunks) * MBNB_MX_DECODE_ROWS;
    const int64_t n0 = (int64_t)(blockIdx.x / row_chunks) * 16;
    const int64_t KB = K / 32, ldw = K / 2;
    const int64_t n = n0 + fr < N ? n0 + fr : N - 1;         // a column past N reads the last weight row and stores nothing
    const bool x_live = m0 + fr < M;                         // a row past M reads row 0 and counts as zeros
    const T *x_row = x + (x_live ? m0 + fr : 0) * K + 8 * g;

    const TileSums part = tile_walk<T>(x_row, x_live, W + n * ldw, Ws + n * KB, KB, wave, g);
    const bool stores = wave == 0 && n0 + fr < N;
    const float b = stores && bias ? load_bias(bias, bias_dtype, n) : 0.0f;   // requested before the reduction's barrier
    v4f s;
    const bool col_nan = tile_reduce(lds, part, wave, lane, s);
    if (stores) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 4 * g + r;
            if (m < M) store_out(out, out_dtype, m * N + n, col_nan ? __uint_as_float(0x7FC00000u) : s[r] + b);
        }
    }
}

// ---------------------------------------------------------------- host side
const char *elem_name(int elem) { return elem == MBNB_MX_FP4 ? "fp4" : "fp8"; }
bool known_dtype(int d) { return d >= MBNB_MX_F16 && d <= MBNB_MX_F32; }
bool known_elem(int e) { return e == MBNB_MX_FP4 || e == MBNB_MX_FP8; }
int64_t code_bytes(int64_t rows, int64_t K, int elem) { return elem == MBNB_MX_FP4 ? rows * K / 2 : rows * K; }

// the checks every entry point shares; 0 or the status
int check_shape(const char *what, int64_t rows, int64_t K) {
    if (rows < 0 || K <= 0) return fail(MBNB_MX_ERR_SHAPE, "%s: rows = %lld, K = %lld", what, (long long)rows, (long long)K);
    if (K % 32) return fail(MBNB_MX_ERR_SHAPE, "%s: K = %lld is not a multiple of the MX block, 32", what, (long long)K);
    if (rows > mbnb::kMaxElems / K) return fail(MBNB_MX_ERR_SHAPE, "%s: %lld x %lld elements exceed one launch", what, (long long)rows, (long long)K);
    return 0;
}

template <typename T, int ELEM> int launch_quantize(const void *x, int64_t rows, int64_t K, void *codes, void *scales, hipStream_t s) {
    const int64_t groups = rows * K / 8;
    hipLaunchKernelGGL((k_mx_quantize<T, ELEM>), dim3((unsigned)((groups + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const T *)x,
                       groups, (uint8_t *)codes, (uint8_t *)scales);
    return mbnb::launch_status("k_mx_quantize");
}

int quantize(const void *x, int64_t rows, int64_t K, int dtype, int elem, void *codes, void *scales, hipStream_t s) {
    return mbnb::with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return elem == MBNB_MX_FP4 ? launch_quantize<T, MBNB_MX_FP4>(x, rows, K, codes, scales, s)
                                   : launch_quantize<T, MBNB_MX_FP8>(x, rows, K, codes, scales, s);
    });
}

template <int AELEM, typename TO>
int launch_gemm(const uint8_t *A, const uint8_t *As, const void *W, const void *Ws, int64_t M, int64_t N, int64_t K, const void *bias,
                int bias_dtype, void *out, hipStream_t s) {
    const int64_t tiles_m = (M + TM - 1) / TM, tiles_n = (N + TN - 1) / TN;
    hipLaunchKernelGGL((k_gemm_mx<AELEM, TO>), dim3((unsigned)(tiles_m * tiles_n)), dim3(kThreads), 0, s, A, As, (const uint8_t *)W,
                       (const uint8_t *)Ws, M, N, K, bias, bias_dtype, (TO *)out, (int)tiles_m);
    return mbnb::launch_status("k_gemm_mx");
}

// the activation rows of one pass of the FMA form: the power of two that holds M, up to kDecodeFmaRows (f32 rows: 64 KiB of LDS)
constexpr int kDecodeFmaRows = MBNB_MX_DECODE_ROWS / 2;
int decode_rows(int64_t M) {
    int mt = 1;
    while (mt < M && mt < kDecodeFmaRows) mt *= 2;
    return mt;
}
// 2 rows and more of 16-bit activations take the MFMA form: 16 weight rows per workgroup, 16 activation rows per pass
bool decode_mfma(int64_t M, int x_dtype) { return M >= 2 && x_dtype != MBNB_MX_F32; }
int64_t decode_grid(int64_t M, int64_t N, int mt, bool mfma) {
    if (mfma) return ((N + 15) / 16) * ((M + MBNB_MX_DECODE_ROWS - 1) / MBNB_MX_DECODE_ROWS);
    const int rows = 4 * decode_rw(mt);
    return ((N + rows - 1) / rows) * ((M + mt - 1) / mt);
}

template <typename T>
int launch_decode_mfma(const void *x, const void *W, const void *Ws, int64_t M, int64_t N, int64_t K, const void *bias, int bias_dtype,
                       void *out, int out_dtype, hipStream_t s) {
    if constexpr (sizeof(T) != 2) {
        return fail(MBNB_MX_ERR_ARG, "k_mx_decode_mfma: 16-bit activations only");
    } else {
        const int chunks = (int)((M + MBNB_MX_DECODE_ROWS - 1) / MBNB_MX_DECODE_ROWS);
        const dim3 grid((unsigned)decode_grid(M, N, MBNB_MX_DECODE_ROWS, true)), block(64 * kMfmaWaves);
        hipLaunchKernelGGL((k_mx_decode_mfma<T>), grid, block, 0, s, (const T *)x, (const uint8_t *)W, (const uint8_t *)Ws, M, N, K, bias,
                           bias_dtype, out, out_dtype, chunks);
        return mbnb::launch_status("k_mx_decode_mfma");
    }
}

template <typename T, int MT>
int launch_decode(const void *x, const void *W, const void *Ws, int64_t M, int64_t N, int64_t K, const void *bias, int bias_dtype, void *out,
                  int out_dtype, hipStream_t s) {
    hipLaunchKernelGGL((k_mx_decode<T, MT>), dim3((unsigned)decode_grid(M, N, MT, false)), dim3(kThreads), 0, s, (const T *)x, (const uint8_t *)W,
                       (const uint8_t *)Ws, M, N, K, bias, bias_dtype, out, out_dtype, (int)((M + MT - 1) / MT));
    return mbnb::launch_status("k_mx_decode");
}

}  // namespace

extern "C" {

int mbnb_mx_abi_version(void) { return MBNB_MX_ABI_VERSION; }

const char *mbnb_mx_last_error(void) { return mbnb::last_error(); }

const char *mbnb_mx_last_launch(void) { return mbnb::last_launch(); }

int mbnb_mx_quantize(const void *x, int64_t rows, int64_t K, int dtype, int elem, void *codes, void *scales, void *stream) {
    if (!known_dtype(dtype)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_quantize: unknown dtype %d", dtype);
    if (!known_elem(elem)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_quantize: unknown element format %d", elem);
    if (const int st = check_shape("mbnb_mx_quantize", rows, K)) return st;
    if (rows == 0) return 0;
    if (!x || !codes || !scales) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_quantize: NULL x, codes or scales");
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(codes, 16))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_quantize: misaligned x or codes (16 bytes each)");
    const int st = quantize(x, rows, K, dtype, elem, codes, scales, (hipStream_t)stream);
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_quant %s", elem_name(elem));
    return st;
}

int mbnb_mx_dequantize(const void *codes, const void *scales, int64_t rows, int64_t K, int elem, int out_dtype, void *out,
                       void *stream) {
    if (!known_elem(elem)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_dequantize: unknown element format %d", elem);
    if (!known_dtype(out_dtype)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_dequantize: unknown dtype %d", out_dtype);
    if (const int st = check_shape("mbnb_mx_dequantize", rows, K)) return st;
    if (rows == 0) return 0;
    if (!codes || !scales || !out) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_dequantize: NULL codes, scales or out");
    if (!mbnb::aligned(codes, 16) || !mbnb::aligned(out, 16))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_dequantize: misaligned codes or out (16 bytes each)");
    const int64_t groups = rows * K / 8;
    const dim3 grid((unsigned)((groups + kThreads - 1) / kThreads));
    hipStream_t s = (hipStream_t)stream;
    const int st = mbnb::with_dtype(out_dtype, [&](auto t) {
        using T = decltype(t);
        if (elem == MBNB_MX_FP4)
            hipLaunchKernelGGL((k_mx_dequantize<T, MBNB_MX_FP4>), grid, dim3(kThreads), 0, s, (const uint8_t *)codes, (const uint8_t *)scales, groups, (T *)out);
        else
            hipLaunchKernelGGL((k_mx_dequantize<T, MBNB_MX_FP8>), grid, dim3(kThreads), 0, s, (const uint8_t *)codes, (const uint8_t *)scales, groups, (T *)out);
        return mbnb::launch_status("k_mx_dequantize");
    });
    if (st == 0) snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_dequant %s", elem_name(elem));
    return st;
}

int64_t mbnb_mx_workspace_bytes(int64_t M, int64_t K, int act_elem) {
    if (!known_elem(act_elem)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_workspace_bytes: unknown element format %d", act_elem);
    if (const int st = check_shape("mbnb_mx_workspace_bytes", M, K)) return st;
    return mbnb::round256(code_bytes(M, K, act_elem)) + mbnb::round256(M * (K / 32));
}

int mbnb_mx_linear(const void *x, int64_t M, int64_t K, int x_dtype, const void *w_codes, const void *w_scales, int64_t N,
                   int act_elem, const void *bias, int bias_dtype, void *out, int out_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream) {
    if (!known_dtype(x_dtype) || !known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: unknown dtype (x %d, bias %d, out %d)", x_dtype, bias_dtype, out_dtype);
    if (!known_elem(act_elem)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: unknown element format %d", act_elem);
    if (const int st = check_shape("mbnb_mx_linear", M, K)) return st;
    if (N <= 0 || N > mbnb::kMaxElems / K || (M > 0 && N > mbnb::kMaxElems / M))
        return fail(MBNB_MX_ERR_SHAPE, "mbnb_mx_linear: N = %lld", (long long)N);
    if (M == 0) return 0;
    const int64_t tiles = ((M + TM - 1) / TM) * ((N + TN - 1) / TN);
    if (tiles > INT32_MAX) return fail(MBNB_MX_ERR_SHAPE, "mbnb_mx_linear: %lld workgroups exceed one launch", (long long)tiles);
    if (!x || !w_codes || !w_scales || !out) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: NULL x, w_codes, w_scales or out");
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w_codes, 16))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: misaligned x or w_codes (16 bytes each)");
    if (!mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: misaligned out or bias (the element size each)");
    const int64_t cbytes = mbnb::round256(code_bytes(M, K, act_elem)), need = cbytes + mbnb::round256(M * (K / 32));
    if (!workspace || workspace_bytes < need)
        return fail(MBNB_MX_ERR_WORKSPACE, "mbnb_mx_linear: workspace of %lld bytes, %lld needed", (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!mbnb::aligned(workspace, 16)) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear: misaligned workspace (16 bytes)");
    uint8_t *a_codes = (uint8_t *)workspace, *a_scales = a_codes + cbytes;
    hipStream_t s = (hipStream_t)stream;
    if (const int st = quantize(x, M, K, x_dtype, act_elem, a_codes, a_scales, s)) return st;
    const int st = mbnb::with_dtype(out_dtype, [&](auto t) {
        using T = decltype(t);
        return act_elem == MBNB_MX_FP4 ? launch_gemm<MBNB_MX_FP4, T>(a_codes, a_scales, w_codes, w_scales, M, N, K, bias, bias_dtype, out, s)
                                       : launch_gemm<MBNB_MX_FP8, T>(a_codes, a_scales, w_codes, w_scales, M, N, K, bias, bias_dtype, out, s);
    });
    if (st == 0)
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, "mx_quant %s + gemm_mx %s %dx%d", elem_name(act_elem), elem_name(act_elem), TM, TN);
    return st;
}

int mbnb_mx_linear_weight_only(const void *x, int64_t M, int64_t K, int x_dtype, const void *w_codes, const void *w_scales, int64_t N,
                               const void *bias, int bias_dtype, void *out, int out_dtype, void *stream) {
    if (!known_dtype(x_dtype) || !known_dtype(out_dtype) || (bias && !known_dtype(bias_dtype)))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear_weight_only: unknown dtype (x %d, bias %d, out %d)", x_dtype, bias_dtype, out_dtype);
    if (const int st = check_shape("mbnb_mx_linear_weight_only", M, K)) return st;
    if (N <= 0 || N > mbnb::kMaxElems / K || (M > 0 && N > mbnb::kMaxElems / M))
        return fail(MBNB_MX_ERR_SHAPE, "mbnb_mx_linear_weight_only: N = %lld", (long long)N);
    if (M == 0) return 0;
    const bool mfma = decode_mfma(M, x_dtype);
    const int mt = mfma ? MBNB_MX_DECODE_ROWS : decode_rows(M);
    const int64_t groups = decode_grid(M, N, mt, mfma);
    if (groups > INT32_MAX)
        return fail(MBNB_MX_ERR_SHAPE, "mbnb_mx_linear_weight_only: %lld workgroups exceed one launch", (long long)groups);
    if (!x || !w_codes || !w_scales || !out) return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear_weight_only: NULL x, w_codes, w_scales or out");
    if (!mbnb::aligned(x, 16) || !mbnb::aligned(w_codes, 16))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear_weight_only: misaligned x or w_codes (16 bytes each)");
    if (!mbnb::aligned(out, mbnb::esize(out_dtype)) || (bias && !mbnb::aligned(bias, mbnb::esize(bias_dtype))))
        return fail(MBNB_MX_ERR_ARG, "mbnb_mx_linear_weight_only: misaligned out or bias (the element size each)");
    hipStream_t s = (hipStream_t)stream;
    const int st = mbnb::with_dtype(x_dtype, [&](auto t) {
        using T = decltype(t);
        if (mfma) return launch_decode_mfma<T>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
        if constexpr (sizeof(T) == 2) {
            return launch_decode<T, 1>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
        } else {
            switch (mt) {
                case 1: return launch_decode<T, 1>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
                case 2: return launch_decode<T, 2>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
                case 4: return launch_decode<T, 4>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
                default: return launch_decode<T, 8>(x, w_codes, w_scales, M, N, K, bias, bias_dtype, out, out_dtype, s);
            }
        }
    });
    if (st == 0) {
        const char *names[] = {"f16", "bf16", "f32"};
        snprintf(mbnb::last_launch(), mbnb::kLaunchBytes, mfma ? "mx_decode_mfma %s MT%d" : "mx_decode %s MT%d", names[x_dtype], mt);
    }
    return st;
}

}  // extern "C"
