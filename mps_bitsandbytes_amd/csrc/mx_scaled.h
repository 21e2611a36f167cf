// mx_scaled.h — the block-scaled MFMA tile, once: what k_gemm_mx (mx_kernels.hip) and k_mx_experts_scaled
// (moemx_kernels.hip) share.  Both are a 4 x 4 grid of v_mfma_scale_f32_16x16x128_f8f6f4 accumulators per wave over the same LDS
// image of a K-step, and a pair of the expert kernel carries exactly the bits of mbnb_mx_linear.  Here, and nowhere else: the stage
// of a K-step, the 16-byte LDS-DMA, the fold of a ballot to a NaN mask, the call of the scaled MFMA and the epilogue value.  Each kernel
// keeps its own K loop (the order inside a K-step, the scale path, the edge addressing and the wait differ on purpose), its own
// store, and -- written out, because as helpers they changed both kernels' instruction streams (§35) -- the fragment reads, the
// zeros past K and the loop over the ballots; a host test holds those texts equal.  All of it forced inline.
//
// The operand map of the instruction: lane l = (g = l >> 4, fr = l & 15) holds row (A) / column (B) fr; fp4: the
// k block g as 16 bytes; fp8: registers 0..3 the 16 k from 16 g, registers 4..7 the 16 k from 64 + 16 g; scale register byte 0:
// the byte of k block g.  D: column fr, rows 4 g + r.  LDS image of a stage, in 16-byte chunks: the activation tile
// [half][row][g] (fp4: one half; fp8: chunk [h][row][g] = the 16 k from 64 h + 16 g), then the weight tile [row][g].
#pragma once

#include "mx_decode.h"

namespace mbnb {
namespace mx {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kScaledKStep = 128;      // the k of one scaled MFMA
constexpr int kScaledThreads = 256;    // four waves, each a 4 x 4 grid of 16 x 16 accumulators

// One LDS stage of a K-step: ROWS_A activation rows (fp8 if A8, else fp4) and ROWS_B fp4 weight rows.
template <bool A8, int ROWS_A, int ROWS_B> struct ScaledStage {
    static constexpr int AH = A8 ? 2 : 1;                    // 16-byte halves of an activation block
    static constexpr int A_BYTES = ROWS_A * 4 * AH * 16, B_BYTES = ROWS_B * 4 * 16, STAGE = A_BYTES + B_BYTES;
    static constexpr int NA = A_BYTES / 16 / kScaledThreads, NB = B_BYTES / 16 / kScaledThreads;   // LDS-DMA instructions per thread and stage
    static constexpr int CBSZ = A8 ? 0 : 4, BLGP = 4;        // the formats of A and B in the instruction
};

__device__ __forceinline__ void dma16(const uint8_t *src, uint8_t *wave_dst) {     // 64 lanes x 16 bytes, lane l to wave_dst + 16 l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)wave_dst, 16, 0,
                                     0);
}

// bit q of the mask: row / column q of the 16 x 16 tile has a NaN block (a lane holds row fr's scale, not its outputs' rows)
__device__ __forceinline__ uint32_t fold16(uint64_t b) { return (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xFFFFu); }

// One K-step of one accumulator: A fragment `a` under its lane's scale byte sa against B fragment `b` under sb.  ONE accumulator
// per output takes the K-steps in ascending order.  Values in and out: over arrays by reference k_mx_experts_scaled's stream changed.
template <int CBSZ, int BLGP> __device__ __forceinline__ v4f scaled_mfma(v8i a, v8i b, v4f acc, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, CBSZ, BLGP, 0, sa, 0, sb);
}

// The value of an output before its one rounding: + bias in f32, NaN if its column's bit or its row's bit (row_bit = 4 g + r of
// the A fragment's mask) is set
__device__ __forceinline__ float scaled_value(float acc, float b, bool col_nan, uint32_t a_nan, int row_bit) {
    float v = acc + b;
    if (col_nan || ((a_nan >> row_bit) & 1u)) v = __uint_as_float(0x7FC00000u);
    return v;
}

}  // namespace mx
}  // namespace mbnb
