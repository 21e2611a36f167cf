// mx_decode.h — the device helpers of the weight-only MXFP4 decode loop on v_mfma_f32_16x16x32, shared by
// mx_kernels.hip (k_mx_decode, k_mx_decode_mfma) and moe_kernels.hip (k_mx_experts): the E8M0 scale, the byte-table
// decode of 8 E2M1 codes to 8 values of the activation's 16-bit type, the MFMA of one MX block, and the bias load and output store
// by dtype code.  Device code only, all of it forced inline; the dtype codes are host.h's, which every public header restates.
#pragma once

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

}  // namespace mx
}  // namespace mbnb
