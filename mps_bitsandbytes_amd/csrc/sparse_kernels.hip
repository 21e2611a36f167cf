// sparse_kernels.hip — the two halves of the LLM.int8 decomposition of libmbnb_sparse.so (include/mbnb_sparse.h):
//   INT8 with column + row statistics   q = rint(x * (1 / sqrt(rm[i] cm[j])) * 127),  Wd = round_T(q * (sqrt(rm[i] cm[j]) / 127))
//   COO sparse operations               dense -> COO, int8 values with one absmax scale, out = sparse . dense through a CSR form
// The MFMA work of matmul_colrow's dense route is libmbnb_hip's public mbnb_gemm_dense with the library's own plan (slices = 0); this
// file holds the passes around it and every other kernel.  Its own last-error and kernel-name records (mbnb_sparse_last_*).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/mbnb_sparse.h"
#include "common.h"
#include "host.h"

// host.h's predicates and with_dtype() take this library's dtype codes
static_assert(MBNB_SPARSE_F16 == mbnb::kF16 && MBNB_SPARSE_BF16 == mbnb::kBF16 && MBNB_SPARSE_F32 == mbnb::kF32, "dtype codes");

namespace {

using mbnb::aligned;
using mbnb::bf16_t;
using mbnb::esize;
using mbnb::f16_t;
using mbnb::fail;
using mbnb::from_f32;
using mbnb::is16;
using mbnb::kMaxElems;
using mbnb::pack2;
using mbnb::round256;
using mbnb::to_f32;
using mbnb::u32x2;
using mbnb::u32x4;
using mbnb::with_dtype;

// ---------------------------------------------------------------- small device helpers
// |v| as its bit pattern.  For non-negative floats the unsigned order of the patterns is the order of the values, +Inf above every finite
// value and every NaN above +Inf: an unsigned maximum of these patterns is torch.max of |x|, NaN propagation included.
__device__ __forceinline__ uint32_t abs_bits(float v) { return __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = umax(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}
// `.clamp(min=1e-8)` on the maximum: NaN stays NaN (the comparison is false)
__device__ __forceinline__ float clamp_absmax(uint32_t bits) {
    const float f = __builtin_bit_cast(float, bits);
    return f < 1e-8f ? 1e-8f : f;
}
// clamp(rint(p), -127, 127) as int8; 0 where p is NaN (torch's NaN -> int8 conversion on the reference's path)
__device__ __forceinline__ int code_of(float p) {
    const float r = fminf(fmaxf(rintf(p), -127.0f), 127.0f);
    return p != p ? 0 : (int)r;
}

// ---------------------------------------------------------------- the col+row rule
// s = sqrt(rm * cm), correctly rounded (sqrtf and `/` are the IEEE operations here: no fast-math, -ffp-contract=off).  Nothing of the chain
// is hoisted out of the element: 1 / s, then * 127; s / 127 is a true division.
__device__ __forceinline__ float cr_scale(float rm, float cm) { return sqrtf(rm * cm); }
__device__ __forceinline__ int cr_quant(float x, float rm, float cm) {
    const float inv = (1.0f / cr_scale(rm, cm)) * 127.0f;
    return code_of(x * inv);
}
// the f32 value of Wd before its rounding to T
__device__ __forceinline__ float cr_dequant(int q, float rm, float cm) { return (float)q * (cr_scale(rm, cm) / 127.0f); }

// Tiles of the col+row kernels: a workgroup of 256 threads covers CR_CB columns; thread t owns 8 of them -- in the vector forms the
// consecutive columns 8t .. 8t + 7 (16-byte loads), in the scalar forms the columns t + 256 e (coalesced 2- or 4-byte loads).
constexpr int CR_CB = 2048;
constexpr int CR_RB = 16;   // rows per workgroup of the statistics kernel
constexpr int CR_UN = 4;    // rows per workgroup of the quantising and dequantising kernels

template <bool VEC> __device__ __forceinline__ int64_t cr_col(int64_t cbase, int tid, int e) {
    return VEC ? cbase + (int64_t)tid * 8 + e : cbase + tid + 256 * (int64_t)e;
}

// 8 elements of row `p` (pointer to the row) as f32; columns >= C and rows switched off read as `fill`
template <typename T, bool VEC>
__device__ __forceinline__ void cr_load8(const T *__restrict__ p, bool row_ok, int64_t cbase, int tid, int64_t C, float fill, float (&v)[8]) {
    if constexpr (VEC) {
        const int64_t c0 = cbase + (int64_t)tid * 8;
        const bool ok = row_ok && c0 < C;          // C % 8 == 0: all eight or none
        if constexpr (sizeof(T) == 2) {
            const u32x4 w = ok ? *reinterpret_cast<const u32x4 *>(p + c0) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[2 * i] = ok ? mbnb::unpack_lo<T>(w[i]) : fill;
                v[2 * i + 1] = ok ? mbnb::unpack_hi<T>(w[i]) : fill;
            }
        } else {
            const mbnb::f32x4 a = ok ? *reinterpret_cast<const mbnb::f32x4 *>(p + c0) : mbnb::f32x4{fill, fill, fill, fill};
            const mbnb::f32x4 b = ok ? *reinterpret_cast<const mbnb::f32x4 *>(p + c0 + 4) : mbnb::f32x4{fill, fill, fill, fill};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = a[i];
                v[4 + i] = b[i];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t c = cr_col<false>(cbase, tid, e);
            v[e] = (row_ok && c < C) ? to_f32(p[c]) : fill;
        }
    }
}

// =====================================================================================
// k_colrow_stats: both absmax vectors from ONE read of the matrix.  A workgroup reads a CR_RB x CR_CB tile; a thread keeps the running
// maximum of each of its 8 columns and each row's maximum over those columns in registers, and the CR_RB wave reductions run after the
// last load (inside the row loop they serialised it: 78 -> 43 us for quantize_colrow at 4096 x 4096).  Results are partial: row_part
// [R, nchunk] (one value per column chunk) and col_part [nrb, C] (one row per row block), merged by k_colrow_merge.
// Maxima are taken on the bit patterns of |x| (abs_bits), so a NaN survives both reductions.
// =====================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_colrow_stats(const T *__restrict__ x, int64_t R, int64_t C, uint32_t *__restrict__ row_part,
                                                     uint32_t *__restrict__ col_part, int64_t nchunk) {
    __shared__ uint32_t srow[4][CR_RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk = blockIdx.x % nchunk, rb = blockIdx.x / nchunk;
    const int64_t cbase = chunk * CR_CB, r0 = rb * CR_RB;
    uint32_t cmx[8] = {}, rmx[CR_RB];
#pragma unroll
    for (int r = 0; r < CR_RB; r++) {      // fully unrolled: all CR_RB loads of a thread are in flight together
        const int64_t row = r0 + r;
        float v[8];
        cr_load8<T, VEC>(x + row * C, row < R, cbase, tid, C, 0.0f, v);
        uint32_t m = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t a = abs_bits(v[e]);
            cmx[e] = umax(cmx[e], a);
            m = umax(m, a);
        }
        rmx[r] = m;
    }
#pragma unroll
    for (int r = 0; r < CR_RB; r++) {      // the cross-lane reductions after the loads, CR_RB independent chains
        const uint32_t m = wave_umax(rmx[r]);
        if (lane == 0) srow[wave][r] = m;
    }
    __syncthreads();
    if (tid < CR_RB && r0 + tid < R)
        row_part[(r0 + tid) * nchunk + chunk] = umax(umax(srow[0][tid], srow[1][tid]), umax(srow[2][tid], srow[3][tid]));
    uint32_t *cp = col_part + rb * C;
    if constexpr (VEC) {
        const int64_t c0 = cbase + (int64_t)tid * 8;
        if (c0 < C) {
            *reinterpret_cast<u32x4 *>(cp + c0) = u32x4{cmx[0], cmx[1], cmx[2], cmx[3]};
            *reinterpret_cast<u32x4 *>(cp + c0 + 4) = u32x4{cmx[4], cmx[5], cmx[6], cmx[7]};
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t c = cr_col<false>(cbase, tid, e);
            if (c < C) cp[c] = cmx[e];
        }
    }
}

// The first `cblocks` workgroups merge the column partials: a workgroup takes 64 columns (a lane each, coalesced), its four waves a quarter
// of the nrb partial rows each, LDS joins the four.  The others merge the row partials, a thread per row.  `.clamp(min=1e-8)` on both.
__global__ __launch_bounds__(256) void k_colrow_merge(const uint32_t *__restrict__ row_part, const uint32_t *__restrict__ col_part, int64_t R,
                                                     int64_t C, int64_t nchunk, int64_t nrb, int64_t cblocks, float *__restrict__ rm,
                                                     float *__restrict__ cm) {
    __shared__ uint32_t sm[4][64];
    if ((int64_t)blockIdx.x < cblocks) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int64_t j = (int64_t)blockIdx.x * 64 + lane;
        uint32_t m = 0;
        if (j < C)
            for (int64_t b = wave; b < nrb; b += 4) m = umax(m, col_part[b * C + j]);
        sm[wave][lane] = m;
        __syncthreads();
        if (wave == 0 && j < C) cm[j] = clamp_absmax(umax(umax(sm[0][lane], sm[1][lane]), umax(sm[2][lane], sm[3][lane])));
        return;
    }
    const int64_t i = ((int64_t)blockIdx.x - cblocks) * 256 + threadIdx.x;
    if (i < R) {
        uint32_t m = 0;
        for (int64_t k = 0; k < nchunk; k++) m = umax(m, row_part[i * nchunk + k]);
        rm[i] = clamp_absmax(m);
    }
}

// =====================================================================================
// k_colrow_quantize: the second read.  A thread takes its 8 columns of CR_UN consecutive rows: cm[] once, then per row one 16-byte load
// (two for f32), eight times the chain sqrt -> 1 / s -> * 127 -> x * inv -> rint -> clamp, and one 8-byte store of the codes.
// =====================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_colrow_quantize(const T *__restrict__ x, const float *__restrict__ rm, const float *__restrict__ cm,
                                                        int64_t R, int64_t C, int8_t *__restrict__ q, int64_t nchunk) {
    const int tid = threadIdx.x;
    const int64_t cbase = (blockIdx.x % nchunk) * CR_CB, r0 = (blockIdx.x / nchunk) * CR_UN;
    if (cr_col<VEC>(cbase, tid, 0) >= C) return;
    float c[8];
    cr_load8<float, VEC>(cm, true, cbase, tid, C, 1.0f, c);
    float v[CR_UN][8];
#pragma unroll
    for (int u = 0; u < CR_UN; u++) cr_load8<T, VEC>(x + (r0 + u) * C, r0 + u < R, cbase, tid, C, 0.0f, v[u]);
#pragma unroll
    for (int u = 0; u < CR_UN; u++) {
        const int64_t row = r0 + u;
        if (row >= R) break;
        const float r = rm[row];
        int code[8];
#pragma unroll
        for (int e = 0; e < 8; e++) code[e] = cr_quant(v[u][e], r, c[e]);
        int8_t *dst = q + row * C;
        if constexpr (VEC) {
            u32x2 o;
#pragma unroll
            for (int h = 0; h < 2; h++)
                o[h] = (uint32_t)(code[4 * h] & 0xFF) | ((uint32_t)(code[4 * h + 1] & 0xFF) << 8) | ((uint32_t)(code[4 * h + 2] & 0xFF) << 16) |
                       ((uint32_t)(code[4 * h + 3] & 0xFF) << 24);
            *reinterpret_cast<u32x2 *>(dst + cbase + (int64_t)tid * 8) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t cc = cr_col<false>(cbase, tid, e);
                if (cc < C) dst[cc] = (int8_t)code[e];
            }
        }
    }
}

// =====================================================================================
// k_colrow_dequant: Wd [R, C] in T.  Same tiling; one 8-byte load of codes and one 16-byte store (two for f32) per row in the vector form.
// from_f32 / pack2 round the f32 product that already exists (no mixed-precision fma): the reference's `.to(dtype)` of an f32 tensor.
// Stores are write-through ("sc1") where the dense GEMM reads Wd next.
// =====================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_colrow_dequant(const int8_t *__restrict__ q, const float *__restrict__ rm, const float *__restrict__ cm,
                                                       int64_t R, int64_t C, T *__restrict__ out, int64_t nchunk, int write_through) {
    const int tid = threadIdx.x;
    const int64_t cbase = (blockIdx.x % nchunk) * CR_CB, r0 = (blockIdx.x / nchunk) * CR_UN;
    if (cr_col<VEC>(cbase, tid, 0) >= C) return;
    float c[8];
    cr_load8<float, VEC>(cm, true, cbase, tid, C, 1.0f, c);
    if constexpr (VEC) {
        const int64_t c0 = cbase + (int64_t)tid * 8;
        u32x2 w[CR_UN];
#pragma unroll
        for (int u = 0; u < CR_UN; u++) w[u] = r0 + u < R ? *reinterpret_cast<const u32x2 *>(q + (r0 + u) * C + c0) : u32x2{0u, 0u};
#pragma unroll
        for (int u = 0; u < CR_UN; u++) {
            const int64_t row = r0 + u;
            if (row >= R) break;
            const float r = rm[row];
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; e++) f[e] = cr_dequant((int)(int8_t)(w[u][e >> 2] >> (8 * (e & 3))), r, c[e]);
            T *dst = out + row * C + c0;
            if constexpr (sizeof(T) == 2) {
                const u32x4 o = {pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7])};
                // s_nop inside the string: hipcc does not know this is a store of more than 64 bits, whose data registers the next VALU write must leave alone
                if (write_through) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(o) : "memory");
                else *reinterpret_cast<u32x4 *>(dst) = o;
            } else {
                *reinterpret_cast<mbnb::f32x4 *>(dst) = mbnb::f32x4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<mbnb::f32x4 *>(dst + 4) = mbnb::f32x4{f[4], f[5], f[6], f[7]};
            }
        }
    } else {
        for (int u = 0; u < CR_UN; u++) {
            const int64_t row = r0 + u;
            if (row >= R) break;
            const float r = rm[row];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t cc = cr_col<false>(cbase, tid, e);
                if (cc < C) out[row * C + cc] = from_f32<T>(cr_dequant(q[row * C + cc], r, c[e]));
            }
        }
    }
}

// =====================================================================================
// Generic matmul_colrow kernel (the shape of libmbnb_train's generic forward): a wave owns one output column n and CR_GM rows m; its lanes
// stride over k, decode Wd[n, k] with the rule above (rounded to T), accumulate in f32, reduce across the wave, add the bias in f32 and
// round ONCE.  Any shape, dtype, alignment and M.  Workgroups are numbered flat: 4 columns x CR_GM rows each.
// =====================================================================================
constexpr int CR_GM = 8;

template <typename T>
__global__ __launch_bounds__(256) void k_colrow_generic(const T *__restrict__ X, int64_t M, int64_t K, const int8_t *__restrict__ W,
                                                       const float *__restrict__ rm, const float *__restrict__ cm, int64_t N,
                                                       const T *__restrict__ bias, T *__restrict__ out, int64_t n_groups) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)(blockIdx.x % n_groups) * 4 + wave;
    const int64_t m0 = (int64_t)(blockIdx.x / n_groups) * CR_GM;
    if (n >= N) return;
    const float r = rm[n];
    const int8_t *wr = W + n * K;
    const T *x[CR_GM];
#pragma unroll
    for (int i = 0; i < CR_GM; i++) x[i] = X + (m0 + i < M ? m0 + i : M - 1) * K;
    float acc[CR_GM] = {};
    for (int64_t k = lane; k < K; k += 64) {
        const float w = to_f32(from_f32<T>(cr_dequant(wr[k], r, cm[k])));
#pragma unroll
        for (int i = 0; i < CR_GM; i++) acc[i] = fmaf(to_f32(x[i][k]), w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < CR_GM; i++) acc[i] = mbnb::wave_sum(acc[i]);
    if (lane < CR_GM && m0 + lane < M) {
        float v = acc[0];
#pragma unroll
        for (int i = 1; i < CR_GM; i++)
            if (lane == i) v = acc[i];
        if (bias) v += to_f32(bias[n]);
        out[(m0 + lane) * N + n] = from_f32<T>(v);
    }
}

// =====================================================================================
// sparse_coo_from_dense.  keep(x): threshold off -> x != 0; on -> |x| >= threshold, or x is NaN (the reference multiplies by the mask:
// NaN * 0 is NaN, which is != 0; -x * 0 is -0.0, which is not).  A wave owns a row and walks it 64 columns at a time.
// =====================================================================================
template <typename T> __device__ __forceinline__ bool coo_keep(T x, float thr) {
    const float f = to_f32(x);
    return thr > 0.0f ? (fabsf(f) >= thr || f != f) : (f != 0.0f);
}

// counts[r + 1] = kept elements of row r, for the scan that follows (counts = row_ptr)
template <typename T>
__global__ __launch_bounds__(256) void k_coo_count(const T *__restrict__ x, int64_t R, int64_t C, float thr, int64_t *__restrict__ row_ptr) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const T *p = x + r * C;
    int64_t n = 0;
    for (int64_t c0 = 0; c0 < C; c0 += 64) {
        const int64_t c = c0 + lane;
        n += __popcll(__ballot(c < C && coo_keep<T>(p[c < C ? c : 0], thr)));
    }
    if (lane == 0) row_ptr[r + 1] = n;
}

// In-place exclusive scan of a[0 .. n]: on entry a[i + 1] holds the count of item i, on exit a[i] the sum of the counts before item i
// and a[n] the total.  ONE workgroup of 1024 threads: a contiguous share per thread, the shares' sums scanned in LDS.  `gate`: an
// optional device flag; the kernel returns at once when *gate == 0.
template <typename I>
__global__ __launch_bounds__(1024) void k_scan_counts(I *__restrict__ a, int64_t n, const int *__restrict__ gate) {
    if (gate && *gate == 0) return;
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = (int64_t)t * per, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; i++) s += (int64_t)a[i + 1];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int64_t run = part[t] - s;      // sum of every share before this one
    if (t == 0) a[0] = 0;
    for (int64_t i = lo; i < hi; i++) {
        run += (int64_t)a[i + 1];
        a[i + 1] = (I)run;
    }
}

// the ordered fill: the kept elements of row r go to row_ptr[r] .. in column order (ballot + prefix count inside each 64-column step)
template <typename T>
__global__ __launch_bounds__(256) void k_coo_fill(const T *__restrict__ x, int64_t R, int64_t C, float thr, const int64_t *__restrict__ row_ptr,
                                                 int64_t *__restrict__ row, int64_t *__restrict__ col, T *__restrict__ values, int64_t nnz) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const T *p = x + r * C;
    int64_t base = row_ptr[r];
    for (int64_t c0 = 0; c0 < C; c0 += 64) {
        const int64_t c = c0 + lane;
        const T v = p[c < C ? c : 0];
        const bool keep = c < C && coo_keep<T>(v, thr);
        const unsigned long long mask = __ballot(keep);
        const int64_t o = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && o < nnz) {      // o < nnz: the counts were taken from the same data; the check keeps a changed input inside the outputs
            row[o] = r;
            col[o] = c;
            values[o] = v;
        }
        base += __popcll(mask);
    }
}

// =====================================================================================
// quantize_sparse_coo.  k_coo_absmax: up to COO_QP workgroups, each the maximum of |v| bits over a grid-strided share -> part[].
// k_coo_quantize: every workgroup merges the partials itself (at most 4 KiB, from L2), so the maximum never leaves the device and no
// workgroup waits for another; workgroup 0 writes the scale.
// =====================================================================================
constexpr int COO_QP = 1024;

template <typename T>
__global__ __launch_bounds__(256) void k_coo_absmax(const T *__restrict__ v, int64_t nnz, uint32_t *__restrict__ part) {
    __shared__ uint32_t sm[4];
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) m = umax(m, abs_bits(to_f32(v[i])));
    m = wave_umax(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = umax(umax(sm[0], sm[1]), umax(sm[2], sm[3]));
}

template <typename T>
__global__ __launch_bounds__(256) void k_coo_quantize(const T *__restrict__ v, int64_t nnz, const uint32_t *__restrict__ part, int nparts,
                                                     int8_t *__restrict__ q, float *__restrict__ scale_out) {
    __shared__ uint32_t sm[4];
    uint32_t m = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) m = umax(m, part[i]);
    m = wave_umax(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    const float scale = clamp_absmax(umax(umax(sm[0], sm[1]), umax(sm[2], sm[3]))) / 127.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = scale;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) q[i] = (int8_t)code_of(to_f32(v[i]) / scale);
}

// =====================================================================================
// COO -> CSR on the device.  Workspace: flag (int32; 0: `row` is non-decreasing), row_ptr int32 [rows + 1], cursor int32 [rows], perm int32 [nnz];
// flag, row_ptr and cursor are zeroed by a memset node in front.  The kernels of the path not taken return on the flag.
// =====================================================================================
__device__ __forceinline__ int64_t ld_index(const void *p, int bits, int64_t e) {
    return bits == 32 ? (int64_t) static_cast<const int32_t *>(p)[e] : static_cast<const int64_t *>(p)[e];
}

// flag = 1 where some row[e] > row[e + 1] (every writer writes the same value), or where the caller forces the general path
__global__ __launch_bounds__(256) void k_coo_flag(const void *__restrict__ row, int bits, int64_t nnz, int *__restrict__ flag, int force) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (force) {
        if (e == 0) atomicOr(flag, 1);
        return;
    }
    if (e + 1 < nnz && ld_index(row, bits, e) > ld_index(row, bits, e + 1)) atomicOr(flag, 1);
}

// sorted path: row_ptr[i] = the first entry whose row is >= i (entries of rows < 0 lie before row_ptr[0], of rows >= `rows` after row_ptr[rows])
__global__ __launch_bounds__(256) void k_coo_search(const void *__restrict__ row, int bits, int64_t nnz, int64_t rows, const int *__restrict__ flag,
                                                   int *__restrict__ row_ptr) {
    if (*flag != 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > rows) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ld_index(row, bits, mid) < i) lo = mid + 1;
        else hi = mid;
    }
    row_ptr[i] = (int)lo;
}

// general path, 1: counts[r + 1] += 1 per entry of an in-range row (integer atomics: the sums do not depend on the order of arrival)
__global__ __launch_bounds__(256) void k_coo_hist(const void *__restrict__ row, int bits, int64_t nnz, int64_t rows, const int *__restrict__ flag,
                                                 int *__restrict__ row_ptr) {
    if (*flag == 0) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int64_t r = ld_index(row, bits, e);
    if (r >= 0 && r < rows) atomicAdd(row_ptr + r + 1, 1);
}

// general path, 3 (after k_scan_counts): entry e takes the next free slot of its row's segment.  The slot depends on arrival order; the set of
// entries in the segment does not, and k_coo_sort puts it in order.
__global__ __launch_bounds__(256) void k_coo_scatter(const void *__restrict__ row, int bits, int64_t nnz, int64_t rows, const int *__restrict__ flag,
                                                    const int *__restrict__ row_ptr, int *__restrict__ cursor, int *__restrict__ perm) {
    if (*flag == 0) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int64_t r = ld_index(row, bits, e);
    if (r < 0 || r >= rows) return;
    const int64_t slot = (int64_t)row_ptr[r] + atomicAdd(cursor + r, 1);
    if (slot < nnz) perm[slot] = (int)e;
}

// general path, 4: a workgroup sorts one row's segment of perm ascending (= by original entry index).  A bitonic network in which every
// comparator puts the smaller value at the lower index (the first step of each merge pairs i with its mirror image i ^ (k - 1)), so a
// segment of any length L sorts like one padded with +infinity to a power of two: comparators that reach past L are skipped.  Segments
// of up to COO_SORT_LDS values are sorted in LDS, longer ones in place in global memory (workgroup barriers order both).
constexpr int COO_SORT_LDS = 4096;

__device__ __forceinline__ void coo_cmpx(int *a, int64_t i, int64_t l, int64_t L) {
    if (l > i && l < L) {
        const int x = a[i], y = a[l];
        if (x > y) {
            a[i] = y;
            a[l] = x;
        }
    }
}

__global__ __launch_bounds__(256) void k_coo_sort(const int *__restrict__ flag, const int *__restrict__ row_ptr, int *perm) {
    if (*flag == 0) return;
    __shared__ int lds[COO_SORT_LDS];
    const int64_t start = row_ptr[blockIdx.x], L = (int64_t)row_ptr[blockIdx.x + 1] - start;
    if (L < 2) return;
    const bool in_lds = L <= COO_SORT_LDS;
    int *seg = perm + start;
    int *a = in_lds ? lds : seg;
    if (in_lds) {
        for (int64_t i = threadIdx.x; i < L; i += 256) lds[i] = seg[i];
    }
    __syncthreads();
    for (int64_t k = 2; (k >> 1) < L; k <<= 1) {
        for (int64_t i = threadIdx.x; i < L; i += 256) coo_cmpx(a, i, i ^ (k - 1), L);
        __syncthreads();
        for (int64_t j = k >> 2; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < L; i += 256) coo_cmpx(a, i, i ^ j, L);
            __syncthreads();
        }
    }
    if (in_lds) {
        for (int64_t i = threadIdx.x; i < L; i += 256) seg[i] = lds[i];
    }
}

// =====================================================================================
// k_spmm_csr: out[i, :] = sum over row i's entries, in entry order, of val(e) * dense[col[e], :].  A group of G lanes (16, 32 or a whole wave,
// chosen on the host from N) owns one output row and one column tile of G * CPL columns; a lane keeps CPL f32 accumulators.  The row's
// entry list is read once per tile (every lane of the group reads the same address); rows of `dense` come in with 16-byte loads in the
// vector form (CPL = 16 / sizeof(T) consecutive columns per lane), with coalesced element loads in the scalar form (CPL = 4 columns, G apart).
// Four entries are in flight per step; their products are added in entry order with fmaf, so the result is a function of the inputs alone.
// Entries are p itself on the sorted path and perm[p] on the general path (the device flag says which).
// =====================================================================================
template <typename T> __device__ __forceinline__ float coo_value(const void *values, int kind, const float *scale, int64_t e) {
    if (kind == MBNB_COO_VALUES) return to_f32(static_cast<const T *>(values)[e]);
    const float q = (float)static_cast<const int8_t *>(values)[e];
    const float s = kind == MBNB_COO_INT8_SCALAR ? scale[0] : to_f32(from_f32<T>(scale[e]));
    return to_f32(from_f32<T>(q * s));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_spmm_csr(const int *__restrict__ flag, const int *__restrict__ row_ptr, const int *__restrict__ perm,
                                                 const void *__restrict__ col, int col_bits, const void *__restrict__ values, int kind,
                                                 const float *__restrict__ scale, const T *__restrict__ dense, int64_t rows, int64_t cols,
                                                 int64_t N, T *__restrict__ out, int G, int64_t ntile) {
    constexpr int CPL = VEC ? 16 / (int)sizeof(T) : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    const int64_t tile = blockIdx.x % ntile, rblk = blockIdx.x / ntile;
    const int64_t row = (rblk * 4 + wave) * (64 / G) + sub;
    const int64_t c0 = tile * G * CPL;
    int64_t cc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; j++) cc[j] = VEC ? c0 + (int64_t)gl * CPL + j : c0 + gl + (int64_t)G * j;
    if (row >= rows || cc[0] >= N) return;
    const bool use_perm = *flag != 0;
    const int64_t start = row_ptr[row], end = row_ptr[row + 1];
    float acc[CPL] = {};
    for (int64_t p = start; p < end; p += 4) {
        float v[4], d[4][CPL];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ok[u] = p + u < end;
            const int64_t e = ok[u] ? (use_perm ? (int64_t)perm[p + u] : p + u) : 0;
            const int64_t c = ok[u] ? ld_index(col, col_bits, e) : -1;
            ok[u] = ok[u] && c >= 0 && c < cols;
            v[u] = ok[u] ? coo_value<T>(values, kind, scale, e) : 0.0f;
            const T *dr = dense + (ok[u] ? c : 0) * N;
            if constexpr (VEC) {
                if constexpr (sizeof(T) == 2) {
                    const u32x4 w = ok[u] ? *reinterpret_cast<const u32x4 *>(dr + cc[0]) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        d[u][2 * j] = mbnb::unpack_lo<T>(w[j]);
                        d[u][2 * j + 1] = mbnb::unpack_hi<T>(w[j]);
                    }
                } else {
                    const mbnb::f32x4 w = ok[u] ? *reinterpret_cast<const mbnb::f32x4 *>(dr + cc[0]) : mbnb::f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < 4; j++) d[u][j] = w[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < CPL; j++) d[u][j] = (ok[u] && cc[j] < N) ? to_f32(dr[cc[j]]) : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!ok[u]) continue;
#pragma unroll
            for (int j = 0; j < CPL; j++) acc[j] = fmaf(v[u], d[u][j], acc[j]);
        }
    }
    T *o = out + row * N;
    if constexpr (VEC) {
        if constexpr (sizeof(T) == 2) {
            *reinterpret_cast<u32x4 *>(o + cc[0]) = u32x4{pack2<T>(acc[0], acc[1]), pack2<T>(acc[2], acc[3]), pack2<T>(acc[4], acc[5]), pack2<T>(acc[6], acc[7])};
        } else {
            *reinterpret_cast<mbnb::f32x4 *>(o + cc[0]) = mbnb::f32x4{acc[0], acc[1], acc[2], acc[3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; j++)
            if (cc[j] < N) o[cc[j]] = from_f32<T>(acc[j]);
    }
}

// ------------------------------------------------------------------------------------- host side
// Every name mbnb_sparse_last_kernel() can report (tests/int8_decomp_cases.py has a GPU case for each).
enum { KN_CR_Q8, KN_CR_Q1, KN_CR_DQ8, KN_CR_DQ1, KN_CR_DENSE, KN_CR_GENERIC, KN_COO_COUNT, KN_COO_FILL, KN_COO_QUANT, KN_SPMM8, KN_SPMM1, KN_SPMM8_GEN,
       KN_SPMM1_GEN };
const char *const kSparseKernelNames[] = {"colrow_quantize8", "colrow_quantize1", "colrow_dequant8", "colrow_dequant1", "colrow_dq+dense", "colrow_generic",
                                          "coo_count", "coo_fill", "coo_quantize", "spmm_coo8", "spmm_coo1", "spmm_coo8_general", "spmm_coo1_general"};

thread_local const char *g_kernel = "";

// The variant of the last call: what the name does not say about the kernel forms that ran ("wt", "parts1024", "G16 x2"; tests/
// int8_decomp_cases.py restates the conditions).  mbnb_sparse_last_kernel() hands out name and variant in one buffer (name, NUL, variant,
// NUL).  The variant of the "+dense" route's GEMM stays in libmbnb_hip's own record.
thread_local char g_variant[64] = "";
thread_local char g_kernel_out[128] = "";

void set_variant(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void set_variant(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_variant, sizeof(g_variant), fmt, ap);
    va_end(ap);
}
// every launching entry point begins with this: a call whose launcher sets no variant reports "", never the previous call's
void begin_call() { g_variant[0] = '\0'; }

// a failed launch leaves the record as every failing call leaves it: the last successful call's name, no variant
int launched(const char *what, int name) {
    if (int rc = mbnb::launch_status(what)) {
        g_variant[0] = '\0';
        return rc;
    }
    g_kernel = kSparseKernelNames[name];
    return MBNB_SPARSE_OK;
}

bool dtype_ok(int dtype) { return dtype >= MBNB_SPARSE_F16 && dtype <= MBNB_SPARSE_F32; }
constexpr int64_t kMaxGrid = 0x7FFFFFFF;

// ---- col + row
int64_t cr_chunks(int64_t C) { return (C + CR_CB - 1) / CR_CB; }
int64_t cr_row_blocks(int64_t R) { return (R + CR_RB - 1) / CR_RB; }
int64_t cr_quantize_ws(int64_t R, int64_t C) { return round256(R * cr_chunks(C) * 4) + round256(cr_row_blocks(R) * C * 4); }

template <typename T>
int cr_dequant_launch(const int8_t *q, const float *rm, const float *cm, int64_t R, int64_t C, T *out, int write_through, hipStream_t st) {
    const int64_t nchunk = cr_chunks(C), blocks = nchunk * ((R + CR_UN - 1) / CR_UN);
    if (blocks > kMaxGrid) return fail(MBNB_SPARSE_ERR_UNSUPPORTED, "colrow_dequantize: %lld workgroups exceed one launch", (long long)blocks);
    if (C % 8 == 0 && aligned(q, 8) && aligned(cm, 16) && aligned(out, 16)) {
        hipLaunchKernelGGL((k_colrow_dequant<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, q, rm, cm, R, C, out, nchunk, write_through);
        if (write_through && sizeof(T) == 2) set_variant("wt");      // the store that goes through to memory (the f32 form has none)
        return launched("colrow_dequantize", KN_CR_DQ8);
    }
    hipLaunchKernelGGL((k_colrow_dequant<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, q, rm, cm, R, C, out, nchunk, 0);
    return launched("colrow_dequantize", KN_CR_DQ1);
}

// Route thresholds of matmul_colrow: libmbnb_train's SwitchBack forward's (train_kernels.hip kSbDenseMacs / kSbBigWeight), the same structure
// (a decode pass into the workspace + mbnb_gemm_dense against one generic kernel).
constexpr int64_t kCrDenseMacs = (int64_t)1 << 27, kCrBigWeight = (int64_t)1 << 25;

bool cr_dense_shape(int64_t M, int64_t N, int64_t K, int dtype) {
    return is16(dtype) && M > 0 && N > 0 && K % 64 == 0 && K >= 128 && 256 * K * 2 < ((int64_t)1 << 31) && M * N * 4 < ((int64_t)1 << 40) &&
           M * N * K >= kCrDenseMacs && (M >= 16 || N * K >= kCrBigWeight);
}

template <typename T>
int cr_matmul(const T *X, int64_t M, int64_t K, const int8_t *W, const float *rm, const float *cm, int64_t N, const T *bias, T *out, void *ws,
              int64_t ws_bytes, int flags, hipStream_t st) {
    const int64_t wd_bytes = round256(N * K * 2);
    const bool dense = !(flags & MBNB_SPARSE_FORCE_GENERIC) && cr_dense_shape(M, N, K, sizeof(T) == 2 ? MBNB_SPARSE_F16 : MBNB_SPARSE_F32) &&
                       ws != nullptr && aligned(ws, 256) && ws_bytes >= wd_bytes + mbnb_gemm_dense_workspace_bytes(M, N, K) && aligned(X, 16) && aligned(W, 8) && aligned(cm, 16) && aligned(out, 16);
    if constexpr (sizeof(T) == 2) if (dense) {
        T *wd = static_cast<T *>(ws);
        if (int rc = cr_dequant_launch<T>(W, rm, cm, N, K, wd, 1, st)) return rc;
        const int dt = std::is_same<T, f16_t>::value ? MBNB_F16 : MBNB_BF16;
        char *part = static_cast<char *>(ws) + wd_bytes;
        const int rc = mbnb_gemm_dense(X, wd, dt, bias, dt, out, M, N, K, K, part, ws_bytes - wd_bytes, 0, st);
        if (rc != 0) {
            g_variant[0] = '\0';
            return fail(rc, "colrow_matmul: mbnb_gemm_dense failed: %s", mbnb_last_error());
        }
        g_kernel = kSparseKernelNames[KN_CR_DENSE];
        return MBNB_SPARSE_OK;
    }
    const int64_t n_groups = (N + 3) / 4, blocks = n_groups * ((M + CR_GM - 1) / CR_GM);
    if (blocks > kMaxGrid) return fail(MBNB_SPARSE_ERR_UNSUPPORTED, "colrow_matmul: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL(k_colrow_generic<T>, dim3((unsigned)blocks), dim3(256), 0, st, X, M, K, W, rm, cm, N, bias, out, n_groups);
    return launched("colrow_matmul(generic)", KN_CR_GENERIC);
}

// ---- spmm: workspace layout
struct SpmmWs {
    int64_t flag_bytes, ptr_bytes, cursor_bytes, perm_bytes;
    int64_t zeroed() const { return flag_bytes + ptr_bytes + cursor_bytes; }
    int64_t total() const { return zeroed() + perm_bytes; }
};
SpmmWs spmm_ws(int64_t nnz, int64_t rows) { return SpmmWs{256, round256((rows + 1) * 4), round256(rows * 4), round256(nnz * 4)}; }
constexpr int64_t kMaxIndex = 0x7FFFFFFE;

}  // namespace

extern "C" {

int mbnb_sparse_abi_version(void) { return MBNB_SPARSE_ABI_VERSION; }
const char *mbnb_sparse_last_error(void) { return mbnb::last_error(); }
const char *mbnb_sparse_last_kernel(void) {
    const size_t n = strlen(g_kernel) + 1;
    memcpy(g_kernel_out, g_kernel, n);
    memcpy(g_kernel_out + n, g_variant, strlen(g_variant) + 1);
    return g_kernel_out;
}

// --------------------------------------------------------------------------- col + row
int64_t mbnb_colrow_quantize_workspace_bytes(int64_t R, int64_t C) {
    if (R <= 0 || C <= 0 || R > kMaxElems / C) return 0;
    return cr_quantize_ws(R, C);
}

int mbnb_colrow_quantize(const void *x, int dtype, int64_t R, int64_t C, int8_t *q, float *row_absmax, float *col_absmax, void *workspace,
                         int64_t workspace_bytes, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "colrow_quantize: unknown dtype %d", dtype);
    if (R < 0 || C < 0) return fail(MBNB_SPARSE_ERR_ARG, "colrow_quantize: negative size");
    if (C > 0 && R > kMaxElems / C) return fail(MBNB_SPARSE_ERR_SHAPE, "colrow_quantize: problem too large");
    if (R == 0 || C == 0) return fail(MBNB_SPARSE_ERR_SHAPE, "colrow_quantize: the maximum of an empty row or column is undefined (R = %lld, C = %lld)",
                                      (long long)R, (long long)C);
    if (!x || !q || !row_absmax || !col_absmax) return fail(MBNB_SPARSE_ERR_ARG, "colrow_quantize: NULL pointer");
    if (!aligned(x, esize(dtype)) || !aligned(row_absmax, 4) || !aligned(col_absmax, 4))
        return fail(MBNB_SPARSE_ERR_ARG, "colrow_quantize: x and the statistics must be aligned to their element size");
    const int64_t need = cr_quantize_ws(R, C);
    if (!workspace || !aligned(workspace, 256) || workspace_bytes < need)
        return fail(MBNB_SPARSE_ERR_ARG, "colrow_quantize: needs a 256-byte aligned workspace of %lld bytes", (long long)need);
    const int64_t nchunk = cr_chunks(C), nrb = cr_row_blocks(R);
    const int64_t b_stats = nchunk * nrb, b_quant = nchunk * ((R + CR_UN - 1) / CR_UN), cblocks = (C + 63) / 64, b_merge = cblocks + (R + 255) / 256;
    if (b_stats > kMaxGrid || b_quant > kMaxGrid || b_merge > kMaxGrid) return fail(MBNB_SPARSE_ERR_UNSUPPORTED, "colrow_quantize: too many workgroups for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t *row_part = static_cast<uint32_t *>(workspace);
    uint32_t *col_part = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + round256(R * nchunk * 4));
    const bool vec = C % 8 == 0 && aligned(x, 16) && aligned(col_absmax, 16) && aligned(q, 8);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        const T *xt = static_cast<const T *>(x);
        if (vec) hipLaunchKernelGGL((k_colrow_stats<T, true>), dim3((unsigned)b_stats), dim3(256), 0, st, xt, R, C, row_part, col_part, nchunk);
        else hipLaunchKernelGGL((k_colrow_stats<T, false>), dim3((unsigned)b_stats), dim3(256), 0, st, xt, R, C, row_part, col_part, nchunk);
        hipLaunchKernelGGL(k_colrow_merge, dim3((unsigned)b_merge), dim3(256), 0, st, row_part, col_part, R, C, nchunk, nrb, cblocks, row_absmax, col_absmax);
        if (vec) hipLaunchKernelGGL((k_colrow_quantize<T, true>), dim3((unsigned)b_quant), dim3(256), 0, st, xt, row_absmax, col_absmax, R, C, q, nchunk);
        else hipLaunchKernelGGL((k_colrow_quantize<T, false>), dim3((unsigned)b_quant), dim3(256), 0, st, xt, row_absmax, col_absmax, R, C, q, nchunk);
        return launched("colrow_quantize", vec ? KN_CR_Q8 : KN_CR_Q1);
    });
}

int mbnb_colrow_dequantize(const int8_t *q, const float *row_scales, const float *col_scales, int64_t R, int64_t C, int dtype, void *out,
                           void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "colrow_dequantize: unknown dtype %d", dtype);
    if (R < 0 || C < 0) return fail(MBNB_SPARSE_ERR_ARG, "colrow_dequantize: negative size");
    if (C > 0 && R > kMaxElems / C) return fail(MBNB_SPARSE_ERR_SHAPE, "colrow_dequantize: problem too large");
    const bool vec_shape = C % 8 == 0;
    if (R == 0 || C == 0) {
        g_kernel = kSparseKernelNames[vec_shape ? KN_CR_DQ8 : KN_CR_DQ1];
        return MBNB_SPARSE_OK;
    }
    if (!q || !row_scales || !col_scales || !out) return fail(MBNB_SPARSE_ERR_ARG, "colrow_dequantize: NULL pointer");
    if (!aligned(out, esize(dtype)) || !aligned(row_scales, 4) || !aligned(col_scales, 4))
        return fail(MBNB_SPARSE_ERR_ARG, "colrow_dequantize: out and the scales must be aligned to their element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return cr_dequant_launch<T>(q, row_scales, col_scales, R, C, static_cast<T *>(out), 0, st);
    });
}

int64_t mbnb_colrow_matmul_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!dtype_ok(dtype) || M <= 0 || N <= 0 || K <= 0 || M > kMaxElems / K || N > kMaxElems / K || M > kMaxElems / N) return 0;
    if (!cr_dense_shape(M, N, K, dtype)) return 0;
    return round256(N * K * 2) + mbnb_gemm_dense_workspace_bytes(M, N, K);
}

int mbnb_colrow_matmul(const void *X, int dtype, int64_t M, int64_t K, const int8_t *W, const float *row_scales, const float *col_scales, int64_t N,
                       const void *bias, void *out, void *workspace, int64_t workspace_bytes, int flags, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: unknown dtype %d", dtype);
    if (flags & ~(MBNB_SPARSE_PASS_ONLY | MBNB_SPARSE_FORCE_GENERIC)) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: unknown flags 0x%x", flags);
    if (flags & MBNB_SPARSE_PASS_ONLY) {     // the pass as the dense route runs it: write-through stores where the vector form applies
        if (N < 0 || K < 0) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: negative size");
        if (N == 0 || K == 0 || (K > 0 && N > kMaxElems / K) || !W || !row_scales || !col_scales || !out || !aligned(out, esize(dtype)) ||
            !aligned(row_scales, 4) || !aligned(col_scales, 4))
            return mbnb_colrow_dequantize(W, row_scales, col_scales, N, K, dtype, out, stream);      // its checks, its messages
        return with_dtype(dtype, [&](auto tag) {
            using T = decltype(tag);
            return cr_dequant_launch<T>(W, row_scales, col_scales, N, K, static_cast<T *>(out), 1, static_cast<hipStream_t>(stream));
        });
    }
    if (M < 0 || N < 0 || K < 0) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: negative size");
    if ((K > 0 && (N > kMaxElems / K || M > kMaxElems / K)) || (N > 0 && M > kMaxElems / N)) return fail(MBNB_SPARSE_ERR_SHAPE, "colrow_matmul: problem too large");
    if (workspace_bytes < 0) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: negative workspace size");
    if (N == 0 || M == 0) {
        g_kernel = kSparseKernelNames[KN_CR_GENERIC];
        return MBNB_SPARSE_OK;
    }
    if (K == 0) return fail(MBNB_SPARSE_ERR_SHAPE, "colrow_matmul: K = 0 with outputs to write");
    if (!X || !W || !row_scales || !col_scales || !out) return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: NULL pointer");
    if (!aligned(out, esize(dtype)) || !aligned(X, esize(dtype)) || (bias && !aligned(bias, esize(dtype))) || !aligned(row_scales, 4) || !aligned(col_scales, 4))
        return fail(MBNB_SPARSE_ERR_ARG, "colrow_matmul: X, bias, out and the scales must be aligned to their element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return cr_matmul<T>(static_cast<const T *>(X), M, K, W, row_scales, col_scales, N, static_cast<const T *>(bias), static_cast<T *>(out), workspace,
                            workspace_bytes, flags, st);
    });
}

// --------------------------------------------------------------------------- dense -> COO
int mbnb_coo_count(const void *x, int dtype, int64_t R, int64_t C, float threshold, int64_t *row_ptr, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "coo_count: unknown dtype %d", dtype);
    if (R < 0 || C < 0) return fail(MBNB_SPARSE_ERR_ARG, "coo_count: negative size");
    if (C > 0 && R > kMaxElems / C) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_count: problem too large");
    if (R > kMaxIndex * 4) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_count: too many rows for one launch");
    if (threshold != threshold) return fail(MBNB_SPARSE_ERR_ARG, "coo_count: the threshold is NaN");
    if (!row_ptr || (R > 0 && C > 0 && !x)) return fail(MBNB_SPARSE_ERR_ARG, "coo_count: NULL pointer");
    if (!aligned(row_ptr, 8) || !aligned(x, esize(dtype))) return fail(MBNB_SPARSE_ERR_ARG, "coo_count: x and row_ptr must be aligned to their element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (R > 0) hipLaunchKernelGGL(k_coo_count<T>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, static_cast<const T *>(x), R, C, threshold, row_ptr);
        hipLaunchKernelGGL(k_scan_counts<int64_t>, dim3(1), dim3(1024), 0, st, row_ptr, R, (const int *)nullptr);
        return launched("coo_count", KN_COO_COUNT);
    });
}

int mbnb_coo_fill(const void *x, int dtype, int64_t R, int64_t C, float threshold, const int64_t *row_ptr, int64_t *row, int64_t *col, void *values,
                  int64_t nnz, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "coo_fill: unknown dtype %d", dtype);
    if (R < 0 || C < 0 || nnz < 0) return fail(MBNB_SPARSE_ERR_ARG, "coo_fill: negative size");
    if (C > 0 && (R > kMaxElems / C || nnz > R * C)) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_fill: problem too large, or more entries than elements");
    if (R > kMaxIndex * 4) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_fill: too many rows for one launch");
    if (threshold != threshold) return fail(MBNB_SPARSE_ERR_ARG, "coo_fill: the threshold is NaN");
    if (nnz == 0 || R == 0 || C == 0) {
        g_kernel = kSparseKernelNames[KN_COO_FILL];
        return MBNB_SPARSE_OK;
    }
    if (!x || !row_ptr || !row || !col || !values) return fail(MBNB_SPARSE_ERR_ARG, "coo_fill: NULL pointer");
    if (!aligned(row_ptr, 8) || !aligned(row, 8) || !aligned(col, 8) || !aligned(x, esize(dtype)) || !aligned(values, esize(dtype)))
        return fail(MBNB_SPARSE_ERR_ARG, "coo_fill: every tensor must be aligned to its element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_coo_fill<T>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, static_cast<const T *>(x), R, C, threshold, row_ptr, row, col,
                           static_cast<T *>(values), nnz);
        return launched("coo_fill", KN_COO_FILL);
    });
}

// --------------------------------------------------------------------------- int8 COO values
int64_t mbnb_coo_quantize_workspace_bytes(void) { return COO_QP * 4; }

int mbnb_coo_quantize(const void *values, int dtype, int64_t nnz, int8_t *q, float *scale, void *workspace, int64_t workspace_bytes, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "coo_quantize: unknown dtype %d", dtype);
    if (nnz < 0) return fail(MBNB_SPARSE_ERR_ARG, "coo_quantize: negative size");
    if (nnz == 0) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_quantize: nnz = 0: the maximum of no values is undefined");
    if (nnz > kMaxElems) return fail(MBNB_SPARSE_ERR_SHAPE, "coo_quantize: problem too large");
    if (!values || !q || !scale) return fail(MBNB_SPARSE_ERR_ARG, "coo_quantize: NULL pointer");
    if (!aligned(values, esize(dtype)) || !aligned(scale, 4)) return fail(MBNB_SPARSE_ERR_ARG, "coo_quantize: values and scale must be aligned to their element size");
    if (!workspace || !aligned(workspace, 256) || workspace_bytes < COO_QP * 4)
        return fail(MBNB_SPARSE_ERR_ARG, "coo_quantize: needs a 256-byte aligned workspace of %d bytes", COO_QP * 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t want = (nnz + 2047) / 2048;     // 8 values per thread and pass
    const int nparts = (int)(want < COO_QP ? want : COO_QP);
    uint32_t *part = static_cast<uint32_t *>(workspace);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_coo_absmax<T>, dim3((unsigned)nparts), dim3(256), 0, st, static_cast<const T *>(values), nnz, part);
        hipLaunchKernelGGL(k_coo_quantize<T>, dim3((unsigned)nparts), dim3(256), 0, st, static_cast<const T *>(values), nnz, part, nparts, q, scale);
        set_variant("parts%d", nparts);
        return launched("coo_quantize", KN_COO_QUANT);
    });
}

// --------------------------------------------------------------------------- spmm
int64_t mbnb_spmm_coo_workspace_bytes(int64_t nnz, int64_t rows) {
    if (nnz < 0 || rows < 0 || nnz > kMaxIndex || rows > kMaxIndex) return 0;
    return spmm_ws(nnz, rows).total();
}

int mbnb_spmm_coo(const void *row, int row_bits, const void *col, int col_bits, const void *values, int value_kind, const float *scale, int64_t nnz,
                  const void *dense, int dtype, int64_t rows, int64_t cols, int64_t N, void *out, void *workspace, int64_t workspace_bytes, int flags,
                  void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: unknown dtype %d", dtype);
    if (flags & ~MBNB_SPARSE_FORCE_GENERIC) return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: unknown flags 0x%x", flags);
    if ((row_bits != 32 && row_bits != 64) || (col_bits != 32 && col_bits != 64)) return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: indices must be int32 or int64");
    if (value_kind < MBNB_COO_VALUES || value_kind > MBNB_COO_INT8_ENTRY) return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: unknown value kind %d", value_kind);
    if (nnz < 0 || rows < 0 || cols < 0 || N < 0) return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: negative size");
    if (nnz > kMaxIndex || rows > kMaxIndex) return fail(MBNB_SPARSE_ERR_SHAPE, "spmm_coo: nnz and rows must be below 2^31 - 1");
    if (N > 0 && (rows > kMaxElems / N || cols > kMaxElems / N)) return fail(MBNB_SPARSE_ERR_SHAPE, "spmm_coo: problem too large");
    const bool vec_shape = (N * esize(dtype)) % 16 == 0;
    const bool general = flags & MBNB_SPARSE_FORCE_GENERIC;
    if (rows == 0 || N == 0) {
        g_kernel = kSparseKernelNames[vec_shape ? (general ? KN_SPMM8_GEN : KN_SPMM8) : (general ? KN_SPMM1_GEN : KN_SPMM1)];
        return MBNB_SPARSE_OK;
    }
    if (!out || (nnz > 0 && (!row || !col || !values || (cols > 0 && !dense) || (value_kind != MBNB_COO_VALUES && !scale))))
        return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: NULL pointer");
    const int vsize = value_kind == MBNB_COO_VALUES ? esize(dtype) : 1;
    if (!aligned(out, esize(dtype)) || !aligned(dense, esize(dtype)) || !aligned(values, vsize) || !aligned(row, row_bits / 8) || !aligned(col, col_bits / 8) ||
        !aligned(scale, 4))
        return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: every tensor must be aligned to its element size");
    const SpmmWs L = spmm_ws(nnz, rows);
    if (!workspace || !aligned(workspace, 256) || workspace_bytes < L.total())
        return fail(MBNB_SPARSE_ERR_ARG, "spmm_coo: needs a 256-byte aligned workspace of %lld bytes", (long long)L.total());
    const bool vec = vec_shape && aligned(dense, 16) && aligned(out, 16);
    const int cpl = vec ? 16 / esize(dtype) : 4;
    int G = 64;
    while (G > 16 && (int64_t)(G / 2) * cpl >= N) G /= 2;      // the smallest group of 16 / 32 / 64 lanes that spans N (a whole wave for wide outputs)
    const int64_t ntile = (N + (int64_t)G * cpl - 1) / ((int64_t)G * cpl), rows_per_wg = 4 * (64 / G);
    const int64_t b_spmm = ntile * ((rows + rows_per_wg - 1) / rows_per_wg);
    if (b_spmm > kMaxGrid) return fail(MBNB_SPARSE_ERR_UNSUPPORTED, "spmm_coo: %lld workgroups exceed one launch", (long long)b_spmm);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *wsb = static_cast<char *>(workspace);
    int *flag = reinterpret_cast<int *>(wsb);
    int *row_ptr = reinterpret_cast<int *>(wsb + L.flag_bytes);
    int *cursor = reinterpret_cast<int *>(wsb + L.flag_bytes + L.ptr_bytes);
    int *perm = reinterpret_cast<int *>(wsb + L.zeroed());
    const hipError_t me = hipMemsetAsync(workspace, 0, (size_t)L.zeroed(), st);
    if (me != hipSuccess) return fail((int)me, "spmm_coo: hipMemsetAsync failed: %s", hipGetErrorString(me));
    const unsigned b_nnz = (unsigned)((nnz + 255) / 256);
    hipLaunchKernelGGL(k_coo_flag, dim3(b_nnz ? b_nnz : 1), dim3(256), 0, st, row, row_bits, nnz, flag, general ? 1 : 0);
    hipLaunchKernelGGL(k_coo_search, dim3((unsigned)((rows + 1 + 255) / 256)), dim3(256), 0, st, row, row_bits, nnz, rows, flag, row_ptr);
    if (nnz > 0) {
        hipLaunchKernelGGL(k_coo_hist, dim3(b_nnz), dim3(256), 0, st, row, row_bits, nnz, rows, flag, row_ptr);
        hipLaunchKernelGGL(k_scan_counts<int>, dim3(1), dim3(1024), 0, st, row_ptr, rows, (const int *)flag);
        hipLaunchKernelGGL(k_coo_scatter, dim3(b_nnz), dim3(256), 0, st, row, row_bits, nnz, rows, flag, row_ptr, cursor, perm);
        hipLaunchKernelGGL(k_coo_sort, dim3((unsigned)rows), dim3(256), 0, st, flag, row_ptr, perm);
    }
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        const T *d = static_cast<const T *>(dense);
        T *o = static_cast<T *>(out);
        if (vec) hipLaunchKernelGGL((k_spmm_csr<T, true>), dim3((unsigned)b_spmm), dim3(256), 0, st, flag, row_ptr, perm, col, col_bits, values, value_kind, scale, d, rows, cols, N, o, G, ntile);
        else hipLaunchKernelGGL((k_spmm_csr<T, false>), dim3((unsigned)b_spmm), dim3(256), 0, st, flag, row_ptr, perm, col, col_bits, values, value_kind, scale, d, rows, cols, N, o, G, ntile);
        set_variant("G%d x%lld", G, (long long)ntile);
        return launched("spmm_coo", vec ? (general ? KN_SPMM8_GEN : KN_SPMM8) : (general ? KN_SPMM1_GEN : KN_SPMM1));
    });
}

}  // extern "C"
