// train_kernels.hip — the trainable-weight linears of libmbnb_train.so (include/mbnb_train.h):
//   SwitchBackLinear's int8 forward   out = round_T(round_T(X . Wd^T) + b),  Wd = round_T(q * round_T(s / 127))
//   the weight gradient               dW = dY^T . X   (a contraction over the token dimension M)
// The MFMA work is libmbnb_hip's public mbnb_gemm_dense with the library's own plan (slices = 0); this file holds the passes that
// feed it and the generic kernels for what it does not take.  Its own last-error and kernel-name records (mbnb_train_last_*).
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/mbnb_train.h"
#include "common.h"
#include "host.h"

// host.h's predicates and with_dtype() take this library's dtype codes
static_assert(MBNB_TRAIN_F16 == mbnb::kF16 && MBNB_TRAIN_BF16 == mbnb::kBF16 && MBNB_TRAIN_F32 == mbnb::kF32, "dtype codes");

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

// ---------------------------------------------------------------- the SwitchBack weight rule (reference SwitchBackFunction.forward)
// `weight_int8.to(T) * (weight_scales[:, None] / 127.0).to(T)`: the quotient in f32, rounded to T, times the code, rounded to T again.
// The product of an int8 code and a 16-bit value is exact in f32, so the second rounding is the only one.  For T = f32 this is
// dequantize_rowwise's q * (s / 127).
template <typename T> __device__ __forceinline__ float sb_scale(float s) { return to_f32(from_f32<T>(s / 127.0f)); }
template <typename T> __device__ __forceinline__ float sb_decode(int q, float s_t) { return to_f32(from_f32<T>((float)q * s_t)); }

// =====================================================================================
// Wd pass, vector form: a thread takes 8 values of UN consecutive rows -- one 8-byte load and ONE 16-byte store each, so a wave's store
// instruction writes 1 KiB contiguous -- the shape of dequantize_rowwise's in-step pass (quant_kernels.hip k_dequantize_rows8_wt).  Stores
// are write-through ("sc1") where the dense GEMM reads Wd next.  16-bit T, K % 8 == 0, W 8-byte and Wd 16-byte aligned.
// =====================================================================================
template <typename T, int UN>
__global__ __launch_bounds__(256) void k_switchback_dq8(const uint8_t *__restrict__ q, const float *__restrict__ scales, int64_t rows, int64_t cols,
                                                       T *__restrict__ out, int write_through) {
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (c0 >= cols) return;
    u32x2 w[UN];
    float s[UN];
#pragma unroll
    for (int u = 0; u < UN; u++) {
        const int64_t r = (int64_t)blockIdx.y * UN + u;
        const bool ok = r < rows;
        w[u] = ok ? *reinterpret_cast<const u32x2 *>(q + r * cols + c0) : u32x2{0u, 0u};
        s[u] = sb_scale<T>(ok ? scales[r] : 0.0f);
    }
#pragma unroll
    for (int u = 0; u < UN; u++) {
        const int64_t r = (int64_t)blockIdx.y * UN + u;
        if (r >= rows) continue;
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t word = w[u][e >> 1];
            const int sh = 16 * (e & 1);
            // pack2 rounds each exact product once (and keeps the multiply out of a mixed-precision fma)
            o[e] = pack2<T>((float)(int)(int8_t)(word >> sh) * s[u], (float)(int)(int8_t)(word >> (sh + 8)) * s[u]);
        }
        T *dst = out + r * cols + c0;
        if (write_through) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(o) : "memory");
        else *reinterpret_cast<u32x4 *>(dst) = o;
    }
}

// Wd pass, scalar form: any K, alignment and dtype (f32 included).  One element per thread.
template <typename T>
__global__ __launch_bounds__(256) void k_switchback_dq1(const int8_t *__restrict__ q, const float *__restrict__ scales, int64_t rows, int64_t cols,
                                                       T *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    out[i] = from_f32<T>(sb_decode<T>(q[i], sb_scale<T>(scales[i / cols])));
}

// The bias of the dense route, in place: out = round_T(out + b) -- torch's `output + bias` on the rounded product.  VEC: 8 elements per
// thread with 16-byte loads and stores (N % 8 == 0, out and bias 16-byte aligned, 16-bit T); else one element per thread.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_bias_add(T *__restrict__ out, const T *__restrict__ bias, int64_t M, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        if (i >= M * N / 8) return;
        const int64_t e0 = i * 8, n = e0 % N;
        u32x4 o = *reinterpret_cast<const u32x4 *>(out + e0);
        const u32x4 b = *reinterpret_cast<const u32x4 *>(bias + n);
#pragma unroll
        for (int p = 0; p < 4; p++)
            o[p] = pack2<T>(mbnb::unpack_lo<T>(o[p]) + mbnb::unpack_lo<T>(b[p]), mbnb::unpack_hi<T>(o[p]) + mbnb::unpack_hi<T>(b[p]));
        *reinterpret_cast<u32x4 *>(out + e0) = o;
    } else {
        if (i >= M * N) return;
        out[i] = from_f32<T>(to_f32(out[i]) + to_f32(bias[i % N]));
    }
}

// =====================================================================================
// Generic SwitchBack kernel: a wave owns one output column n and SB_GM rows m; its lanes stride over k (coalesced reads of X rows and of
// W's row n), decode W[n, k] with the rule above, accumulate in f32, reduce across the wave, and round twice: the product, then + bias.
// Any shape, dtype, alignment and M.  Workgroups are numbered flat: 4 columns x SB_GM rows each.
// =====================================================================================
constexpr int SB_GM = 8;

template <typename T>
__global__ __launch_bounds__(256) void k_switchback_generic(const T *__restrict__ X, int64_t M, int64_t K, const int8_t *__restrict__ W,
                                                           const float *__restrict__ scales, int64_t N, const T *__restrict__ bias,
                                                           T *__restrict__ out, int64_t n_groups) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)(blockIdx.x % n_groups) * 4 + wave;
    const int64_t m0 = (int64_t)(blockIdx.x / n_groups) * SB_GM;
    if (n >= N) return;
    const float s = sb_scale<T>(scales[n]);
    const int8_t *wr = W + n * K;
    const T *x[SB_GM];
#pragma unroll
    for (int i = 0; i < SB_GM; i++) x[i] = X + (m0 + i < M ? m0 + i : M - 1) * K;
    float acc[SB_GM] = {};
    for (int64_t k = lane; k < K; k += 64) {
        const float w = sb_decode<T>(wr[k], s);
#pragma unroll
        for (int i = 0; i < SB_GM; i++) acc[i] = fmaf(to_f32(x[i][k]), w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < SB_GM; i++) acc[i] = mbnb::wave_sum(acc[i]);
    if (lane < SB_GM && m0 + lane < M) {
        float v = acc[0];
#pragma unroll
        for (int i = 1; i < SB_GM; i++)
            if (lane == i) v = acc[i];
        T y = from_f32<T>(v);
        if (bias) y = from_f32<T>(to_f32(y) + to_f32(bias[n]));
        out[(m0 + lane) * N + n] = y;
    }
}

// =====================================================================================
// Transposing, zero-padding copy of a 16-bit [M, C] matrix into [C, Mp] (Mp % 64 == 0): the pattern of grad_kernels.hip's k_dequant_t in
// its MBNB_W_DENSE form.  A lane loads an 8 x 8 block -- 8 rows m, 8 columns c -- as 32 pair words, transposes it in registers and writes
// 8 rows c of the output, 8 values m each: one 16-byte store per row.  Lanes 0-7 of a wave hold m-blocks 0-7 of the same c-block, so a store
// instruction writes eight whole 128-byte lines; no value crosses a lane.  Rows m >= M load as zeros, so columns M .. Mp-1 of the output are
// written as zeros (the grid covers all Mp / 64 m-blocks).  A wave covers 64 m x 64 c, a workgroup four waves along c.
// VEC_IN: C % 8 == 0 and A 16-byte aligned (16-byte loads); otherwise 2-byte loads of the c < C values.  Write-through stores where the
// dense GEMM reads the copy next.
// =====================================================================================
template <bool VEC_IN>
__global__ __launch_bounds__(256) void k_transpose_pad(const uint16_t *__restrict__ A, int64_t M, int64_t C, int64_t Mp, uint16_t *__restrict__ out,
                                                      int write_through) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * 64 + (lane & 7) * 8;
    const int64_t c0 = ((int64_t)blockIdx.y * 4 + wave) * 64 + (lane >> 3) * 8;
    if (c0 >= C) return;
    uint32_t P[8][4];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t m = m0 + r;
        const bool ok = m < M;
        if constexpr (VEC_IN) {
            const u32x4 q = ok ? *reinterpret_cast<const u32x4 *>(A + m * C + c0) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int p = 0; p < 4; p++) P[r][p] = q[p];
        } else {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int64_t c = c0 + 2 * p;
                const uint32_t lo = (ok && c < C) ? A[m * C + c] : 0u;
                const uint32_t hi = (ok && c + 1 < C) ? A[m * C + c + 1] : 0u;
                P[r][p] = lo | (hi << 16);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t c = c0 + j;
        if (c >= C) break;
        const int p = j >> 1;
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; q++)
            o[q] = (j & 1) ? ((P[2 * q][p] >> 16) | (P[2 * q + 1][p] & 0xFFFF0000u)) : ((P[2 * q][p] & 0xFFFFu) | (P[2 * q + 1][p] << 16));
        uint16_t *dst = out + c * Mp + m0;
        if (write_through) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(o) : "memory");
        else *reinterpret_cast<u32x4 *>(dst) = o;
    }
}

// =====================================================================================
// Generic weight-gradient kernel: a thread owns one column k and GW_GN rows n of dW; it walks m, reads X[m, k] (coalesced over the wave)
// and dY[m, n0 .. n0 + 3] (one address per wave), and accumulates in f32; one rounding to T.  Any dtype, shape and alignment; M = 0 writes
// zeros.  Workgroups are numbered flat: 256 columns x GW_GN rows each.
// =====================================================================================
constexpr int GW_GN = 4;

template <typename T>
__global__ __launch_bounds__(256) void k_grad_w_generic(const T *__restrict__ dY, const T *__restrict__ X, int64_t M, int64_t N, int64_t K,
                                                       T *__restrict__ dW, int64_t k_groups) {
    const int64_t k = (int64_t)(blockIdx.x % k_groups) * 256 + threadIdx.x;
    const int64_t n0 = (int64_t)(blockIdx.x / k_groups) * GW_GN;
    if (k >= K) return;
    int64_t nn[GW_GN];
#pragma unroll
    for (int i = 0; i < GW_GN; i++) nn[i] = n0 + i < N ? n0 + i : N - 1;
    float acc[GW_GN] = {};
    for (int64_t m = 0; m < M; m++) {
        const float x = to_f32(X[m * K + k]);
        const T *y = dY + m * N;
#pragma unroll
        for (int i = 0; i < GW_GN; i++) acc[i] = fmaf(to_f32(y[nn[i]]), x, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < GW_GN; i++)
        if (n0 + i < N) dW[(n0 + i) * K + k] = from_f32<T>(acc[i]);
}

// ------------------------------------------------------------------------------------- host side
// Every name mbnb_train_last_kernel() can report (tests/switchback_cases.py has a GPU case for each).
enum { KN_SB_DQ, KN_SB_DENSE, KN_SB_GENERIC, KN_GW_T, KN_GW_DENSE, KN_GW_GENERIC };
const char *const kTrainKernelNames[] = {"switchback_dq", "switchback_dq+dense", "switchback_generic", "grad_w_t", "grad_w_t+dense", "grad_w_generic"};

thread_local const char *g_kernel = "";

// The variant of the last call: which kernel forms ran behind the name, as words joined by blanks ("dq8x4 bias8", "dy1 x8"; tests/
// switchback_cases.py restates the conditions).  mbnb_train_last_kernel() hands out name and variant in one buffer (name, NUL, variant, NUL).
// The variant of a "+dense" route's GEMM stays in libmbnb_hip's own record.
thread_local char g_variant[64] = "";
thread_local char g_kernel_out[128] = "";

void set_variant(const char *word) { snprintf(g_variant, sizeof(g_variant), "%s", word); }
void add_variant(const char *word) {
    const size_t n = strlen(g_variant);
    snprintf(g_variant + n, sizeof(g_variant) - n, n ? " %s" : "%s", word);
}
// every launching entry point begins with this: a call whose launcher sets no variant reports "", never the previous call's
void begin_call() { g_variant[0] = '\0'; }

// a failed launch leaves the record as every failing call leaves it: the last successful call's name, no variant
int launched(const char *what, int name) {
    if (int rc = mbnb::launch_status(what)) {
        g_variant[0] = '\0';
        return rc;
    }
    g_kernel = kTrainKernelNames[name];
    return MBNB_TRAIN_OK;
}

int from_gemm(int rc, const char *what) {
    if (rc != 0) {
        g_variant[0] = '\0';
        return fail(rc, "%s: mbnb_gemm_dense failed: %s", what, mbnb_last_error());
    }
    return MBNB_TRAIN_OK;
}

// Route thresholds, measured with MBNB_TRAIN_FORCE_GENERIC against the default: the generic kernels win only on
// small products.  The forward takes the dense route from 2^27 multiply-adds, and below M = 16 only on weights of 2^25 elements or more
// (bf16 4096 x 4096: M = 8 24.8 us generic against 28.7; 11008 x 4096: M = 4 60.6 against 41.1).  The weight gradient takes it above
// 2^26 (2 M weights: M = 17 9.3 us generic against 16 for the two passes + GEMM; M = 64 25.5 against 16.1).  mbnb_gemm_dense serves any
// M (rows past M read as zeros).
constexpr int64_t kSbDenseMacs = (int64_t)1 << 27, kSbBigWeight = (int64_t)1 << 25, kGwDenseMacs = (int64_t)1 << 26;

// ---- SwitchBack forward
bool sb_dense_shape(int64_t M, int64_t N, int64_t K, int dtype) {
    return is16(dtype) && M > 0 && N > 0 && K % 64 == 0 && K >= 128 && 256 * K * 2 < ((int64_t)1 << 31) && M * N * 4 < ((int64_t)1 << 40) &&
           M * N * K >= kSbDenseMacs && (M >= 16 || N * K >= kSbBigWeight);
}
int64_t sb_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!sb_dense_shape(M, N, K, dtype)) return 0;
    return round256(N * K * 2) + mbnb_gemm_dense_workspace_bytes(M, N, K);
}

template <typename T>
int sb_pass(const int8_t *W, const float *scales, int64_t N, int64_t K, T *out, int write_through, hipStream_t st) {
    const uint8_t *q = reinterpret_cast<const uint8_t *>(W);
    if constexpr (sizeof(T) == 2) {
        if (K % 8 == 0 && aligned(W, 8) && aligned(out, 16)) {
            const unsigned gx = (unsigned)((K / 8 + 255) / 256);
            if (N * K <= ((int64_t)1 << 25) && (N + 3) / 4 <= 65535) {
                hipLaunchKernelGGL((k_switchback_dq8<T, 4>), dim3(gx, (unsigned)((N + 3) / 4)), dim3(256), 0, st, q, scales, N, K, out, write_through);
                set_variant("dq8x4");
                return 0;
            }
            if (N <= 65535) {
                hipLaunchKernelGGL((k_switchback_dq8<T, 1>), dim3(gx, (unsigned)N), dim3(256), 0, st, q, scales, N, K, out, write_through);
                set_variant("dq8x1");
                return 0;
            }
        }
    }
    hipLaunchKernelGGL(k_switchback_dq1<T>, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, W, scales, N, K, out);   // N K <= kMaxElems
    set_variant("dq1");
    return 0;
}

template <typename T>
int sb_forward(const T *X, int64_t M, int64_t K, const int8_t *W, const float *scales, int64_t N, const T *bias, T *out, void *ws,
               int64_t ws_bytes, int flags, hipStream_t st) {
    if (flags & MBNB_TRAIN_PASS_ONLY) {
        sb_pass<T>(W, scales, N, K, out, 0, st);
        return launched("switchback_forward(pass)", KN_SB_DQ);
    }
    if (M == 0) {
        g_kernel = kTrainKernelNames[KN_SB_GENERIC];
        return MBNB_TRAIN_OK;
    }
    const int64_t wd_bytes = round256(N * K * 2);
    const bool dense = !(flags & MBNB_TRAIN_FORCE_GENERIC) && sb_dense_shape(M, N, K, sizeof(T) == 2 ? MBNB_TRAIN_F16 : MBNB_TRAIN_F32) &&
                       ws != nullptr && aligned(ws, 256) && ws_bytes >= wd_bytes && aligned(X, 16) && aligned(W, 8) && aligned(out, 16);
    if constexpr (sizeof(T) == 2) if (dense) {
        T *wd = static_cast<T *>(ws);
        sb_pass<T>(W, scales, N, K, wd, 1, st);
        if (int rc = launched("switchback_forward(pass)", KN_SB_DQ)) return rc;
        const int dt = std::is_same<T, f16_t>::value ? MBNB_F16 : MBNB_BF16;
        char *part = static_cast<char *>(ws) + wd_bytes;
        if (int rc = from_gemm(mbnb_gemm_dense(X, wd, dt, nullptr, dt, out, M, N, K, K, part, ws_bytes - wd_bytes, 0, st), "switchback_forward"))
            return rc;
        if (!bias) {
            add_variant("nobias");
        } else if (N % 8 == 0 && aligned(bias, 16)) {
            hipLaunchKernelGGL((k_bias_add<T, true>), dim3((unsigned)((M * N / 8 + 255) / 256)), dim3(256), 0, st, out, bias, M, N);
            add_variant("bias8");
        } else {
            hipLaunchKernelGGL((k_bias_add<T, false>), dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, st, out, bias, M, N);
            add_variant("bias1");
        }
        return launched("switchback_forward(bias)", KN_SB_DENSE);
    }
    const int64_t n_groups = (N + 3) / 4, blocks = n_groups * ((M + SB_GM - 1) / SB_GM);
    if (blocks > 0x7FFFFFFF) return fail(MBNB_TRAIN_ERR_UNSUPPORTED, "switchback_forward: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL(k_switchback_generic<T>, dim3((unsigned)blocks), dim3(256), 0, st, X, M, K, W, scales, N, bias, out, n_groups);
    return launched("switchback_forward(generic)", KN_SB_GENERIC);
}

// ---- weight gradient
int64_t padded_rows(int64_t M) {
    const int64_t p = (M + 63) / 64 * 64;
    return p < 128 ? 128 : p;
}
bool gw_dense_shape(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!is16(dtype) || N <= 0 || K <= 0 || M < 0) return false;
    const int64_t Mp = padded_rows(M);
    return 256 * Mp * 2 < ((int64_t)1 << 31) && (K + 255) / 256 <= 65535 && (N + 255) / 256 <= 65535 && N * K * 4 < ((int64_t)1 << 40) &&
           M * N * K > kGwDenseMacs;
}
int64_t gw_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!gw_dense_shape(M, N, K, dtype)) return 0;
    const int64_t Mp = padded_rows(M);
    return round256(N * Mp * 2) + round256(K * Mp * 2) + mbnb_gemm_dense_workspace_bytes(N, K, Mp);
}

// A [M, C] -> out [C, Mp]; C / 256 <= 65535 (checked by the callers).  True where the 16-byte loads ran.
bool transpose_pad(const void *A, int64_t M, int64_t C, int64_t Mp, void *out, int write_through, hipStream_t st) {
    const dim3 grid((unsigned)(Mp / 64), (unsigned)((C + 255) / 256));
    const uint16_t *a = static_cast<const uint16_t *>(A);
    uint16_t *o = static_cast<uint16_t *>(out);
    const bool vec = C % 8 == 0 && aligned(A, 16);
    if (vec) hipLaunchKernelGGL(k_transpose_pad<true>, grid, dim3(256), 0, st, a, M, C, Mp, o, write_through);
    else hipLaunchKernelGGL(k_transpose_pad<false>, grid, dim3(256), 0, st, a, M, C, Mp, o, write_through);
    return vec;
}

template <typename T>
int gw_generic(const T *dY, const T *X, int64_t M, int64_t N, int64_t K, T *dW, hipStream_t st) {
    const int64_t k_groups = (K + 255) / 256, blocks = k_groups * ((N + GW_GN - 1) / GW_GN);
    if (blocks > 0x7FFFFFFF) return fail(MBNB_TRAIN_ERR_UNSUPPORTED, "linear_grad_weight: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL(k_grad_w_generic<T>, dim3((unsigned)blocks), dim3(256), 0, st, dY, X, M, N, K, dW, k_groups);
    return launched("linear_grad_weight(generic)", KN_GW_GENERIC);
}

int gw_dispatch(const void *dY, const void *X, int64_t M, int64_t N, int64_t K, int dtype, void *dW, void *ws, int64_t ws_bytes, int flags,
                hipStream_t st) {
    const int64_t Mp = padded_rows(M);
    if (flags & MBNB_TRAIN_PASS_ONLY) {
        if (!is16(dtype) || 256 * Mp * 2 >= ((int64_t)1 << 31) || (K + 255) / 256 > 65535 || !aligned(dW, 16))
            return fail(MBNB_TRAIN_ERR_UNSUPPORTED, "linear_grad_weight: the transposing pass alone needs a 16-bit dtype, a 16-byte aligned "
                                                    "output and sizes within one launch");
        if (transpose_pad(X, M, K, Mp, dW, 0, st)) set_variant("x8");
        else set_variant("x1");
        return launched("linear_grad_weight(pass)", KN_GW_T);
    }
    const int64_t yt_bytes = round256(N * Mp * 2), xt_bytes = round256(K * Mp * 2);
    const bool dense = !(flags & MBNB_TRAIN_FORCE_GENERIC) && gw_dense_shape(M, N, K, dtype) && ws != nullptr && aligned(ws, 256) &&
                       ws_bytes >= yt_bytes + xt_bytes && aligned(dW, 16);
    if (dense) {
        char *wsb = static_cast<char *>(ws);
        if (transpose_pad(dY, M, N, Mp, wsb, 1, st)) set_variant("dy8");
        else set_variant("dy1");
        if (transpose_pad(X, M, K, Mp, wsb + yt_bytes, 1, st)) add_variant("x8");
        else add_variant("x1");
        if (int rc = launched("linear_grad_weight(transpose)", KN_GW_T)) return rc;
        if (int rc = from_gemm(mbnb_gemm_dense(wsb, wsb + yt_bytes, dtype, nullptr, dtype, dW, N, K, Mp, Mp, wsb + yt_bytes + xt_bytes,
                                               ws_bytes - yt_bytes - xt_bytes, 0, st),
                               "linear_grad_weight"))
            return rc;
        g_kernel = kTrainKernelNames[KN_GW_DENSE];
        return MBNB_TRAIN_OK;
    }
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return gw_generic<T>(static_cast<const T *>(dY), static_cast<const T *>(X), M, N, K, static_cast<T *>(dW), st);
    });
}

bool dtype_ok(int dtype) { return dtype >= MBNB_TRAIN_F16 && dtype <= MBNB_TRAIN_F32; }

}  // namespace

extern "C" {

int mbnb_train_abi_version(void) { return MBNB_TRAIN_ABI_VERSION; }
const char *mbnb_train_last_error(void) { return mbnb::last_error(); }
const char *mbnb_train_last_kernel(void) {
    const size_t n = strlen(g_kernel) + 1;
    memcpy(g_kernel_out, g_kernel, n);
    memcpy(g_kernel_out + n, g_variant, strlen(g_variant) + 1);
    return g_kernel_out;
}
int64_t mbnb_train_padded_rows(int64_t M) { return M < 0 ? 0 : padded_rows(M); }

int64_t mbnb_switchback_forward_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!dtype_ok(dtype) || M <= 0 || N <= 0 || K <= 0 || M > kMaxElems / K || N > kMaxElems / K || M > kMaxElems / N) return 0;
    return sb_workspace_bytes(M, N, K, dtype);
}

int mbnb_switchback_forward(const void *X, int dtype, int64_t M, int64_t K, const int8_t *W, const float *scales, int64_t N, const void *bias,
                            void *out, void *workspace, int64_t workspace_bytes, int flags, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: unknown dtype %d", dtype);
    if (flags & ~(MBNB_TRAIN_PASS_ONLY | MBNB_TRAIN_FORCE_GENERIC)) return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: unknown flags 0x%x", flags);
    const bool pass = flags & MBNB_TRAIN_PASS_ONLY;
    if ((!pass && M < 0) || N < 0 || K < 0) return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: negative size");
    if ((K > 0 && (N > kMaxElems / K || (!pass && M > kMaxElems / K))) || (!pass && N > 0 && M > kMaxElems / N))
        return fail(MBNB_TRAIN_ERR_SHAPE, "switchback_forward: problem too large");
    if (workspace_bytes < 0) return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: negative workspace size");
    if (N == 0 || (!pass && M == 0)) {
        g_kernel = kTrainKernelNames[pass ? KN_SB_DQ : KN_SB_GENERIC];
        return MBNB_TRAIN_OK;
    }
    if (K == 0 && !pass) return fail(MBNB_TRAIN_ERR_SHAPE, "switchback_forward: K = 0 with outputs to write");
    if (!W || !scales || !out || (!pass && !X)) return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: NULL pointer");
    if (K == 0) {
        g_kernel = kTrainKernelNames[KN_SB_DQ];
        return MBNB_TRAIN_OK;
    }
    if (!aligned(out, esize(dtype)) || (!pass && (!aligned(X, esize(dtype)) || (bias && !aligned(bias, esize(dtype))))))
        return fail(MBNB_TRAIN_ERR_ARG, "switchback_forward: X, bias and out must be aligned to their element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return sb_forward<T>(static_cast<const T *>(X), M, K, W, scales, N, static_cast<const T *>(bias), static_cast<T *>(out), workspace, workspace_bytes,
                             flags, st);
    });
}

int64_t mbnb_linear_grad_weight_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    if (!dtype_ok(dtype) || M < 0 || N <= 0 || K <= 0 || M > kMaxElems / (N > K ? N : K) || N > kMaxElems / K) return 0;
    return gw_workspace_bytes(M, N, K, dtype);
}

int mbnb_linear_grad_weight(const void *dY, const void *X, int64_t M, int64_t N, int64_t K, int dtype, void *dW, void *workspace,
                            int64_t workspace_bytes, int flags, void *stream) {
    begin_call();
    if (!dtype_ok(dtype)) return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: unknown dtype %d", dtype);
    if (flags & ~(MBNB_TRAIN_PASS_ONLY | MBNB_TRAIN_FORCE_GENERIC)) return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: unknown flags 0x%x", flags);
    const bool pass = flags & MBNB_TRAIN_PASS_ONLY;
    if (M < 0 || (!pass && N < 0) || K < 0) return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: negative size");
    const int64_t big = pass ? K : (N > K ? N : K);
    if ((big > 0 && (M > kMaxElems / big || padded_rows(M) > kMaxElems / big)) || (!pass && K > 0 && N > kMaxElems / K))
        return fail(MBNB_TRAIN_ERR_SHAPE, "linear_grad_weight: problem too large");
    if (workspace_bytes < 0) return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: negative workspace size");
    if (K == 0 || (!pass && N == 0)) {
        g_kernel = kTrainKernelNames[pass ? KN_GW_T : KN_GW_GENERIC];
        return MBNB_TRAIN_OK;
    }
    if (!dW || (M > 0 && (!X || (!pass && !dY)))) return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: NULL pointer");
    if (!aligned(dW, esize(dtype)) || (M > 0 && (!aligned(X, esize(dtype)) || (!pass && !aligned(dY, esize(dtype))))))
        return fail(MBNB_TRAIN_ERR_ARG, "linear_grad_weight: dY, X and dW must be aligned to their element size");
    return gw_dispatch(dY, X, M, N, K, dtype, dW, workspace, workspace_bytes, flags, static_cast<hipStream_t>(stream));
}

}  // extern "C"
