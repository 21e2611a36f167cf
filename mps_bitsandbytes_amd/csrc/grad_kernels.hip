// grad_kernels.hip — input gradient of the quantised linears (mbnb_linear_grad_input, include/mbnb_hip.h):
//   dX[M, K] = dY[M, N] · dequant(W)[N, K]
// The weight is stored [N, K] and every GEMM of the library contracts over its K, so the dense path first writes the transposed
// weight Wt [K, N] in the weight dtype (k_dequant_t), then runs the forward's dense GEMM with A = dY, weight = Wt, ldw = N and the
// library's own plan (gemm_dense.hip).  k_grad_generic decodes W on the fly and serves everything the dense path does not.
#include "common.h"
#include "dispatch.h"

namespace mbnb {

// =====================================================================================
// Transposed dequantise pass.  A lane decodes an 8 x 8 block -- 8 consecutive rows n of W, 8 consecutive columns k -- into 32 pair words
// (row r, columns 2p, 2p + 1), transposes it in registers (each output word takes the same half of the pair words of rows 2q and 2q + 1)
// and writes 8 rows k of Wt, 8 values n each: one 16-byte store per row.  Lanes 0-7 of a wave hold n-blocks 0-7 of the same k-block,
// so a store instruction writes eight whole 128-byte lines (64 n of each of 8 rows k); a load instruction reads 8 rows x 8 lanes of
// consecutive words.  No value crosses a lane, so the transpose needs no LDS exchange (the 4-bit code table is the only LDS).
// A wave covers 64 n x 64 k, a workgroup four waves along k (64 n x 256 k).  Stores are write-through ("sc1") where the dense GEMM reads
// Wt next, as the forward's in-step dequantise pass does.
//   FMT: MBNB_NF4 / MBNB_FP4 (one packed dword per row, blocksize >= 8: one absmax per row), MBNB_W_INT8_ROWWISE / MBNB_W_FP8_E4M3
//   (8 bytes per row), MBNB_W_DENSE (16 bytes per row: the 16-bit weight itself, moved as bits).
// vec: N % 8 == 0 and Wt 16-byte aligned (16-byte stores); otherwise 2-byte stores of the n < N values.
// =====================================================================================
template <typename T, int FMT, bool NESTED>
__global__ __launch_bounds__(256) void k_dequant_t(const uint8_t *__restrict__ W, AbsmaxView am, const float *__restrict__ scales, int64_t N,
                                                  int64_t K, int64_t ldq, int bs_shift, T *__restrict__ out, int vec, int write_through) {
    __shared__ float lut[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 64 + (lane & 7) * 8;
    const int64_t k0 = ((int64_t)blockIdx.y * 4 + wave) * 64 + (lane >> 3) * 8;
    const bool active = k0 < K;
    uint32_t P[8][4];
    // loads first: the code table's barrier sits under the HBM round trip
    if constexpr (FMT == MBNB_NF4 || FMT == MBNB_FP4) {
        uint32_t w[8];
        float a[8];
        const int64_t nblk = (ldq * 2) >> bs_shift;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int64_t n = n0 + r;
            const bool ok = active && n < N;
            w[r] = ok ? *reinterpret_cast<const uint32_t *>(W + n * ldq + k0 / 2) : 0u;
            a[r] = ok ? load_absmax<NESTED>(am, n * nblk + (k0 >> bs_shift)) : 0.0f;
        }
        fill_code_lut<FMT>(lut, threadIdx.x);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int p = 0; p < 4; p++) P[r][p] = pack2<T>(lut[(w[r] >> (8 * p)) & 15] * a[r], lut[(w[r] >> (8 * p + 4)) & 15] * a[r]);
    } else if constexpr (FMT == MBNB_W_INT8_ROWWISE || FMT == MBNB_W_FP8_E4M3) {
        constexpr int WF = FMT == MBNB_W_FP8_E4M3 ? W8_FP8 : W8_INT8;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int64_t n = n0 + r;
            const bool ok = active && n < N;
            const u32x2 q = ok ? *reinterpret_cast<const u32x2 *>(W + n * ldq + k0) : u32x2{0u, 0u};
            const float sc = ok ? scales[n] : 0.0f;
            const float s = WF == W8_FP8 ? sc : sc / 127.0f;  // functional.py:635
#pragma unroll
            for (int p = 0; p < 4; p++)
                P[r][p] = pack2<T>(w8_decode_sel<WF>(q[p >> 1], (2 * p) & 3) * s, w8_decode_sel<WF>(q[p >> 1], (2 * p + 1) & 3) * s);
        }
    } else {   // MBNB_W_DENSE
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int64_t n = n0 + r;
            const u32x4 q = (active && n < N) ? *reinterpret_cast<const u32x4 *>(W + n * ldq + k0 * 2) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int p = 0; p < 4; p++) P[r][p] = q[p];
        }
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t k = k0 + j;
        if (k >= K) break;
        const int p = j >> 1;
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; q++)
            o[q] = (j & 1) ? ((P[2 * q][p] >> 16) | (P[2 * q + 1][p] & 0xFFFF0000u)) : ((P[2 * q][p] & 0xFFFFu) | (P[2 * q + 1][p] << 16));
        T *dst = out + k * N + n0;
        if (vec) {
            if (n0 >= N) continue;
            if (write_through) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(o) : "memory");
            else *reinterpret_cast<u32x4 *>(dst) = o;
        } else {
            uint16_t *d16 = reinterpret_cast<uint16_t *>(dst);
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (n0 + e < N) d16[e] = (uint16_t)(o[e >> 1] >> (16 * (e & 1)));
        }
    }
}

// =====================================================================================
// Generic kernel: a thread owns one column k and GM = 4 rows m of dX; it walks n, decodes W[n, k] once (rounded to the weight dtype T,
// as dequantize_* writes it) and adds it times dY[m, n] into four f32 accumulators.  Any format, dtype, blocksize, shape and alignment.
// =====================================================================================
constexpr int GRAD_GM = 4;

template <typename T, int FMT, bool NESTED>
__device__ __forceinline__ float grad_decode(const uint8_t *__restrict__ W, const AbsmaxView &am, const float *__restrict__ scales,
                                             const float *lut, int64_t n, int64_t k, int64_t ldq, int bs_shift) {
    float v;
    if constexpr (FMT == MBNB_NF4 || FMT == MBNB_FP4) {
        const int64_t K_weight = ldq * 2;
        const int64_t flat = n * K_weight + k;
        const uint8_t b = W[flat >> 1];
        const int idx = (flat & 1) ? (b >> 4) : (b & 15);
        v = lut[idx] * load_absmax<NESTED>(am, n * (K_weight >> bs_shift) + (k >> bs_shift));
    } else if constexpr (FMT == MBNB_W_INT8_ROWWISE) {
        v = (float)(int)(int8_t)W[n * ldq + k] * (scales[n] / 127.0f);
    } else if constexpr (FMT == MBNB_W_FP8_E4M3) {
        v = fp8_e4m3_to_float(W[n * ldq + k]) * scales[n];
    } else {
        return to_f32(reinterpret_cast<const T *>(W + n * ldq)[k]);
    }
    return to_f32(from_f32<T>(v));
}

template <typename T, typename O, int FMT, bool NESTED>
__global__ __launch_bounds__(256) void k_grad_generic(const T *__restrict__ dY, int64_t M, int64_t N, const uint8_t *__restrict__ W, AbsmaxView am,
                                                     const float *__restrict__ scales, int64_t K, int64_t ldq, int bs_shift, O *__restrict__ dX) {
    __shared__ float lut[16];
    if constexpr (FMT == MBNB_NF4 || FMT == MBNB_FP4) {
        fill_code_lut<FMT>(lut, threadIdx.x);
        __syncthreads();
    }
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;   // no barrier below: the code table's is above
    // grid.y holds at most 65535 row groups: a workgroup walks on by the grid's height, as the forward's generic kernels do
    for (int64_t m0 = (int64_t)blockIdx.y * GRAD_GM; m0 < M; m0 += (int64_t)gridDim.y * GRAD_GM) {
        const T *y[GRAD_GM];
#pragma unroll
        for (int i = 0; i < GRAD_GM; i++) y[i] = dY + (m0 + i < M ? m0 + i : M - 1) * N;
        float acc[GRAD_GM] = {};
        for (int64_t n = 0; n < N; n++) {
            const float w = grad_decode<T, FMT, NESTED>(W, am, scales, lut, n, k, ldq, bs_shift);
#pragma unroll
            for (int i = 0; i < GRAD_GM; i++) acc[i] = fmaf(to_f32(y[i][n]), w, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < GRAD_GM; i++)
            if (m0 + i < M) dX[(m0 + i) * K + k] = (O)to_f32(from_f32<T>(acc[i]));   // one rounding to the weight dtype, then the cast
    }
}

// ------------------------------------------------------------------------------------- host side
static bool is4(int fmt) { return fmt == MBNB_NF4 || fmt == MBNB_FP4; }

// the words of the variant record (mbnb_last_kernel's second string): which instantiation a launch took
template <typename T> constexpr bool kIsBf16 = false;
template <> constexpr bool kIsBf16<bf16_t> = true;

// the pass serves this weight (the caller checks W's alignment)
static bool grad_t_shape(int64_t N, int64_t K, int fmt, int blocksize) {
    if (N <= 0 || K <= 0 || (int64_t)((K + 255) / 256) > 65535 || (N + 63) / 64 > 0x7FFFFFFF) return false;
    return is4(fmt) ? blocksize >= 8 : (K % 8 == 0);
}

// the dense path serves this problem: 16-bit weights, the dense GEMM's reduction constraints on N, the pass
bool grad_dense_shape(int64_t M, int64_t N, int64_t K, int fmt, int w_dtype) {
    if (w_dtype != MBNB_F16 && w_dtype != MBNB_BF16) return false;
    if (M <= 0 || N < 128 || N % 64 != 0 || 256 * N * 2 >= ((int64_t)1 << 31)) return false;
    return is4(fmt) || K % 8 == 0;
}

int64_t grad_input_workspace_bytes(int64_t M, int64_t N, int64_t K, int fmt, int w_dtype) {
    if (!grad_dense_shape(M, N, K, fmt, w_dtype)) return 0;
    const int64_t s = gemm_dense_slices(M, K, N);
    return gemm_dense_wd_bytes(K, N) + (s > 1 ? s * M * K * 4 : 0);
}

template <typename T, int FMT>
static int launch_dequant_t(const uint8_t *W, const AbsmaxView &am, const float *scales, int64_t N, int64_t K, int64_t ldq, int blocksize, T *out,
                            int write_through, hipStream_t st) {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((K + 255) / 256));
    const int vec = (N % 8 == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int sh = is4(FMT) ? __builtin_ctz((unsigned)blocksize) : 0;
    const bool nested = is4(FMT) && am.i8;
    if (nested) hipLaunchKernelGGL((k_dequant_t<T, FMT, true>), grid, dim3(256), 0, st, W, am, scales, N, K, ldq, sh, out, vec, write_through);
    else hipLaunchKernelGGL((k_dequant_t<T, FMT, false>), grid, dim3(256), 0, st, W, am, scales, N, K, ldq, sh, out, vec, write_through);
    // (on the dense path the GEMM's own variant replaces this one)
    set_kernel_variant("grad_t %s %s %s %s", FMT == MBNB_NF4 ? "nf4" : FMT == MBNB_FP4 ? "fp4" : FMT == MBNB_W_INT8_ROWWISE ? "int8" : FMT == MBNB_W_FP8_E4M3 ? "fp8" : "dense",
                       kIsBf16<T> ? "bf16" : "f16", nested ? "nested" : "plain", vec ? "vec" : "scalar");
    return check_launch("linear_grad_input(transpose)");
}

template <typename T>
static int dequant_t_dispatch(int fmt, const uint8_t *W, const AbsmaxView &am, const float *scales, int64_t N, int64_t K, int64_t ldq, int blocksize,
                              T *out, int write_through, hipStream_t st) {
    switch (fmt) {
        case MBNB_NF4: return launch_dequant_t<T, MBNB_NF4>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);
        case MBNB_FP4: return launch_dequant_t<T, MBNB_FP4>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);
        case MBNB_W_INT8_ROWWISE: return launch_dequant_t<T, MBNB_W_INT8_ROWWISE>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);
        case MBNB_W_FP8_E4M3: return launch_dequant_t<T, MBNB_W_FP8_E4M3>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);
        default: return launch_dequant_t<T, MBNB_W_DENSE>(W, am, scales, N, K, ldq, blocksize, out, write_through, st);
    }
}

template <typename T, typename O, int FMT>
static void launch_generic_fmt(const T *dY, int64_t M, int64_t N, const uint8_t *W, const AbsmaxView &am, const float *scales, int64_t K, int64_t ldq,
                               int sh, O *dX, hipStream_t st) {
    const int64_t groups = (M + GRAD_GM - 1) / GRAD_GM;
    const dim3 grid((unsigned)((K + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));   // the kernel walks the row groups past grid.y
    const bool nested = is4(FMT) && am.i8;
    if (nested) hipLaunchKernelGGL((k_grad_generic<T, O, FMT, true>), grid, dim3(256), 0, st, dY, M, N, W, am, scales, K, ldq, sh, dX);
    else hipLaunchKernelGGL((k_grad_generic<T, O, FMT, false>), grid, dim3(256), 0, st, dY, M, N, W, am, scales, K, ldq, sh, dX);
    set_kernel_variant("grad_generic %s %s>%s %s", FMT == MBNB_NF4 ? "nf4" : FMT == MBNB_FP4 ? "fp4" : FMT == MBNB_W_INT8_ROWWISE ? "int8" : FMT == MBNB_W_FP8_E4M3 ? "fp8" : "dense",
                       sizeof(T) == 4 ? "f32" : kIsBf16<T> ? "bf16" : "f16", sizeof(O) == 4 ? "f32" : kIsBf16<O> ? "bf16" : "f16", nested ? "nested" : "plain");
}

template <typename T, typename O>
static int launch_generic(int fmt, const T *dY, int64_t M, int64_t N, const uint8_t *W, const AbsmaxView &am, const float *scales, int64_t K,
                          int64_t ldq, int blocksize, O *dX, hipStream_t st) {
    if ((K + 255) / 256 > 0x7FFFFFFF) {
        set_error("linear_grad_input: the generic kernel takes at most %lld columns", (long long)0x7FFFFFFF * 256);
        return MBNB_ERR_UNSUPPORTED;
    }
    const int sh = is4(fmt) ? __builtin_ctz((unsigned)blocksize) : 0;
    switch (fmt) {
        case MBNB_NF4: launch_generic_fmt<T, O, MBNB_NF4>(dY, M, N, W, am, scales, K, ldq, sh, dX, st); break;
        case MBNB_FP4: launch_generic_fmt<T, O, MBNB_FP4>(dY, M, N, W, am, scales, K, ldq, sh, dX, st); break;
        case MBNB_W_INT8_ROWWISE: launch_generic_fmt<T, O, MBNB_W_INT8_ROWWISE>(dY, M, N, W, am, scales, K, ldq, sh, dX, st); break;
        case MBNB_W_FP8_E4M3: launch_generic_fmt<T, O, MBNB_W_FP8_E4M3>(dY, M, N, W, am, scales, K, ldq, sh, dX, st); break;
        default: launch_generic_fmt<T, O, MBNB_W_DENSE>(dY, M, N, W, am, scales, K, ldq, sh, dX, st); break;
    }
    set_kernel_name("grad_generic");
    return check_launch("linear_grad_input(generic)");
}

template <typename T>
static int generic_out(int fmt, const void *dY, int64_t M, int64_t N, const uint8_t *W, const AbsmaxView &am, const float *scales, int64_t K,
                       int64_t ldq, int blocksize, int out_dtype, void *dX, hipStream_t st) {
    const T *y = static_cast<const T *>(dY);
    switch (out_dtype) {
        case MBNB_F16: return launch_generic<T, f16_t>(fmt, y, M, N, W, am, scales, K, ldq, blocksize, static_cast<f16_t *>(dX), st);
        case MBNB_BF16: return launch_generic<T, bf16_t>(fmt, y, M, N, W, am, scales, K, ldq, blocksize, static_cast<bf16_t *>(dX), st);
        default: return launch_generic<T, float>(fmt, y, M, N, W, am, scales, K, ldq, blocksize, static_cast<float *>(dX), st);
    }
}

// ldq: bytes per row of W.  The arguments were validated by mbnb_linear_grad_input (api.hip).
int linear_grad_input_dispatch(const void *dY, int64_t M, int64_t N, int fmt, const void *Wv, const AbsmaxView &am, const float *scales, int64_t K,
                               int64_t ldq, int blocksize, int w_dtype, int out_dtype, void *dX, void *ws, int64_t ws_bytes, bool transpose_only,
                               hipStream_t st) {
    const uint8_t *W = static_cast<const uint8_t *>(Wv);
    const uintptr_t wa = reinterpret_cast<uintptr_t>(W);
    const bool w_aligned = fmt == MBNB_W_DENSE ? (wa & 15) == 0 : is4(fmt) ? (wa & 3) == 0 : (wa & 7) == 0;
    if (transpose_only) {
        if ((w_dtype != MBNB_F16 && w_dtype != MBNB_BF16) || !grad_t_shape(N, K, fmt, blocksize) || !w_aligned) {
            set_error("linear_grad_input: the transposed pass alone needs a 16-bit weight dtype, blocksize >= 8 (4-bit) or K %% 8 == 0, and an aligned W");
            return MBNB_ERR_UNSUPPORTED;
        }
        const int rc = w_dtype == MBNB_F16 ? dequant_t_dispatch<f16_t>(fmt, W, am, scales, N, K, ldq, blocksize, static_cast<f16_t *>(dX), 0, st)
                                           : dequant_t_dispatch<bf16_t>(fmt, W, am, scales, N, K, ldq, blocksize, static_cast<bf16_t *>(dX), 0, st);
        set_kernel_name("grad_t");
        return rc;
    }
    const int64_t wt_bytes = gemm_dense_wd_bytes(K, N);
    const bool dense = grad_dense_shape(M, N, K, fmt, w_dtype) && (!is4(fmt) || blocksize >= 32) && w_aligned && ws != nullptr &&
                       (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= wt_bytes && (reinterpret_cast<uintptr_t>(dY) & 15) == 0 &&
                       grad_t_shape(N, K, fmt, blocksize);
    if (dense) {
        int64_t slices = gemm_dense_slices(M, K, N);
        if (slices > 1 && ws_bytes < wt_bytes + slices * M * K * 4) slices = 1;   // a short workspace costs the split, never the result
        char *wsb = static_cast<char *>(ws);
        int rc = w_dtype == MBNB_F16 ? dequant_t_dispatch<f16_t>(fmt, W, am, scales, N, K, ldq, blocksize, reinterpret_cast<f16_t *>(wsb), 1, st)
                                     : dequant_t_dispatch<bf16_t>(fmt, W, am, scales, N, K, ldq, blocksize, reinterpret_cast<bf16_t *>(wsb), 1, st);
        if (rc) return rc;
        rc = gemm_dense_direct(dY, wsb, w_dtype, nullptr, out_dtype, dX, M, K, N, N, reinterpret_cast<float *>(wsb + wt_bytes), slices, 0, 0, st);
        set_kernel_name(slices > 1 ? "grad_t+dense_splitk" : "grad_t+dense");
        return rc;
    }
    switch (w_dtype) {
        case MBNB_F16: return generic_out<f16_t>(fmt, dY, M, N, W, am, scales, K, ldq, blocksize, out_dtype, dX, st);
        case MBNB_BF16: return generic_out<bf16_t>(fmt, dY, M, N, W, am, scales, K, ldq, blocksize, out_dtype, dX, st);
        default: return generic_out<float>(fmt, dY, M, N, W, am, scales, K, ldq, blocksize, out_dtype, dX, st);
    }
}

}  // namespace mbnb
