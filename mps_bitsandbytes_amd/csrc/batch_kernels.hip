// batch_kernels.hip — the grouped 4-bit decode launches for 2 to 16 activation rows and the C ABI of libmbnb_batch.so
// (include/mbnb_batch.h).
//
// libmbnb_group.so and libmbnb_lora.so fuse the layers that share an activation ROW.  A serving loop hands every projection 2 to 16
// rows per step, and there mbnb_matmul_4bit streams each weight through k_skinny4 (matmul4_kernels.hip), one launch per layer, and
// an un-merged adapter costs four torch launches more.  Here:
//   k_skinny4_group         k_skinny4's workgroup (MT = 1, NR = 1: 16 weight rows x all M activation rows, 16 waves over the
//                           128-k blocks) behind the member table of gemv4_group.h: ONE launch for up to 16 layers;
//   k_lora_down_rows        t_g[m, j] = A_g[j, :] . x[m, :] in f32, one workgroup per adapter row of every member (k_lora_down's
//                           chunking and summation chain, the row of A held in registers over the M activation rows);
//   k_skinny4_group (LORA)  the same workgroup with a rank-R epilogue: element (m, n) adds scaling_g B_g[n, :] . t_g[m, :] to its
//                           f32 sum before the bias add and the double rounding.
// Every sum runs in a fixed order (wave order through LDS, DPP wave sums, quarter order; no atomics).
#include "../../include/mbnb_batch.h"
#include "host.h"
#include "gemv4_group.h"

#include <math.h>

static_assert(MBNB_BATCH_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_BATCH_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "the argument checks are shared");
static_assert(MBNB_BATCH_NOT_APPLICABLE == MBNB_GROUP_NOT_APPLICABLE && MBNB_BATCH_NOT_APPLICABLE == MBNB_LORA_NOT_APPLICABLE, "one NOT_APPLICABLE");
static_assert(MBNB_LORA_MAX_R == mbnb::kLoraMaxR, "the epilogue's slices");
static_assert(MBNB_BATCH_MAX_M == 16, "one 16 x 16 MFMA tile holds every activation row");
static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");

namespace {

using mbnb::AbsmaxView;
using mbnb::aligned;
using mbnb::bf16_t;
using mbnb::bfe_u32;
using mbnb::Dot2;
using mbnb::dpp_wave_sum;
using mbnb::f16_t;
using mbnb::f32x4;
using mbnb::fail;
using mbnb::fill_code_lut;
using mbnb::from_f32;
using mbnb::load_absmax;
using mbnb::LoraRow;
using mbnb::Mfma16;
using mbnb::pack2;
using mbnb::to_f32;
using mbnb::u32x4;

constexpr int kMax = mbnb::kGroupMax;
constexpr int kWaves = 16;                      // waves of a k_skinny4 workgroup
constexpr int kRedBytes = kWaves * 1024;        // [16 waves][256] f32 partial tiles
constexpr int kPartBytes = 4 * 1024;            // LORA: [4 quarters][256] f32 partial up-sums

// k_skinny4_group's arguments: member i owns the workgroups [first_block[i], first_block[i+1]); entries past n hold the total
struct BatchArgs {
    const void *x;      // [M, K] row-major in the call's dtype
    int64_t K;
    int32_t M;
    int32_t bs_shift;   // log2(blocksize)
    int32_t first_block[kMax + 1];
    int32_t n;
    mbnb_group_member m[kMax];
};

// the LORA kernel's: the adapters by member (t is [M, R] here) and the row pitch, in floats, of the two LDS slices: odd and >= every R
template <bool LORA> struct SkinnyArgs {
    BatchArgs g;
};
template <> struct SkinnyArgs<true> {
    BatchArgs g;
    LoraRow rows[kMax];
    int32_t pitch;
};

// k_lora_down_rows' arguments: member i owns the workgroups (= adapter rows) [first_row[i], first_row[i+1])
struct DownArgs {
    const void *x;
    int64_t K;
    int32_t M;
    int32_t n;
    int32_t first_row[kMax + 1];
    struct {
        const void *a;
        float *t;
        int64_t R;
    } m[kMax];
};
static_assert(sizeof(SkinnyArgs<true>) + sizeof(DownArgs) <= 4096, "both tables must fit the kernel-argument segment");
static_assert(sizeof(SkinnyArgs<false>) <= 4096, "the member table must fit the kernel-argument segment");

// One workgroup = 16 waves x 16 weight rows of ONE member x all M <= 16 activation rows.
//
// From the member's pointers on THIS IS A COPY of the body of k_skinny4<T, T, QT, NESTED, MT = 1, NR = 1> (matmul4_kernels.hip), kept
// in step BY HAND as group_row (gemv4_group.h) is with k_gemv4_lean, for the reason given there: that kernel's schedule must not
// move.  K_weight == K here (the library's condition).  tests/test_gpu_batch.py holds the two equal bit for bit.
//
// LORA: with R > 0 wave w requests, before the k-loop, row n0 + w of B (dead rows clamped) and row w of t -- lane l takes
// j = 64 c + l for c < ceil(R / 64) through range-checked descriptors, so j >= R and rows m >= M read zeros -- and parks them in LDS
// beside the partial tiles.  After the wave-order reduction the element (m, n) of thread e = tid & 255 is shared by the four threads
// e + 256 qr: quarter qr adds f32(B[n, j]) * t[m, j] (a rounded product, then the add) for j = qr, qr + 4, ... in rising j, and thread
// e forms u = ((p0 + p1) + p2) + p3, then (s + scaling * u) + bias.  R == 0 (workgroup-uniform) takes none of this.
template <typename T, int QT, bool NESTED, bool LORA>
__global__ __launch_bounds__(1024) void k_skinny4_group(const SkinnyArgs<LORA> args) {
    constexpr int WV = kWaves;
    __shared__ float lut[16];
    extern __shared__ __attribute__((aligned(16))) char red_raw[];   // [WV][256] f32; LORA: + [4][256] f32 + t [16][pitch] + B [16][pitch]
    float *red = reinterpret_cast<float *>(red_raw);
    const BatchArgs &a = args.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    // the member that owns this workgroup: the compare chain of k_gemv4_group (kernel arguments and blockIdx only: scalar)
    const int blk = (int)blockIdx.x;
    int g = 0, first = 0;
#pragma unroll
    for (int i = 1; i < kMax; i++) {
        const int fb = a.first_block[i];     // nondecreasing; the total from member n on
        g = fb <= blk ? i : g;
        first = fb <= blk ? fb : first;
    }
    g = __builtin_amdgcn_readfirstlane(g);
    const mbnb_group_member &mem = a.m[g];
    const T *__restrict__ X = static_cast<const T *>(a.x);
    const uint8_t *__restrict__ packed = static_cast<const uint8_t *>(mem.packed);
    const AbsmaxView am{mem.absmax_f32, mem.absmax_i8, mem.absmax2, mem.blocksize2};
    const T *__restrict__ bias = static_cast<const T *>(mem.bias);
    T *__restrict__ out = static_cast<T *>(mem.out);
    const int64_t M = a.M, N = mem.N, K = a.K;
    const int bs_shift = a.bs_shift;

    // ---- k_skinny4<T, T, QT, NESTED, 1, 1> from here (n0 counts from the member's row 0)
    const int64_t n0 = (int64_t)(blk - first) * 16;
    const int64_t nblk = K >> bs_shift, row_bytes = K >> 1;
    fill_code_lut<QT>(lut, threadIdx.x);

    int64_t nw = n0 + r16;
    nw = nw < N ? nw : N - 1;
    const uint8_t *wrow = packed + nw * row_bytes;
    const int64_t arow = nw * nblk;
    int64_t mx = r16;
    mx = mx < M ? mx : M - 1;
    const T *xrow = X + mx * K;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t nb128 = K >> 7;
    // packed weights + absmax of block b + WV are requested before block b is decoded (HBM latency); the activation
    // fragments (L2-resident) are requested at the top of each trip
    u32x4 w, w_n;
    float am_c, am_n;
    auto request_w = [&](int64_t b) {
        const int64_t k_lane = (b << 7) + 32 * q;
        w_n = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wrow + (k_lane >> 1)));
        am_n = load_absmax<NESTED>(am, arow + (k_lane >> bs_shift));
    };
    if (wave < nb128) request_w(wave);

    // LORA: this wave's slices of row n0 + wave of B (16-bit loads in a range of 2 R bytes) and of row `wave` of t (32-bit loads in a
    // range of 4 R bytes, 0 bytes for a row the batch does not have)
    constexpr int kSlices = mbnb::kLoraMaxR / 64;
    int R = 0;
    uint16_t lb[kSlices] = {};
    float lt[kSlices] = {};
    if constexpr (LORA) {
        const LoraRow &lr = args.rows[g];
        R = lr.R;
        if (R > 0) {
            const int wv = __builtin_amdgcn_readfirstlane(wave);
            int64_t nb = n0 + wv;
            nb = nb < N ? nb : N - 1;
            const char *brow = static_cast<const char *>(lr.b) + nb * (int64_t)R * 2;
            const float *trow = lr.t + (wv < M ? (int64_t)wv * R : 0);
            const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(brow), 0, R * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(trow), 0, wv < M ? R * 4 : 0, 0x00020000);
#pragma unroll
            for (int c = 0; c < kSlices; c++) {
                if (64 * c < R) {          // workgroup-uniform
                    lb[c] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs_b, lane * 2, c * 128, 0);
                    lt[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, lane * 4, c * 256, 0));
                }
            }
        }
    }

    // raw barrier for the code table (__syncthreads() would drain the requests just issued)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    for (int64_t b = wave; b < nb128; b += WV) {
        const int64_t k_lane = (b << 7) + 32 * q;
        typename Mfma16<T>::frag xf[4];
#pragma unroll
        for (int gq = 0; gq < 4; gq++) xf[gq] = *reinterpret_cast<const typename Mfma16<T>::frag *>(xrow + k_lane + 8 * gq);
        __builtin_amdgcn_sched_barrier(0);
        w = w_n;
        am_c = am_n;
        if (b + WV < nb128) request_w(b + WV);
        __builtin_amdgcn_sched_barrier(0);   // every request of the block is in flight before the first use
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            // the reference's dequantize arithmetic: code * absmax in f32 -> RNE 16 bit (functional.py:388-416)
            const uint32_t wd = w[gq];
            const uint32_t wo = wd & 0xF0F0F0F0u;
            const uint32_t we = (wd << 2) & 0x3C3C3C3Cu;
            const char *lutb = reinterpret_cast<const char *>(lut);
            u32x4 fr;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float lo = *reinterpret_cast<const float *>(lutb + bfe_u32(we, 8 * j, 8)) * am_c;
                const float hi = *reinterpret_cast<const float *>(lutb + bfe_u32(wo, 8 * j + 2, 6)) * am_c;
                fr[j] = pack2<T>(lo, hi);
            }
            const auto af = __builtin_bit_cast(typename Mfma16<T>::frag, fr);
            acc = Mfma16<T>::run(af, xf[gq], acc);
        }
    }
    // ---- reduce the WV partial 16 x 16 tiles in wave order
    *reinterpret_cast<f32x4 *>(red + (wave * 256 + lane * 4)) = acc;
    float *part = red + kRedBytes / 4;
    float *ts = part + kPartBytes / 4;
    int pitch = 0;
    if constexpr (LORA) {
        pitch = args.pitch;
        if (R > 0) {
            float *bs = ts + 16 * pitch;
#pragma unroll
            for (int c = 0; c < kSlices; c++) {
                const int j = 64 * c + lane;
                if (j < R) {
                    ts[wave * pitch + j] = lt[c];
                    bs[wave * pitch + j] = to_f32(__builtin_bit_cast(T, lb[c]));
                }
            }
        }
    }
    __syncthreads();
    const int e = threadIdx.x & 255;
    const int ln = e >> 2, r = e & 3;
    const int nl = 4 * (ln >> 4) + r;        // D[a][b]: a = 4 * (lane >> 4) + r (weight row), b = lane & 15
    const int64_t n = n0 + nl;
    const int64_t m = ln & 15;
    float s = 0.0f;
    if (threadIdx.x < 256) {
#pragma unroll
        for (int wv = 0; wv < WV; wv++) s += red[wv * 256 + e];
    }
    if constexpr (LORA) {
        if (R > 0) {      // workgroup-uniform: every thread meets the barrier
            const float *bs = ts + 16 * pitch;
            const float *bn = bs + nl * pitch, *tm = ts + (int)m * pitch;
            float p = 0.0f;
            for (int j = (int)(threadIdx.x >> 8); j < R; j += 4) p += bn[j] * tm[j];      // a rounded product, then the add (-ffp-contract=off)
            part[threadIdx.x] = p;
            __syncthreads();
            if (threadIdx.x < 256) {
                const float up = ((part[e] + part[256 + e]) + part[512 + e]) + part[768 + e];
                s += args.rows[g].scaling * up;
            }
        }
    }
    if (threadIdx.x < 256 && n < N && m < M) {
        const float v = s + (bias ? to_f32(bias[n]) : 0.0f);
        out[m * N + n] = from_f32<T>(to_f32(from_f32<T>(v)));
    }
}

// t_g[m, j] = A_g[j, :] . x[m, :] for every m < M.  One workgroup of 256 threads per adapter row; the K chunking is k_lora_down's:
// thread tid takes the 16 bytes at k = 2048 u + 8 tid of the row and of each x row, for u < KU, through descriptors of K * 2 bytes (a
// partial last chunk reads zeros).  The row of A stays in registers; the x rows come from L2.  Per m the chain is k_lora_down's:
// Dot2 over the thread's chunks, the DPP wave sum, the four wave sums added in wave order by one lane.
template <typename T, int KU>
__global__ __launch_bounds__(256) void k_lora_down_rows(const DownArgs a) {
    __shared__ float part[MBNB_BATCH_MAX_M][4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = (int)blockIdx.x;
    int g = 0, first = 0;      // the compare chain of k_gemv4_group: scalar
#pragma unroll
    for (int i = 1; i < kMax; i++) {
        const int fr = a.first_row[i];
        g = fr <= blk ? i : g;
        first = fr <= blk ? fr : first;
    }
    g = __builtin_amdgcn_readfirstlane(g);
    const int64_t K = a.K;
    const int M = a.M;
    const int j = blk - first;
    const char *row = static_cast<const char *>(a.m[g].a) + (int64_t)j * K * 2;
    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(row), 0, (int)(K * 2), 0x00020000);
    u32x4 aq[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) aq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, tid * 16, u * 4096, 2));    // aux 2: nt
    for (int m = 0; m < M; m++) {
        const char *xr = static_cast<const char *>(a.x) + (int64_t)m * K * 2;
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xr), 0, (int)(K * 2), 0x00020000);
        u32x4 xq[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) xq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, tid * 16, u * 4096, 0));
        float acc = 0.0f;
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc = Dot2<T>::run(aq[u][c], xq[u][c], acc);
        const float s = dpp_wave_sum(acc);
        if (lane == 63) part[m][wave] = s;
    }
    __syncthreads();
    if (tid < M) a.m[g].t[(int64_t)tid * a.m[g].R + j] = ((part[tid][0] + part[tid][1]) + part[tid][2]) + part[tid][3];
}

// ---------------------------------------------------------------- host side
constexpr int kLaunchBytes = 128;
char *last_launch() {
    static thread_local char text[kLaunchBytes] = "";
    return text;
}

template <typename T, int QT, bool NESTED>
int launch(const BatchArgs &g, hipStream_t stream) {
    SkinnyArgs<false> a;
    a.g = g;
    hipLaunchKernelGGL((k_skinny4_group<T, QT, NESTED, false>), dim3((unsigned)g.first_block[g.n]), dim3(1024), kRedBytes, stream, a);
    const int rc = mbnb::launch_status("mbnb_batch_gemm4");
    if (rc == 0) snprintf(last_launch(), kLaunchBytes, "skinny_group G%d M%d", g.n, g.M);
    return rc;
}

template <typename T, int QT, bool NESTED>
int launch_lora(const DownArgs &d, const SkinnyArgs<true> &a, hipStream_t stream) {
    const int ku = (int)((a.g.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 down((unsigned)d.first_row[d.n]), grid((unsigned)a.g.first_block[a.g.n]);
    const size_t lds = (size_t)kRedBytes + kPartBytes + (size_t)2 * 16 * a.pitch * 4;      // <= 53376 bytes at pitch 257
#define MBNB_BATCH_DOWN(KU_)                                                                    \
    case KU_:                                                                                   \
        hipLaunchKernelGGL((k_lora_down_rows<T, KU_>), down, dim3(256), 0, stream, d);          \
        break
    switch (KU) {
        MBNB_BATCH_DOWN(1);
        MBNB_BATCH_DOWN(2);
        MBNB_BATCH_DOWN(3);
        MBNB_BATCH_DOWN(4);
        MBNB_BATCH_DOWN(6);
        MBNB_BATCH_DOWN(8);
    }
#undef MBNB_BATCH_DOWN
    hipLaunchKernelGGL((k_skinny4_group<T, QT, NESTED, true>), grid, dim3(1024), lds, stream, a);
    const int rc = mbnb::launch_status("mbnb_batch_gemm4_lora");
    if (rc == 0)
        snprintf(last_launch(), kLaunchBytes, "lora_down_rows G%d R%d M%d ku%d/KU%d + skinny_group_lora G%d M%d", d.n, d.first_row[d.n], d.M, ku, KU,
                 a.g.n, a.g.M);
    return rc;
}

// 0, or the negative code of an argument error: mbnb_group_gemv4's checks of a member table (gemv4_group.h), and M
int argument_errors(const char *who, const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members,
                    int n, int flags) {
    if (const int rc = mbnb::group_argument_errors(who, x, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (M <= 0) return fail(MBNB_BATCH_ERR_SHAPE, "%s: M = %lld", who, (long long)M);
    return 0;
}

// The conditions of the fused launch: this is the one place they live.  0 with `a` filled and `nested` set, or
// MBNB_BATCH_NOT_APPLICABLE after recording the reason; nothing is dereferenced.
//
// They are a subset of the shapes for which launch_matmul4 (matmul4_kernels.hip) takes "skinny MT1 NR1": its fast_layout (16-bit,
// blocksize >= 32, K_weight % 32 == 0, K % 8 == 0, A and packed 16-byte aligned), then skinny (2 <= M, K % 128 == 0, M <= 16 for
// MT = 1).  gemm_small_shape needs M > 16 and the GEMV branch needs !skinny, so neither takes such a call first: a call that is
// fused here is a call whose members mbnb_matmul_4bit would have sent to that same instantiation.
int conditions(const char *who, const void *x, int64_t M, int64_t K, int dtype, int blocksize, const mbnb_group_member *members, int n, BatchArgs &a,
               bool &nested) {
    const int na = MBNB_BATCH_NOT_APPLICABLE;
    if (M < MBNB_BATCH_MIN_M || M > MBNB_BATCH_MAX_M)
        return fail(na, "%s: %d <= M <= %d is needed, got M = %lld", who, MBNB_BATCH_MIN_M, MBNB_BATCH_MAX_M, (long long)M);
    if (!mbnb::is16(dtype)) return fail(na, "%s: a 16-bit dtype is needed, got dtype %d", who, dtype);
    if (blocksize < 32 || (blocksize & (blocksize - 1)) != 0) return fail(na, "%s: a blocksize that is a power of two >= 32 is needed, got %d", who, blocksize);
    if (K % 128 != 0 || K % blocksize != 0 || K < 128 || K > 16384)
        return fail(na, "%s: K %% 128 == 0, K %% blocksize == 0 and 128 <= K <= 16384 are needed, got K = %lld with blocksize %d", who, (long long)K,
                    blocksize);
    if (!aligned(x, 16)) return fail(na, "%s: x is not 16-byte aligned", who);
    nested = members[0].absmax_i8 != nullptr;
    a.x = x;
    a.K = K;
    a.M = (int32_t)M;
    a.bs_shift = __builtin_ctz((unsigned)blocksize);
    a.n = n;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const mbnb_group_member &m = members[i];
        if (!aligned(m.packed, 16)) return fail(na, "%s: member %d's packed weight is not 16-byte aligned", who, i);
        if (m.N >= ((int64_t)1 << 40) || m.N * (K / 2) >= ((int64_t)1 << 40)) return fail(na, "%s: member %d's packed weight has 2^40 bytes or more", who, i);
        if ((m.absmax_i8 != nullptr) != nested)
            return fail(na, "%s: plain and double-quantised absmax in one group (member %d differs from member 0)", who, i);
        if (nested && m.blocksize2 <= 0) return fail(na, "%s: member %d's blocksize2 is %d", who, i, m.blocksize2);
        a.first_block[i] = (int32_t)blocks;
        blocks += (m.N + 15) / 16;
        if (blocks >= ((int64_t)1 << 31)) return fail(na, "%s: 2^31 workgroups or more", who);
        a.m[i] = m;
        a.m[i].pad_ = 0;
    }
    for (int i = n; i <= kMax; ++i) a.first_block[i] = (int32_t)blocks;
    for (int i = n; i < kMax; ++i) a.m[i] = mbnb_group_member{};
    return 0;
}

#define MBNB_BATCH_FORMS(FN, ...)                                                                                                   \
    (dtype == MBNB_GROUP_F16                                                                                                        \
         ? (quant_type == MBNB_GROUP_NF4 ? (nested ? FN<f16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<f16_t, MBNB_NF4, false>(__VA_ARGS__))    \
                                         : (nested ? FN<f16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<f16_t, MBNB_FP4, false>(__VA_ARGS__)))   \
         : (quant_type == MBNB_GROUP_NF4 ? (nested ? FN<bf16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<bf16_t, MBNB_NF4, false>(__VA_ARGS__))  \
                                         : (nested ? FN<bf16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<bf16_t, MBNB_FP4, false>(__VA_ARGS__))))

}  // namespace

extern "C" {

int mbnb_batch_abi_version(void) { return MBNB_BATCH_ABI_VERSION; }

const char *mbnb_batch_last_error(void) { return mbnb::last_error(); }

const char *mbnb_batch_last_launch(void) { return last_launch(); }

int mbnb_batch_gemm4(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members, int n, int flags,
                     void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_batch_gemm4";
    if (const int rc = argument_errors(who, x, M, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    BatchArgs a;
    bool nested;
    if (const int rc = conditions(who, x, M, K, dtype, blocksize, members, n, a, nested)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return MBNB_BATCH_FORMS(launch, a, s);
}

int mbnb_batch_gemm4_lora(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members,
                          const mbnb_lora_adapter *adapters, int n, int flags, void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_batch_gemm4_lora";
    // ---- argument errors: mbnb_batch_gemm4's, then the adapter table's
    if (const int rc = argument_errors(who, x, M, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (!adapters) return fail(MBNB_BATCH_ERR_ARG, "%s: NULL adapter table", who);
    for (int i = 0; i < n; ++i) {
        const mbnb_lora_adapter &ad = adapters[i];
        if (ad.R < 0) return fail(MBNB_BATCH_ERR_SHAPE, "%s: member %d has R = %d", who, i, ad.R);
        if (ad.R > 0 && (!ad.a || !ad.b)) return fail(MBNB_BATCH_ERR_ARG, "%s: member %d has R = %d with a NULL a or b", who, i, ad.R);
    }
    // ---- the conditions of the fused launches: mbnb_batch_gemm4's, then the adapters'
    SkinnyArgs<true> a;
    bool nested;
    if (const int rc = conditions(who, x, M, K, dtype, blocksize, members, n, a.g, nested)) return rc;
    const int na = MBNB_BATCH_NOT_APPLICABLE;
    DownArgs d;
    d.x = x;
    d.K = K;
    d.M = (int32_t)M;
    d.n = n;
    int rows = 0, rmax = 0;
    for (int i = 0; i < kMax; ++i) {
        d.first_row[i] = rows;
        d.m[i].a = nullptr;
        d.m[i].t = nullptr;
        d.m[i].R = 0;
        a.rows[i] = LoraRow{nullptr, nullptr, 0, 0.0f};
        if (i >= n || adapters[i].R == 0) continue;
        const mbnb_lora_adapter &ad = adapters[i];
        if (ad.R > MBNB_LORA_MAX_R) return fail(na, "%s: member %d has R = %d, 1 <= R <= %d is needed", who, i, ad.R, MBNB_LORA_MAX_R);
        if (!aligned(ad.a, 16)) return fail(na, "%s: member %d's a is not 16-byte aligned", who, i);
        if (!aligned(ad.b, 2)) return fail(na, "%s: member %d's b is not 2-byte aligned", who, i);
        if (!ad.t || !aligned(ad.t, 4)) return fail(na, "%s: member %d's t is NULL or not 4-byte aligned", who, i);
        if (!isfinite(ad.scaling)) return fail(na, "%s: member %d's scaling is not finite", who, i);
        d.m[i].a = ad.a;
        d.m[i].t = ad.t;
        d.m[i].R = ad.R;
        a.rows[i] = LoraRow{ad.b, ad.t, ad.R, ad.scaling};
        rows += ad.R;
        rmax = ad.R > rmax ? ad.R : rmax;
    }
    d.first_row[kMax] = rows;
    if (rows == 0) return fail(na, "%s: no member has an adapter (R > 0): the call is mbnb_batch_gemm4's", who);
    a.pitch = rmax | 1;      // odd: the 16 rows of a slice start in 16 different LDS banks
    hipStream_t s = (hipStream_t)stream;
    return MBNB_BATCH_FORMS(launch_lora, d, a, s);
}

}  // extern "C"
