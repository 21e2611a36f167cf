// mlora_kernels.hip — the grouped 4-bit decode launches for 2 to 16 activation rows with a different un-merged LoRA adapter per row,
// and the C ABI of libmbnb_mlora.so (include/mbnb_mlora.h).
//
// libmbnb_batch.so serves these rows with the member's ONE adapter.  Continuous batching over one frozen 4-bit base hands a projection
// rows whose requests carry different adapters: every member has a bank of S adapters here, and row m uses slot ids[m], read ON THE
// DEVICE (the host never sees the ids, so a captured graph serves a new assignment once the ids tensor is overwritten).  Here:
//   k_lora_down_sel    t_g[m, j] = A_{g,ids[m]}[j, :] . x[m, :] in f32, one workgroup per (member, adapter row j, activation row m):
//                      k_lora_down_rows' chunking and summation chain (batch_kernels.hip) on the row of the slot;
//   k_skinny4_mlora    k_skinny4's workgroup behind the member table (the third copy, after k_skinny4_group) with a per-row rank-R
//                      epilogue: element (m, n) adds scaling_g[ids[m]] B_{g,ids[m]}[n, :] . t_g[m, :] to its f32 sum before the
//                      bias add and the double rounding.
// A row whose id is outside [0, S) reads nothing from the bank or from t and takes none of the epilogue's arithmetic.  Every sum runs
// in a fixed order (wave order through LDS, DPP wave sums, quarter order; nothing is accumulated in memory): a row with slot s gets
// the bits k_skinny4_group<LORA> gives it with that one adapter.
#include "../../include/mbnb_mlora.h"
#include "host.h"
#include "gemv4_group.h"

static_assert(MBNB_MLORA_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_MLORA_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "the argument checks are shared");
static_assert(MBNB_MLORA_NOT_APPLICABLE == MBNB_GROUP_NOT_APPLICABLE, "one NOT_APPLICABLE");
static_assert(MBNB_MLORA_MAX_R == 64, "one wave-wide slice of a row of B and of t");
static_assert(MBNB_MLORA_MAX_M == 16, "one 16 x 16 MFMA tile holds every activation row");
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
using mbnb::Mfma16;
using mbnb::pack2;
using mbnb::to_f32;
using mbnb::u32x4;

constexpr int kMax = mbnb::kGroupMax;
constexpr int kWaves = 16;                      // waves of a k_skinny4 workgroup
constexpr int kRedBytes = kWaves * 1024;        // [16 waves][256] f32 partial tiles
constexpr int kPartBytes = 4 * 1024;            // [4 quarters][256] f32 partial up-sums
constexpr int kRowBytes = 2 * 16 * 4;           // per activation row: f32 scaling of its slot, then i32 "has an adapter"

// the member table of k_skinny4_group (batch_kernels.hip): member i owns the workgroups [first_block[i], first_block[i+1]); entries
// past n hold the total
struct BatchArgs {
    const void *x;      // [M, K] row-major in the call's dtype
    int64_t K;
    int32_t M;
    int32_t bs_shift;   // log2(blocksize)
    int32_t first_block[kMax + 1];
    int32_t n;
    mbnb_group_member m[kMax];
};

// a member's bank as the epilogue sees it: slot s's B is the [N, R] block s of b
struct BankRow {
    const void *b;
    const float *scaling;
    const float *t;
    int32_t R;
    int32_t S;
};

// k_skinny4_mlora's arguments; pitch: floats per LDS row of t (odd, >= every R); pitch_b: 16-bit elements per LDS row of B (an odd
// number of dwords, >= every R)
struct SkinnyArgs {
    BatchArgs g;
    BankRow rows[kMax];
    const int32_t *ids;
    int32_t pitch;
    int32_t pitch_b;
};

// k_lora_down_sel's arguments: member i owns blockIdx.x (= adapter rows) in [first_row[i], first_row[i+1]); blockIdx.y is the activation row
struct DownArgs {
    const void *x;
    const int32_t *ids;
    int64_t K;
    int32_t n;
    int32_t first_row[kMax + 1];
    struct {
        const void *a;
        float *t;
        int32_t R;
        int32_t S;
    } m[kMax];
};
static_assert(sizeof(SkinnyArgs) + sizeof(DownArgs) <= 4096, "both tables must fit the kernel-argument segment");

// One workgroup = 16 waves x 16 weight rows of ONE member x all M <= 16 activation rows.
//
// From the member's pointers on THIS IS A COPY of the body of k_skinny4<T, T, QT, NESTED, MT = 1, NR = 1> (matmul4_kernels.hip), the
// third after k_skinny4_group (batch_kernels.hip), kept in step BY HAND for the reason given in gemv4_group.h: that kernel's schedule
// must not move.  K_weight == K here (the library's condition).  tests/test_gpu_mlora.py holds the copies equal bit for bit.
//
// The epilogue: with R > 0 wave w < M resolves s = ids[w] first of all (one load, made scalar), and with 0 <= s < S requests, before the
// k-loop, row w of t (lane l takes j = l) and the 16 rows n0 ... n0 + 15 of B_{g,s} (request c: row n0 + c, lane l its element j = l)
// through range-checked descriptors, so rows past N read zeros, and its slot's scaling; after the k-loop it parks them in LDS, B in
// the 16-bit dtype keyed by (n, m).  After the wave-order reduction the element (m, n) of thread e = tid & 255 is shared by the four
// threads e + 256 qr: quarter qr adds f32(B[n, j]) * t[m, j] (a rounded product, then the add) for j = qr, qr + 4, ... in rising j from an
// exact 0, and thread e forms u = ((p0 + p1) + p2) + p3, then (s + scaling * u) + bias.  A row without an adapter takes none of this
// arithmetic; R == 0 (workgroup-uniform) takes none of the code.  Every thread meets every barrier.
template <typename T, int QT, bool NESTED>
__global__ __launch_bounds__(1024) void k_skinny4_mlora(const SkinnyArgs args) {
    constexpr int WV = kWaves;
    __shared__ float lut[16];
    extern __shared__ __attribute__((aligned(16))) char red_raw[];   // [WV][256] f32 + [4][256] f32 + rows + t [16][pitch] f32 + B [16 n][16 m][pitch_b] 16 bit
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
    // this wave's row of the batch and its slot: requested before the weights and used after their first request, so that the wait for
    // it is neither a wait for HBM nor a delay of that request
    const BankRow &bank = args.rows[g];
    const int R = bank.R;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const bool asks = R > 0 && wv < M;
    const int slot_v = asks ? __builtin_nontemporal_load(args.ids + wv) : -1;

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

    // the epilogue's operands of row `wave`: 16 rows of the slot's B (16-bit loads in a range of live rows x 2 R bytes), the row of t
    // (32-bit loads in a range of 4 R bytes) and the slot's scaling
    const int slot = __builtin_amdgcn_readfirstlane(slot_v);
    const bool has = asks && (unsigned)slot < (unsigned)bank.S;      // wave-uniform; false for R == 0 and for a row the batch does not have
    uint32_t lb[16] = {};      // one register each, untouched until they are parked: nothing before the k-loop waits for them
    float lt = 0.0f, lsc = 0.0f;
    if (has) {
        const int64_t live = N - n0 < 16 ? N - n0 : 16;
        const char *brow = static_cast<const char *>(bank.b) + ((int64_t)slot * N + n0) * R * 2;
        const float *trow = bank.t + (int64_t)wv * R;
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(brow), 0, (int)live * R * 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(trow), 0, R * 4, 0x00020000);
#pragma unroll
        for (int c = 0; c < 16; c++) lb[c] = __builtin_amdgcn_raw_buffer_load_b16(rs_b, (c * R + lane) * 2, 0, 0);      // the row in the checked offset
        lt = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, lane * 4, 0, 0));
        lsc = bank.scaling[slot];
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
    float *scal = part + kPartBytes / 4;                       // [16] the rows' scalings
    int *flag = reinterpret_cast<int *>(scal + 16);            // [16] 1: the row has an adapter
    float *ts = scal + kRowBytes / 4;
    const int pitch = args.pitch, pitch_b = args.pitch_b;
    uint16_t *bs = reinterpret_cast<uint16_t *>(ts + 16 * pitch);
    if (R > 0) {
        if (lane == 0) {
            scal[wave] = lsc;
            flag[wave] = has ? 1 : 0;
        }
        if (has && lane < R) {
            ts[wave * pitch + lane] = lt;
#pragma unroll
            for (int c = 0; c < 16; c++) bs[(c * 16 + wave) * pitch_b + lane] = (uint16_t)lb[c];
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
        for (int wv2 = 0; wv2 < WV; wv2++) s += red[wv2 * 256 + e];
    }
    if (R > 0) {      // workgroup-uniform: every thread meets the barrier
        const bool mine = flag[m] != 0;
        float p = 0.0f;
        if (mine) {
            const uint16_t *bn = bs + (nl * 16 + (int)m) * pitch_b;
            const float *tm = ts + (int)m * pitch;
            for (int j = (int)(threadIdx.x >> 8); j < R; j += 4) p += to_f32(__builtin_bit_cast(T, bn[j])) * tm[j];      // a rounded product, then the add (-ffp-contract=off)
        }
        part[threadIdx.x] = p;
        __syncthreads();
        if (threadIdx.x < 256 && mine) {
            const float up = ((part[e] + part[256 + e]) + part[512 + e]) + part[768 + e];
            s += scal[m] * up;
        }
    }
    if (threadIdx.x < 256 && n < N && m < M) {
        const float v = s + (bias ? to_f32(bias[n]) : 0.0f);
        out[m * N + n] = from_f32<T>(to_f32(from_f32<T>(v)));
    }
}

// t_g[m, j] = A_{g,s}[j, :] . x[m, :] with s = ids[m], for blockIdx.y = m; nothing for a row whose id is outside the bank.  One
// workgroup of 256 threads; the K chunking is k_lora_down's: thread tid takes the 16 bytes at k = 2048 u + 8 tid of the row of A and of
// x[m], for u < KU, through descriptors of K * 2 bytes (a partial last chunk reads zeros).  The chain is k_lora_down_rows' for that m:
// Dot2 over the thread's chunks in rising u, the DPP wave sum, the four wave sums added in wave order by one lane.
template <typename T, int KU>
__global__ __launch_bounds__(256) void k_lora_down_sel(const DownArgs a) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = (int)blockIdx.x;
    const int m = (int)blockIdx.y;
    int g = 0, first = 0;      // the compare chain of k_gemv4_group: scalar
#pragma unroll
    for (int i = 1; i < kMax; i++) {
        const int fr = a.first_row[i];
        g = fr <= blk ? i : g;
        first = fr <= blk ? fr : first;
    }
    g = __builtin_amdgcn_readfirstlane(g);
    const int slot = __builtin_amdgcn_readfirstlane(a.ids[m]);
    if ((unsigned)slot >= (unsigned)a.m[g].S) return;      // workgroup-uniform: no adapter for this row, nothing stored
    const int64_t K = a.K;
    const int R = a.m[g].R;
    const int j = blk - first;
    const char *row = static_cast<const char *>(a.m[g].a) + ((int64_t)slot * R + j) * K * 2;
    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(row), 0, (int)(K * 2), 0x00020000);
    const char *xr = static_cast<const char *>(a.x) + (int64_t)m * K * 2;
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xr), 0, (int)(K * 2), 0x00020000);
    u32x4 aq[KU], xq[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) aq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, tid * 16, u * 4096, 2));    // aux 2: nt
#pragma unroll
    for (int u = 0; u < KU; u++) xq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, tid * 16, u * 4096, 0));
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < KU; u++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc = Dot2<T>::run(aq[u][c], xq[u][c], acc);
    const float s = dpp_wave_sum(acc);
    if (lane == 63) part[wave] = s;
    __syncthreads();
    if (tid == 0) a.m[g].t[(int64_t)m * R + j] = ((part[0] + part[1]) + part[2]) + part[3];
}

// ---------------------------------------------------------------- host side
constexpr int kLaunchBytes = 128;
char *last_launch() {
    static thread_local char text[kLaunchBytes] = "";
    return text;
}

template <typename T, int QT, bool NESTED>
int launch(const DownArgs &d, const SkinnyArgs &a, hipStream_t stream) {
    const int ku = (int)((a.g.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 down((unsigned)d.first_row[d.n], (unsigned)a.g.M), grid((unsigned)a.g.first_block[a.g.n]);
    // <= 58560 bytes at R = 64 (pitch 65, pitch_b 66): two workgroups fit a CU's LDS
    const size_t lds = (size_t)kRedBytes + kPartBytes + kRowBytes + (size_t)16 * a.pitch * 4 + (size_t)256 * a.pitch_b * 2;
#define MBNB_MLORA_DOWN(KU_)                                                                   \
    case KU_:                                                                                  \
        hipLaunchKernelGGL((k_lora_down_sel<T, KU_>), down, dim3(256), 0, stream, d);          \
        break
    switch (KU) {
        MBNB_MLORA_DOWN(1);
        MBNB_MLORA_DOWN(2);
        MBNB_MLORA_DOWN(3);
        MBNB_MLORA_DOWN(4);
        MBNB_MLORA_DOWN(6);
        MBNB_MLORA_DOWN(8);
    }
#undef MBNB_MLORA_DOWN
    hipLaunchKernelGGL((k_skinny4_mlora<T, QT, NESTED>), grid, dim3(1024), lds, stream, a);
    const int rc = mbnb::launch_status("mbnb_mlora_gemm4");
    if (rc == 0)
        snprintf(last_launch(), kLaunchBytes, "lora_down_sel G%d R%d M%d ku%d/KU%d + skinny_mlora G%d M%d", d.n, d.first_row[d.n], a.g.M, ku, KU, a.g.n,
                 a.g.M);
    return rc;
}

// The conditions of the base launch: those of mbnb_batch_gemm4 (batch_kernels.hip), restated here because each library keeps its
// conditions next to its launch.  0 with `a` filled and `nested` set, or MBNB_MLORA_NOT_APPLICABLE after recording the reason; nothing
// is dereferenced.
int conditions(const char *who, const void *x, int64_t M, int64_t K, int dtype, int blocksize, const mbnb_group_member *members, int n, BatchArgs &a,
               bool &nested) {
    const int na = MBNB_MLORA_NOT_APPLICABLE;
    if (M < MBNB_MLORA_MIN_M || M > MBNB_MLORA_MAX_M)
        return fail(na, "%s: %d <= M <= %d is needed, got M = %lld", who, MBNB_MLORA_MIN_M, MBNB_MLORA_MAX_M, (long long)M);
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

#define MBNB_MLORA_FORMS(FN, ...)                                                                                                   \
    (dtype == MBNB_GROUP_F16                                                                                                        \
         ? (quant_type == MBNB_GROUP_NF4 ? (nested ? FN<f16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<f16_t, MBNB_NF4, false>(__VA_ARGS__))    \
                                         : (nested ? FN<f16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<f16_t, MBNB_FP4, false>(__VA_ARGS__)))   \
         : (quant_type == MBNB_GROUP_NF4 ? (nested ? FN<bf16_t, MBNB_NF4, true>(__VA_ARGS__) : FN<bf16_t, MBNB_NF4, false>(__VA_ARGS__))  \
                                         : (nested ? FN<bf16_t, MBNB_FP4, true>(__VA_ARGS__) : FN<bf16_t, MBNB_FP4, false>(__VA_ARGS__))))

}  // namespace

extern "C" {

int mbnb_mlora_abi_version(void) { return MBNB_MLORA_ABI_VERSION; }

const char *mbnb_mlora_last_error(void) { return mbnb::last_error(); }

const char *mbnb_mlora_last_launch(void) { return last_launch(); }

int mbnb_mlora_gemm4(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members,
                     const mbnb_mlora_bank *banks, const int32_t *ids, int n, int flags, void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_mlora_gemm4";
    // ---- argument errors: mbnb_batch_gemm4's, then the bank table's and the ids'
    if (const int rc = mbnb::group_argument_errors(who, x, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (M <= 0) return fail(MBNB_MLORA_ERR_SHAPE, "%s: M = %lld", who, (long long)M);
    if (!banks) return fail(MBNB_MLORA_ERR_ARG, "%s: NULL bank table", who);
    if (!ids) return fail(MBNB_MLORA_ERR_ARG, "%s: NULL ids", who);
    for (int i = 0; i < n; ++i) {
        const mbnb_mlora_bank &bk = banks[i];
        if (bk.R < 0 || bk.S < 0) return fail(MBNB_MLORA_ERR_SHAPE, "%s: member %d has R = %d, S = %d", who, i, bk.R, bk.S);
        if (bk.R > 0 && (!bk.a || !bk.b)) return fail(MBNB_MLORA_ERR_ARG, "%s: member %d has R = %d with a NULL a or b", who, i, bk.R);
    }
    // ---- the conditions of the fused launches: mbnb_batch_gemm4's, then the ids' and the banks'
    SkinnyArgs a;
    bool nested;
    if (const int rc = conditions(who, x, M, K, dtype, blocksize, members, n, a.g, nested)) return rc;
    const int na = MBNB_MLORA_NOT_APPLICABLE;
    if (!aligned(ids, 4)) return fail(na, "%s: ids is not 4-byte aligned", who);
    DownArgs d;
    d.x = x;
    d.ids = ids;
    d.K = K;
    d.n = n;
    a.ids = ids;
    int rows = 0, rmax = 0;
    for (int i = 0; i < kMax; ++i) {
        d.first_row[i] = rows;
        d.m[i].a = nullptr;
        d.m[i].t = nullptr;
        d.m[i].R = 0;
        d.m[i].S = 0;
        a.rows[i] = BankRow{nullptr, nullptr, nullptr, 0, 0};
        if (i >= n || banks[i].R == 0) continue;
        const mbnb_mlora_bank &bk = banks[i];
        if (bk.R > MBNB_MLORA_MAX_R) return fail(na, "%s: member %d has R = %d, 1 <= R <= %d is needed", who, i, bk.R, MBNB_MLORA_MAX_R);
        if (bk.S < 1) return fail(na, "%s: member %d has S = %d slots, S >= 1 is needed", who, i, bk.S);
        if (!aligned(bk.a, 16)) return fail(na, "%s: member %d's a is not 16-byte aligned", who, i);
        if (!aligned(bk.b, 2)) return fail(na, "%s: member %d's b is not 2-byte aligned", who, i);
        if (!bk.scaling || !aligned(bk.scaling, 4)) return fail(na, "%s: member %d's scaling is NULL or not 4-byte aligned", who, i);
        if (!bk.t || !aligned(bk.t, 4)) return fail(na, "%s: member %d's t is NULL or not 4-byte aligned", who, i);
        d.m[i].a = bk.a;
        d.m[i].t = bk.t;
        d.m[i].R = bk.R;
        d.m[i].S = bk.S;
        a.rows[i] = BankRow{bk.b, bk.scaling, bk.t, bk.R, bk.S};
        rows += bk.R;
        rmax = bk.R > rmax ? bk.R : rmax;
    }
    d.first_row[kMax] = rows;
    if (rows == 0) return fail(na, "%s: no member has a bank (R > 0): the call is mbnb_batch_gemm4's", who);
    a.pitch = rmax | 1;                         // odd: the 16 rows of t start in 16 different LDS banks
    a.pitch_b = 2 * (((rmax + 1) / 2) | 1);     // an odd number of dwords per (n, m) row of B
    hipStream_t s = (hipStream_t)stream;
    return MBNB_MLORA_FORMS(launch, d, a, s);
}

}  // extern "C"
