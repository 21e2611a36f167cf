// skinny4_group.h — what libmbnb_batch.so (batch_kernels.hip) and libmbnb_mlora.so (mlora_kernels.hip) share: the member table of the
// 2 to 16 row launches, k_skinny4_group -- k_skinny4's workgroup behind that table, with its three epilogues -- the LDS sizes, and the
// host checks of such a call.
//
// The three epilogues sit behind `if constexpr (EPI == ...)` at the places they take in the body; every instantiation has the
// instruction stream, registers, LDS and kernel-argument segment it had when the two libraries each carried a kernel of their own
// (DESIGN.md 24 holds the comparison).
//
// Host part: include host.h first (fail / aligned / is16), as the one source file of a library does.
#pragma once
#include "gemv4_group.h"

namespace mbnb {

constexpr int kSkinnyWaves = 16;                   // waves of a k_skinny4 workgroup
constexpr int kRedBytes = kSkinnyWaves * 1024;     // [16 waves][256] f32 partial tiles
constexpr int kPartBytes = 4 * 1024;               // an epilogue's [4 quarters][256] f32 partial up-sums
constexpr int kRowBytes = 2 * 16 * 4;              // kEpiBank, per activation row: f32 scaling of its slot, then i32 "has an adapter"

// the member table: member i owns the workgroups [first_block[i], first_block[i+1]); entries past n hold the total
struct BatchArgs {
    const void *x;      // [M, K] row-major in the call's dtype
    int64_t K;
    int32_t M;
    int32_t bs_shift;   // log2(blocksize)
    int32_t first_block[kGroupMax + 1];
    int32_t n;
    mbnb_group_member m[kGroupMax];
};

// a member's bank as the kEpiBank epilogue sees it: slot s's B is the [N, R] block s of b
struct BankRow {
    const void *b;
    const float *scaling;
    const float *t;
    int32_t R;
    int32_t S;
};

// the epilogue of k_skinny4_group: none; the member's ONE adapter (a LoraRow whose t is [M, R]); a bank of adapters per member with
// row m's slot in ids[m]
constexpr int kEpiNone = 0, kEpiLora = 1, kEpiBank = 2;

// the kernel's arguments.  kEpiLora: pitch is the row pitch, in floats, of the two LDS slices (odd and >= every R).  kEpiBank: pitch:
// floats per LDS row of t (odd, >= every R); pitch_b: 16-bit elements per LDS row of B (an odd number of dwords, >= every R)
template <int EPI> struct SkinnyArgs {
    BatchArgs g;
};
template <> struct SkinnyArgs<kEpiLora> {
    BatchArgs g;
    LoraRow rows[kGroupMax];
    int32_t pitch;
};
template <> struct SkinnyArgs<kEpiBank> {
    BatchArgs g;
    BankRow rows[kGroupMax];
    const int32_t *ids;
    int32_t pitch;
    int32_t pitch_b;
};

namespace {      // the kernel's linkage stays internal to the library that instantiates it

// One workgroup = 16 waves x 16 weight rows of ONE member x all M <= 16 activation rows.
//
// From the member's pointers on THIS IS A COPY of the body of k_skinny4<T, T, QT, NESTED, MT = 1, NR = 1> (matmul4_kernels.hip), kept
// in step BY HAND as group_row (gemv4_group.h) is with k_gemv4_lean, for the reason given there: that kernel's schedule must not
// move.  It is the ONLY copy: every 2 to 16 row launch of both libraries is an instantiation of this template.  K_weight == K here (the
// libraries' condition).  tests/test_gpu_batch.py holds it equal to k_skinny4 bit for bit, tests/test_gpu_mlora.py kEpiBank to kEpiLora.
//
// The member compare chain is written out here (and in the down-projection kernels): routed through a __forceinline__ function it
// moved the instruction stream of every instantiation.
//
// kEpiLora: with R > 0 wave w requests, before the k-loop, row n0 + w of B (dead rows clamped) and row w of t -- lane l takes
// j = 64 c + l for c < ceil(R / 64) through range-checked descriptors, so j >= R and rows m >= M read zeros -- and parks them in LDS
// beside the partial tiles.  After the wave-order reduction the element (m, n) of thread e = tid & 255 is shared by the four threads
// e + 256 qr: quarter qr adds f32(B[n, j]) * t[m, j] (a rounded product, then the add) for j = qr, qr + 4, ... in rising j, and thread
// e forms u = ((p0 + p1) + p2) + p3, then (s + scaling * u) + bias.  R == 0 (workgroup-uniform) takes none of this.
//
// kEpiBank: with R > 0 wave w < M resolves s = ids[w] first of all (one load, made scalar), and with 0 <= s < S requests, before the
// k-loop, row w of t (lane l takes j = l) and the 16 rows n0 ... n0 + 15 of B_{g,s} (request c: row n0 + c, lane l its element j = l)
// through range-checked descriptors, so rows past N read zeros, and its slot's scaling; after the k-loop it parks them in LDS, B in
// the 16-bit dtype keyed by (n, m).  The quarter sums are kEpiLora's, from an exact 0, with the row's own scaling.  A row without an
// adapter takes none of this arithmetic; R == 0 (workgroup-uniform) takes none of the code.  Every thread meets every barrier.
template <typename T, int QT, bool NESTED, int EPI>
__global__ __launch_bounds__(1024) void k_skinny4_group(const SkinnyArgs<EPI> args) {
    constexpr int WV = kSkinnyWaves;
    constexpr int kMax = kGroupMax;
    __shared__ float lut[16];
    // [WV][256] f32; kEpiLora: + [4][256] f32 + t [16][pitch] + B [16][pitch];
    // kEpiBank: + [4][256] f32 + rows + t [16][pitch] f32 + B [16 n][16 m][pitch_b] 16 bit
    extern __shared__ __attribute__((aligned(16))) char red_raw[];
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
    // the epilogues' state that lives across the k-loop (an instantiation that does not use a register does not have it)
    constexpr int kSlices = kLoraMaxR / 64;
    int R = 0, wv = 0, slot_v = -1;
    bool asks = false, has = false;
    uint16_t lb[kSlices] = {};      // kEpiLora: this wave's slices of its row of B
    float lt[kSlices] = {};         // this wave's slices of its row of t (kEpiBank: one)
    uint32_t lbk[16] = {};          // kEpiBank: one register per row of B, untouched until they are parked: nothing before the k-loop waits for them
    float lsc = 0.0f;               // kEpiBank: the scaling of this wave's slot
    // kEpiBank: this wave's row of the batch and its slot: requested before the weights and used after their first request, so that the
    // wait for it is neither a wait for HBM nor a delay of that request
    if constexpr (EPI == kEpiBank) {
        R = args.rows[g].R;
        wv = __builtin_amdgcn_readfirstlane(wave);
        asks = R > 0 && wv < M;
        slot_v = asks ? __builtin_nontemporal_load(args.ids + wv) : -1;
    }

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

    // kEpiLora: this wave's slices of row n0 + wave of B (16-bit loads in a range of 2 R bytes) and of row `wave` of t (32-bit loads in a
    // range of 4 R bytes, 0 bytes for a row the batch does not have)
    if constexpr (EPI == kEpiLora) {
        const LoraRow &lr = args.rows[g];
        R = lr.R;
        if (R > 0) {
            wv = __builtin_amdgcn_readfirstlane(wave);
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
    // kEpiBank: the operands of row `wave`: 16 rows of the slot's B (16-bit loads in a range of live rows x 2 R bytes), the row of t
    // (32-bit loads in a range of 4 R bytes) and the slot's scaling
    if constexpr (EPI == kEpiBank) {
        const BankRow &bank = args.rows[g];
        const int slot = __builtin_amdgcn_readfirstlane(slot_v);
        has = asks && (unsigned)slot < (unsigned)bank.S;      // wave-uniform; false for R == 0 and for a row the batch does not have
        if (has) {
            const int64_t live = N - n0 < 16 ? N - n0 : 16;
            const char *brow = static_cast<const char *>(bank.b) + ((int64_t)slot * N + n0) * R * 2;
            const float *trow = bank.t + (int64_t)wv * R;
            const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(brow), 0, (int)live * R * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(trow), 0, R * 4, 0x00020000);
#pragma unroll
            for (int c = 0; c < 16; c++) lbk[c] = __builtin_amdgcn_raw_buffer_load_b16(rs_b, (c * R + lane) * 2, 0, 0);      // the row in the checked offset
            lt[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, lane * 4, 0, 0));
            lsc = bank.scaling[slot];
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
    // ---- reduce the WV partial 16 x 16 tiles in wave order; the epilogues park their operands beside them
    *reinterpret_cast<f32x4 *>(red + (wave * 256 + lane * 4)) = acc;
    float *part = red + kRedBytes / 4;
    float *scal = part + kPartBytes / 4;                       // kEpiBank: [16] the rows' scalings
    int *flag = reinterpret_cast<int *>(scal + 16);            // kEpiBank: [16] 1: the row has an adapter
    float *ts = EPI == kEpiBank ? scal + kRowBytes / 4 : scal;
    int pitch = 0, pitch_b = 0;
    if constexpr (EPI == kEpiLora) {
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
    if constexpr (EPI == kEpiBank) {
        pitch = args.pitch;
        pitch_b = args.pitch_b;
        uint16_t *bs = reinterpret_cast<uint16_t *>(ts + 16 * pitch);
        if (R > 0) {
            if (lane == 0) {
                scal[wave] = lsc;
                flag[wave] = has ? 1 : 0;
            }
            if (has && lane < R) {
                ts[wave * pitch + lane] = lt[0];
#pragma unroll
                for (int c = 0; c < 16; c++) bs[(c * 16 + wave) * pitch_b + lane] = (uint16_t)lbk[c];
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
        for (int i = 0; i < WV; i++) s += red[i * 256 + e];
    }
    if constexpr (EPI == kEpiLora) {
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
    if constexpr (EPI == kEpiBank) {
        if (R > 0) {      // workgroup-uniform: every thread meets the barrier
            const uint16_t *bs = reinterpret_cast<const uint16_t *>(ts + 16 * pitch);
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
    }
    if (threadIdx.x < 256 && n < N && m < M) {
        const float v = s + (bias ? to_f32(bias[n]) : 0.0f);
        out[m * N + n] = from_f32<T>(to_f32(from_f32<T>(v)));
    }
}

}  // namespace

// ---------------------------------------------------------------- host side: the checks of a 2 to 16 row call, for both libraries
// skinny_argument_errors: 0, or the negative code of an argument error: mbnb_group_gemv4's checks of a member table, and M.
static int skinny_argument_errors(const char *who, const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize,
                                  const mbnb_group_member *members, int n, int flags) {
    if (const int rc = group_argument_errors(who, x, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (M <= 0) return fail(MBNB_GROUP_ERR_SHAPE, "%s: M = %lld", who, (long long)M);
    return 0;
}

// The conditions of the fused launch: this is the one place they live.  0 with `a` filled and `nested` set, or `not_applicable` after
// recording the reason; nothing is dereferenced.
//
// They are a subset of the shapes for which launch_matmul4 (matmul4_kernels.hip) takes "skinny MT1 NR1": its fast_layout (16-bit,
// blocksize >= 32, K_weight % 32 == 0, K % 8 == 0, A and packed 16-byte aligned), then skinny (2 <= M, K % 128 == 0, M <= 16 for
// MT = 1).  gemm_small_shape needs M > 16 and the GEMV branch needs !skinny, so neither takes such a call first: a call that is
// fused here is a call whose members mbnb_matmul_4bit would have sent to that same instantiation.
static int skinny_conditions(const char *who, int not_applicable, int min_m, int max_m, const void *x, int64_t M, int64_t K, int dtype,
                             int blocksize, const mbnb_group_member *members, int n, BatchArgs &a, bool &nested) {
    const int na = not_applicable;
    if (M < min_m || M > max_m) return fail(na, "%s: %d <= M <= %d is needed, got M = %lld", who, min_m, max_m, (long long)M);
    if (!is16(dtype)) return fail(na, "%s: a 16-bit dtype is needed, got dtype %d", who, dtype);
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
    for (int i = n; i <= kGroupMax; ++i) a.first_block[i] = (int32_t)blocks;
    for (int i = n; i < kGroupMax; ++i) a.m[i] = mbnb_group_member{};
    return 0;
}

}  // namespace mbnb
