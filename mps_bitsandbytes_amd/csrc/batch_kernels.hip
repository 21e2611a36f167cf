// batch_kernels.hip — the grouped 4-bit decode launches for 2 to 16 activation rows and the C ABI of libmbnb_batch.so
// (include/mbnb_batch.h).
//
// libmbnb_group.so and libmbnb_lora.so fuse the layers that share an activation ROW.  A serving loop hands every projection 2 to 16
// rows per step, and there mbnb_matmul_4bit streams each weight through k_skinny4 (matmul4_kernels.hip), one launch per layer, and
// an un-merged adapter costs four torch launches more.  Here:
//   k_skinny4_group<kEpiNone>  k_skinny4's workgroup (MT = 1, NR = 1: 16 weight rows x all M activation rows, 16 waves over the
//                              128-k blocks) behind a member table: ONE launch for up to 16 layers;
//   k_lora_down_rows           t_g[m, j] = A_g[j, :] . x[m, :] in f32, one workgroup per adapter row of every member (k_lora_down's
//                              chunking and summation chain, the row of A held in registers over the M activation rows);
//   k_skinny4_group<kEpiLora>  the same workgroup with a rank-R epilogue: element (m, n) adds scaling_g B_g[n, :] . t_g[m, :] to its
//                              f32 sum before the bias add and the double rounding.
// k_skinny4_group, its member table and the host checks of a 2 to 16 row call are in skinny4_group.h, shared with libmbnb_mlora.so;
// this file instantiates the first two epilogues and holds k_lora_down_rows.
// Every sum runs in a fixed order (wave order through LDS, DPP wave sums, quarter order; no atomics).
#include "../../include/mbnb_batch.h"
#include "host.h"
#include "skinny4_group.h"

static_assert(MBNB_BATCH_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_BATCH_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "the argument checks are shared");
static_assert(MBNB_BATCH_NOT_APPLICABLE == MBNB_GROUP_NOT_APPLICABLE && MBNB_BATCH_NOT_APPLICABLE == MBNB_LORA_NOT_APPLICABLE, "one NOT_APPLICABLE");
static_assert(MBNB_LORA_MAX_R == mbnb::kLoraMaxR, "the epilogue's slices");
static_assert(MBNB_BATCH_MAX_M == 16, "one 16 x 16 MFMA tile holds every activation row");
static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");

namespace {

using mbnb::BatchArgs;
using mbnb::Dot2;
using mbnb::dpp_wave_sum;
using mbnb::kEpiLora;
using mbnb::kEpiNone;
using mbnb::kLaunchBytes;
using mbnb::kPartBytes;
using mbnb::kRedBytes;
using mbnb::last_launch;
using mbnb::SkinnyArgs;
using mbnb::u32x4;

constexpr int kMax = mbnb::kGroupMax;

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
static_assert(sizeof(SkinnyArgs<kEpiLora>) + sizeof(DownArgs) <= 4096, "both tables must fit the kernel-argument segment");
static_assert(sizeof(SkinnyArgs<kEpiNone>) <= 4096, "the member table must fit the kernel-argument segment");

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
template <typename T, int QT, bool NESTED>
int launch(const BatchArgs &g, hipStream_t stream) {
    SkinnyArgs<kEpiNone> a;
    a.g = g;
    hipLaunchKernelGGL((mbnb::k_skinny4_group<T, QT, NESTED, kEpiNone>), dim3((unsigned)g.first_block[g.n]), dim3(1024), kRedBytes, stream, a);
    const int rc = mbnb::launch_status("mbnb_batch_gemm4");
    if (rc == 0) snprintf(last_launch(), kLaunchBytes, "skinny_group G%d M%d", g.n, g.M);
    return rc;
}

template <typename T, int QT, bool NESTED>
int launch_lora(const DownArgs &d, const SkinnyArgs<kEpiLora> &a, hipStream_t stream) {
    const int ku = (int)((a.g.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 down((unsigned)d.first_row[d.n]), grid((unsigned)a.g.first_block[a.g.n]);
    const size_t lds = (size_t)kRedBytes + kPartBytes + (size_t)2 * 16 * a.pitch * 4;      // <= 53376 bytes at pitch 257
    mbnb::with_ku(KU, [&](auto ku_) { hipLaunchKernelGGL((k_lora_down_rows<T, decltype(ku_)::value>), down, dim3(256), 0, stream, d); });
    hipLaunchKernelGGL((mbnb::k_skinny4_group<T, QT, NESTED, kEpiLora>), grid, dim3(1024), lds, stream, a);
    const int rc = mbnb::launch_status("mbnb_batch_gemm4_lora");
    if (rc == 0)
        snprintf(last_launch(), kLaunchBytes, "lora_down_rows G%d R%d M%d ku%d/KU%d + skinny_group_lora G%d M%d", d.n, d.first_row[d.n], d.M, ku, KU,
                 a.g.n, a.g.M);
    return rc;
}

}  // namespace

extern "C" {

int mbnb_batch_abi_version(void) { return MBNB_BATCH_ABI_VERSION; }

const char *mbnb_batch_last_error(void) { return mbnb::last_error(); }

const char *mbnb_batch_last_launch(void) { return last_launch(); }

int mbnb_batch_gemm4(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members, int n, int flags,
                     void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_batch_gemm4";
    if (const int rc = mbnb::skinny_argument_errors(who, x, M, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    // the conditions of the fused launch (skinny4_group.h: the one place they live)
    const int na = MBNB_BATCH_NOT_APPLICABLE;
    BatchArgs a;
    bool nested;
    if (const int rc = mbnb::skinny_conditions(who, na, MBNB_BATCH_MIN_M, MBNB_BATCH_MAX_M, x, M, K, dtype, blocksize, members, n, a, nested)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return MBNB_GROUP_FORMS(dtype, quant_type, nested, launch, a, s);
}

int mbnb_batch_gemm4_lora(const void *x, int64_t M, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members,
                          const mbnb_lora_adapter *adapters, int n, int flags, void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_batch_gemm4_lora";
    // ---- argument errors: mbnb_batch_gemm4's, then the adapter table's
    if (const int rc = mbnb::skinny_argument_errors(who, x, M, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (const int rc = mbnb::adapter_argument_errors(who, adapters, n)) return rc;
    // ---- the conditions of the fused launches: mbnb_batch_gemm4's, then the adapters' (gemv4_group.h)
    const int na = MBNB_BATCH_NOT_APPLICABLE;
    SkinnyArgs<kEpiLora> a;
    bool nested;
    if (const int rc = mbnb::skinny_conditions(who, na, MBNB_BATCH_MIN_M, MBNB_BATCH_MAX_M, x, M, K, dtype, blocksize, members, n, a.g, nested)) return rc;
    DownArgs d;
    d.x = x;
    d.K = K;
    d.M = (int32_t)M;
    d.n = n;
    if (const int rc = mbnb::adapter_conditions(who, na, "mbnb_batch_gemm4", adapters, n, d, a.rows)) return rc;
    int rmax = 0;
    for (int i = 0; i < kMax; ++i) {
        d.m[i].R = a.rows[i].R;
        rmax = a.rows[i].R > rmax ? a.rows[i].R : rmax;
    }
    a.pitch = rmax | 1;      // odd: the 16 rows of a slice start in 16 different LDS banks
    hipStream_t s = (hipStream_t)stream;
    return MBNB_GROUP_FORMS(dtype, quant_type, nested, launch_lora, d, a, s);
}

}  // extern "C"
