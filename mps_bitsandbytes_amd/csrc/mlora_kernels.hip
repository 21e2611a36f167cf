// mlora_kernels.hip — the grouped 4-bit decode launches for 2 to 16 activation rows with a different un-merged LoRA adapter per row,
// and the C ABI of libmbnb_mlora.so (include/mbnb_mlora.h).
//
// libmbnb_batch.so serves these rows with the member's ONE adapter.  Continuous batching over one frozen 4-bit base hands a projection
// rows whose requests carry different adapters: every member has a bank of S adapters here, and row m uses slot ids[m], read ON THE
// DEVICE (the host never sees the ids, so a captured graph serves a new assignment once the ids tensor is overwritten).  Here:
//   k_lora_down_sel    t_g[m, j] = A_{g,ids[m]}[j, :] . x[m, :] in f32, one workgroup per (member, adapter row j, activation row m):
//                      k_lora_down_rows' chunking and summation chain (batch_kernels.hip) on the row of the slot;
//   k_skinny4_group<kEpiBank>  k_skinny4's workgroup behind the member table (skinny4_group.h: the template libmbnb_batch.so
//                      instantiates too, with the third of its epilogues) with a per-row rank-R epilogue: element (m, n) adds
//                      scaling_g[ids[m]] B_{g,ids[m]}[n, :] . t_g[m, :] to its f32 sum before the bias add and the double rounding.
// A row whose id is outside [0, S) reads nothing from the bank or from t and takes none of the epilogue's arithmetic.  Every sum runs
// in a fixed order (wave order through LDS, DPP wave sums, quarter order; nothing is accumulated in memory): a row with slot s gets
// the bits k_skinny4_group<kEpiLora> gives it with that one adapter.
#include "../../include/mbnb_mlora.h"
#include "host.h"
#include "skinny4_group.h"

static_assert(MBNB_MLORA_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_MLORA_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "the argument checks are shared");
static_assert(MBNB_MLORA_NOT_APPLICABLE == MBNB_GROUP_NOT_APPLICABLE, "one NOT_APPLICABLE");
static_assert(MBNB_MLORA_MAX_R == 64, "one wave-wide slice of a row of B and of t");
static_assert(MBNB_MLORA_MAX_M == 16, "one 16 x 16 MFMA tile holds every activation row");
static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");

namespace {

using mbnb::aligned;
using mbnb::BankRow;
using mbnb::Dot2;
using mbnb::dpp_wave_sum;
using mbnb::fail;
using mbnb::kEpiBank;
using mbnb::kLaunchBytes;
using mbnb::kPartBytes;
using mbnb::kRedBytes;
using mbnb::kRowBytes;
using mbnb::last_launch;
using mbnb::u32x4;

constexpr int kMax = mbnb::kGroupMax;
using SkinnyArgs = mbnb::SkinnyArgs<kEpiBank>;

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
template <typename T, int QT, bool NESTED>
int launch(const DownArgs &d, const SkinnyArgs &a, hipStream_t stream) {
    const int ku = (int)((a.g.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 down((unsigned)d.first_row[d.n], (unsigned)a.g.M), grid((unsigned)a.g.first_block[a.g.n]);
    // <= 58560 bytes at R = 64 (pitch 65, pitch_b 66): two workgroups fit a CU's LDS
    const size_t lds = (size_t)kRedBytes + kPartBytes + kRowBytes + (size_t)16 * a.pitch * 4 + (size_t)256 * a.pitch_b * 2;
    mbnb::with_ku(KU, [&](auto ku_) { hipLaunchKernelGGL((k_lora_down_sel<T, decltype(ku_)::value>), down, dim3(256), 0, stream, d); });
    hipLaunchKernelGGL((mbnb::k_skinny4_group<T, QT, NESTED, kEpiBank>), grid, dim3(1024), lds, stream, a);
    const int rc = mbnb::launch_status("mbnb_mlora_gemm4");
    if (rc == 0)
        snprintf(last_launch(), kLaunchBytes, "lora_down_sel G%d R%d M%d ku%d/KU%d + skinny_mlora G%d M%d", d.n, d.first_row[d.n], a.g.M, ku, KU, a.g.n,
                 a.g.M);
    return rc;
}

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
    if (const int rc = mbnb::skinny_argument_errors(who, x, M, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (!banks) return fail(MBNB_MLORA_ERR_ARG, "%s: NULL bank table", who);
    if (!ids) return fail(MBNB_MLORA_ERR_ARG, "%s: NULL ids", who);
    for (int i = 0; i < n; ++i) {
        const mbnb_mlora_bank &bk = banks[i];
        if (bk.R < 0 || bk.S < 0) return fail(MBNB_MLORA_ERR_SHAPE, "%s: member %d has R = %d, S = %d", who, i, bk.R, bk.S);
        if (bk.R > 0 && (!bk.a || !bk.b)) return fail(MBNB_MLORA_ERR_ARG, "%s: member %d has R = %d with a NULL a or b", who, i, bk.R);
    }
    // ---- the conditions of the fused launches: mbnb_batch_gemm4's (skinny4_group.h: the one place they live), then the ids' and the banks'
    const int na = MBNB_MLORA_NOT_APPLICABLE;
    SkinnyArgs a;
    bool nested;
    if (const int rc = mbnb::skinny_conditions(who, na, MBNB_MLORA_MIN_M, MBNB_MLORA_MAX_M, x, M, K, dtype, blocksize, members, n, a.g, nested)) return rc;
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
    return MBNB_GROUP_FORMS(dtype, quant_type, nested, launch, d, a, s);
}

}  // extern "C"
