// lora_kernels.hip — the grouped M = 1 decode GEMV with un-merged LoRA adapters and the C ABI of libmbnb_lora.so (include/mbnb_lora.h).
//
// A LoRA trained over a 4-bit base decodes with base(x) + s (x A^T) B^T per adapted projection: in torch ops, four small launches
// beside each 4-bit GEMV, each of which costs what a launch boundary costs (2.5 us against 4.9 us for a whole 4096^2
// layer).  One call here makes TWO launches for up to 16 layers that share x:
//   k_lora_down         t_g[j] = A_g[j, :] . x in f32, one workgroup per adapter row of every member;
//   k_gemv4_group_lora  k_gemv4_group's workgroup (gemv4_group.h) with the rank-R epilogue: row n adds scaling_g B_g[n, :] . t_g to its
//                       f32 accumulator before the bias add and the single rounding.
// Both sums run in a fixed order (DPP wave sums, the four wave sums of k_lora_down added in wave order by one lane; no atomics).
#include "../../include/mbnb_lora.h"
#include "host.h"
#include "gemv4_group.h"

static_assert(MBNB_LORA_ERR_ARG == MBNB_GROUP_ERR_ARG && MBNB_LORA_ERR_SHAPE == MBNB_GROUP_ERR_SHAPE, "the argument checks are shared");
static_assert(MBNB_LORA_NOT_APPLICABLE == MBNB_GROUP_NOT_APPLICABLE, "one NOT_APPLICABLE");
static_assert(MBNB_LORA_MAX_R == mbnb::kLoraMaxR, "the row epilogue's slices");
static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");

namespace {

using mbnb::Dot2;
using mbnb::dpp_wave_sum;
using mbnb::GroupArgs;
using mbnb::kLaunchBytes;
using mbnb::last_launch;
using mbnb::LoraRow;
using mbnb::u32x4;

constexpr int kMax = mbnb::kGroupMax;

// k_gemv4_group_lora's arguments: k_gemv4_group's, and the adapters by member
struct LoraArgs {
    GroupArgs g;
    LoraRow rows[kMax];
};

// k_lora_down's arguments: member i owns the workgroups (= adapter rows) [first_row[i], first_row[i+1]); entries past n hold the total
struct DownArgs {
    const void *x;
    int64_t K;
    int32_t first_row[kMax + 1];
    int32_t n;
    struct {
        const void *a;
        float *t;
    } m[kMax];
};
static_assert(sizeof(LoraArgs) + sizeof(DownArgs) <= 4096, "both tables must fit the kernel-argument segment");

// t_g[j] = A_g[j, :] . x.  One workgroup of 256 threads per adapter row; the K chunking is the GEMV's: thread tid takes the 16 bytes
// at k = 2048 u + 8 tid of both x and the row, for u < KU, through descriptors of K * 2 bytes (a partial last chunk reads zeros).
template <typename T, int KU>
__global__ __launch_bounds__(256) void k_lora_down(const DownArgs a) {
    __shared__ float part[4];
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
    const int j = blk - first;
    const char *row = static_cast<const char *>(a.m[g].a) + (int64_t)j * K * 2;
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.x), 0, (int)(K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(row), 0, (int)(K * 2), 0x00020000);
    u32x4 xq[KU], aq[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) {
        xq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, tid * 16, u * 4096, 0));
        aq[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, tid * 16, u * 4096, 2));    // aux 2: nt
    }
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < KU; u++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc = Dot2<T>::run(aq[u][c], xq[u][c], acc);
    const float s = dpp_wave_sum(acc);
    if (lane == 63) part[wave] = s;
    __syncthreads();
    if (tid == 0) a.m[g].t[j] = ((part[0] + part[1]) + part[2]) + part[3];
}

template <typename T, int QT, bool NESTED, int KU>
__global__ __launch_bounds__(256) void k_gemv4_group_lora(const LoraArgs a) {
    __shared__ float lut[16];
    extern __shared__ __attribute__((aligned(16))) char xs[];      // the activation row: K * 2 bytes
    mbnb::group_workgroup<T, QT, NESTED, KU, true>(a.g, a.rows, lut, xs);
}

// ---------------------------------------------------------------- host side
template <typename T, int QT, bool NESTED>
int launch(const DownArgs &d, const LoraArgs &a, hipStream_t stream) {
    const int ku = (int)((a.g.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 down((unsigned)d.first_row[d.n]), grid((unsigned)a.g.first_block[a.g.n]);
    mbnb::with_ku(KU, [&](auto ku_) {
        constexpr int KU_ = decltype(ku_)::value;
        hipLaunchKernelGGL((k_lora_down<T, KU_>), down, dim3(256), 0, stream, d);
        hipLaunchKernelGGL((k_gemv4_group_lora<T, QT, NESTED, KU_>), grid, dim3(256), (size_t)KU_ * 4096, stream, a);
    });
    const int rc = mbnb::launch_status("mbnb_lora_gemv4");
    if (rc == 0)
        snprintf(last_launch(), kLaunchBytes, "lora_down G%d R%d ku%d/KU%d + gemv_lora G%d ku%d/KU%d", d.n, d.first_row[d.n], ku, KU, a.g.n, ku,
                 KU);
    return rc;
}

}  // namespace

extern "C" {

int mbnb_lora_abi_version(void) { return MBNB_LORA_ABI_VERSION; }

const char *mbnb_lora_last_error(void) { return mbnb::last_error(); }

const char *mbnb_lora_last_launch(void) { return last_launch(); }

int mbnb_lora_gemv4(const void *x, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members,
                    const mbnb_lora_adapter *adapters, int n, int flags, void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_lora_gemv4";
    // ---- argument errors: mbnb_group_gemv4's, then the adapter table's
    if (const int rc = mbnb::group_argument_errors(who, x, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    if (const int rc = mbnb::adapter_argument_errors(who, adapters, n)) return rc;
    // ---- the conditions of the fused launches: mbnb_group_gemv4's, then the adapters' (both in gemv4_group.h: the one place these live)
    LoraArgs a;
    bool nested;
    if (const int rc = mbnb::group_conditions(who, MBNB_LORA_NOT_APPLICABLE, x, K, dtype, blocksize, members, n, a.g, nested)) return rc;
    DownArgs d;
    d.x = x;
    d.K = K;
    d.n = n;
    if (const int rc = mbnb::adapter_conditions(who, MBNB_LORA_NOT_APPLICABLE, "mbnb_group_gemv4", adapters, n, d, a.rows)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return MBNB_GROUP_FORMS(dtype, quant_type, nested, launch, d, a, s);
}

}  // extern "C"
