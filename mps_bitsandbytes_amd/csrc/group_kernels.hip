// group_kernels.hip — the grouped M = 1 decode GEMV and the C ABI of libmbnb_group.so (include/mbnb_group.h).
//
// k_gemv4_lean (gemv4_lean.h) spends about 2 of its 5 us per 4096^2 layer on what does not depend on the weight: the launch, staging
// the activation row into LDS, the code table, the barrier.  A decoder block hands the same row to q / k / v and
// again to gate / up; k_gemv4_group serves the rows of all those weights from ONE launch.  A workgroup still owns four rows of one
// weight and runs the arithmetic of k_gemv4_lean on them (group_row, gemv4_group.h), so each output equals mbnb_matmul_4bit's bit for bit; what
// is new is the member table in the kernel arguments and the search that tells a workgroup whose rows it has.
#include "../../include/mbnb_group.h"
#include "host.h"
#include "gemv4_group.h"

static_assert(MBNB_GROUP_F16 == mbnb::kF16 && MBNB_GROUP_BF16 == mbnb::kBF16 && MBNB_GROUP_F32 == mbnb::kF32, "dtype codes");
static_assert(MBNB_GROUP_F16 == MBNB_F16 && MBNB_GROUP_BF16 == MBNB_BF16 && MBNB_GROUP_F32 == MBNB_F32, "dtype codes of mbnb_hip.h");
static_assert(MBNB_GROUP_NF4 == MBNB_NF4 && MBNB_GROUP_FP4 == MBNB_FP4, "code tables of mbnb_hip.h");

namespace {

using mbnb::GroupArgs;
using mbnb::kLaunchBytes;
using mbnb::last_launch;

// the member table, the workgroup body and the row body (a marked copy of k_gemv4_lean's) are in gemv4_group.h, shared with
// k_gemv4_group_lora of libmbnb_lora.so; LORA = false here
template <typename T, int QT, bool NESTED, int KU>
__global__ __launch_bounds__(256) void k_gemv4_group(const GroupArgs a) {
    __shared__ float lut[16];
    extern __shared__ __attribute__((aligned(16))) char xs[];      // the activation row: K * 2 bytes
    mbnb::group_workgroup<T, QT, NESTED, KU, false>(a, nullptr, lut, xs);
}

// ---------------------------------------------------------------- host side
template <typename T, int QT, bool NESTED>
int launch(const GroupArgs &a, hipStream_t stream) {
    const int ku = (int)((a.K + 2047) / 2048);
    const int KU = mbnb::group_ku_form(ku);
    const dim3 grid((unsigned)a.first_block[a.n]);
    mbnb::with_ku(KU, [&](auto ku_) {
        constexpr int KU_ = decltype(ku_)::value;
        hipLaunchKernelGGL((k_gemv4_group<T, QT, NESTED, KU_>), grid, dim3(256), (size_t)KU_ * 4096, stream, a);
    });
    const int rc = mbnb::launch_status("mbnb_group_gemv4");
    if (rc == 0) snprintf(last_launch(), kLaunchBytes, "gemv_group G%d ku%d/KU%d", a.n, ku, KU);
    return rc;
}

}  // namespace

extern "C" {

int mbnb_group_abi_version(void) { return MBNB_GROUP_ABI_VERSION; }

const char *mbnb_group_last_error(void) { return mbnb::last_error(); }

const char *mbnb_group_last_launch(void) { return last_launch(); }

int mbnb_group_gemv4(const void *x, int64_t K, int quant_type, int dtype, int blocksize, const mbnb_group_member *members, int n,
                     int flags, void *stream) {
    if (n == 0) return 0;
    static const char who[] = "mbnb_group_gemv4";
    if (const int rc = mbnb::group_argument_errors(who, x, K, quant_type, dtype, blocksize, members, n, flags)) return rc;
    // the conditions of the fused launch (gemv4_group.h: the one place they live)
    GroupArgs a;
    bool nested;
    if (const int rc = mbnb::group_conditions(who, MBNB_GROUP_NOT_APPLICABLE, x, K, dtype, blocksize, members, n, a, nested)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return MBNB_GROUP_FORMS(dtype, quant_type, nested, launch, a, s);
}

}  // extern "C"
