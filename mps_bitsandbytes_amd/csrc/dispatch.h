// dispatch.h — the library's internal entry points that one translation unit defines and another calls: the per-operation
// dispatchers behind the C ABI (api.hip), the per-path launchers of the GEMM families and their shape / workspace queries.
// Declarations only, each in one place with its default arguments; every .hip file includes this header.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mbnb {

struct AbsmaxView;
struct OutlierEpilogue;
template <typename T, bool NESTED> struct Q4ProducerRT;

// quant_kernels.hip
int quantize_4bit_dispatch(const void *, int, int64_t, int64_t, int64_t, int, int, const float *, uint8_t *, float *, hipStream_t);
int quantize_4bit_dq_dispatch(const void *, int, int64_t, int64_t, int64_t, int, int, uint8_t *, int8_t *, float *, hipStream_t);
int dequantize_4bit_dispatch(const uint8_t *, const AbsmaxView &, int64_t, int64_t, int64_t, int, int, int, void *, hipStream_t, int store_policy = 0);
int quantize_blockwise_dispatch(const void *, int, int64_t, int, const float *, int8_t *, float *, hipStream_t);
int dequantize_blockwise_dispatch(const int8_t *, int64_t, const float *, int, int, void *, hipStream_t);
int dequant_absmax_dispatch(const void *, int, int64_t, int64_t, const float *, int64_t, int, float *, hipStream_t);
int quantize_rowwise_dispatch(const void *, int, int64_t, int64_t, int8_t *, float *, hipStream_t);
int dequantize_rowwise_dispatch(const int8_t *, const float *, int64_t, int64_t, int, void *, hipStream_t, int store_policy = 0);
int double_quant_dispatch(const void *, int, int64_t, int64_t, int8_t *, int8_t *, float *, float *, int, int, hipStream_t);
int quantize_fp8_dispatch(const void *, int, int64_t, int64_t, uint8_t *, float *, hipStream_t);
int dequantize_fp8_dispatch(const uint8_t *, const float *, int64_t, int64_t, int, void *, hipStream_t, int store_policy = 0);

// matmul4_kernels.hip
int matmul_4bit_dispatch(const void *, int64_t, int64_t, const uint8_t *, const AbsmaxView &, int64_t, int64_t, int, int, int, const void *, int, void *, void *, int64_t, int,
                         hipStream_t);
int64_t matmul4_splitk_slices(int64_t M, int64_t N, int64_t K);

// gemm_mid.hip
bool gemm_mid_shape(int64_t M, int64_t N, int64_t K);
int64_t gemm_mid_workspace_bytes(int64_t, int64_t, int64_t);
template <typename T, typename OutT, bool NESTED>
int launch_gemm_mid(const T *x, const typename Q4ProducerRT<T, NESTED>::Params &wp, const T *bias, OutT *out, int64_t M,
                    int64_t N, int64_t K, float *ws, int64_t ws_bytes, int force_slices, hipStream_t st);

// gemm_small.hip
bool gemm_small_shape(int64_t M, int64_t N, int64_t K, int64_t K_weight);
bool gemm_small_one_round(int64_t M, int64_t N, int64_t K, int64_t K_weight, int64_t ws_bytes);
int64_t gemm_small_workspace_bytes(int64_t, int64_t, int64_t, int64_t);
bool gemm_small8_shape(int64_t M, int64_t N, int64_t K);
int64_t gemm_small8_slices(int64_t M, int64_t N, int64_t K);
int64_t gemm_small8_workspace_bytes(int64_t, int64_t, int64_t);
template <typename T, typename OutT, bool NESTED>
int launch_gemm_small(const T *, const uint8_t *, const AbsmaxView &, const T *, OutT *, int64_t, int64_t, int64_t, int64_t, int, int, float *,
                      int64_t, hipStream_t);

// gemm_small8.hip
template <typename T, int WF>
int launch_gemm_small8(const T *, const uint8_t *, const float *, const T *, T *, int64_t, int64_t, int64_t, float *, int64_t, hipStream_t);

// gemm_fused4.hip
int matmul_4bit_fused4_path(const void *, int64_t, int64_t, const uint8_t *, const AbsmaxView &, int64_t, int64_t, int, int, int, const void *, int, void *,
                            hipStream_t);

// gemm_f32.hip
int matmul_4bit_f32_path(const void *, int64_t, int64_t, const uint8_t *, const AbsmaxView &, int64_t, int64_t, int, int, const void *, int, void *, void *, int64_t, hipStream_t);
int64_t gemm_f32_workspace_bytes(int64_t, int64_t, int64_t, int64_t);

// gemm_dense.hip
int matmul_4bit_dense_path(const void *, int64_t, int64_t, const uint8_t *, const AbsmaxView &, int64_t, int64_t, int, int, int, const void *,
                           int, void *, void *, int64_t, hipStream_t);
int linear8_dense_path(const void *, int, int64_t, int64_t, const void *, const float *, int64_t, bool, const void *, void *, void *, int64_t,
                       hipStream_t);
int64_t gemm_dense_workspace_bytes(int64_t, int64_t, int64_t, int64_t);
bool gemm_dense_shape(int64_t, int64_t, int64_t, int64_t);
int64_t gemm_dense_slices(int64_t, int64_t, int64_t);
int64_t gemm_dense_wd_bytes(int64_t, int64_t);
int gemm_dense_direct(const void *, const void *, int, const void *, int, void *, int64_t, int64_t, int64_t, int64_t, float *, int64_t, int, int,
                      hipStream_t);
// the four-wave pipeline on int8 operands (ep: OutlierAwareLinear's second term and bias in its epilogue)
bool gemm_i8_dense_shape(int64_t M, int64_t N, int64_t K);
bool gemm_i8_dense_outlier_ok(const OutlierEpilogue &ep, int out_dtype);
int launch_gemm_i8_dense(const int8_t *, const int8_t *, const float *, const float *, int64_t, int64_t, int64_t, int, void *, hipStream_t,
                         const OutlierEpilogue *ep = nullptr);

// gemm_i8_inplace.hip
bool gemm_i8_inplace_shape(const int8_t *, const int8_t *, int64_t, int64_t, int64_t);
int launch_gemm_i8_inplace(const int8_t *, const int8_t *, const float *, const float *, int64_t, int64_t, int64_t, int, void *, hipStream_t);

// int8_kernels.hip
int matmul_int8_dispatch(const int8_t *, const int8_t *, const float *, const float *, int64_t, int64_t, int64_t, int, void *, void *, hipStream_t);
int64_t matmul_int8_workspace_bytes(int64_t, int64_t, int64_t);
// `ep` (may be nullptr): outlier / bias epilogue.  It is applied only by the 256 x 256 kernels with a 16-bit output;
// *ep_done tells the caller whether it was (otherwise the caller runs k_outlier_add afterwards).
int matmul_int8_nt_dispatch(const int8_t *A, const int8_t *Bt, const float *sA, const float *sB, int64_t M, int64_t N,
                            int64_t K, int out_dtype, void *out, hipStream_t st, const OutlierEpilogue *ep = nullptr,
                            bool *ep_done = nullptr);
int linear_int8_dispatch(const void *, int, int64_t, int64_t, const int8_t *, const float *, int64_t, const void *, void *, void *, int64_t, bool, hipStream_t);
int linear_fp8_dispatch(const void *, int, int64_t, int64_t, const uint8_t *, const float *, int64_t, const void *, void *, void *, int64_t, bool, hipStream_t);

// nn_kernels.hip
int embedding_4bit_dispatch(const int64_t *, int64_t, const uint8_t *, const float *, int64_t, int64_t, int, int, int, int64_t, int, void *, hipStream_t);
int embedding_8bit_dispatch(const int64_t *, int64_t, const int8_t *, const float *, int64_t, int64_t, int, int64_t, int, void *, hipStream_t);
int outlier_linear_dispatch(const void *, int, int64_t, int64_t, const int8_t *, const float *, int64_t, const int64_t *, int64_t, const void *, const void *, void *, void *, int64_t, hipStream_t);
int64_t outlier_linear_workspace_bytes(int64_t, int64_t, int64_t);

// grad_kernels.hip
int64_t grad_input_workspace_bytes(int64_t, int64_t, int64_t, int, int);
int linear_grad_input_dispatch(const void *, int64_t, int64_t, int, const void *, const AbsmaxView &, const float *, int64_t, int64_t, int, int, int,
                               void *, void *, int64_t, bool, hipStream_t);

}  // namespace mbnb
