// Host-side entry points of the decode GEMM family, declared once for the
// .hip files that define or chain them and for ext.cpp. Plain C linkage,
// raw pointers; every launcher is hipGraph-capturable.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

extern "C" {
// gemm_skinny.hip
hipError_t launch_gemm_skinny(void* y, float* workspace, const void* x,
                              const void* w, int M, int N, int K, int nsk,
                              int swz, hipStream_t stream);
hipError_t launch_gemm_reduce(void* y, const float* yw, int64_t mn, int nsk,
                              hipStream_t stream);
int gemm_reduce_rmsnorm_covers(int N);
hipError_t launch_gemm_reduce_rmsnorm(void* out, void* residual,
                                      const float* yw, const void* weight,
                                      float eps, int M, int N, int nsk,
                                      hipStream_t stream);
// What follows a split-K GEMM kernel: nothing at nsk == 1, the plain slab
// reduction into y, or — with out set — the fused reduce + residual add +
// RMSNorm (residual updated in place, y not written).
hipError_t launch_splitk_tail(void* y, const float* workspace, int M, int N,
                              int nsk, void* residual, const void* norm_weight,
                              float eps, void* out, hipStream_t stream);
// gemm_m256.hip
hipError_t launch_gemm_m256(void* y, float* workspace, const void* x,
                            const void* w, int M, int N, int K, int nsk, int nf,
                            int variant, int pipe, int swiglu, void* residual,
                            const void* norm_weight, float eps, void* norm_out,
                            hipStream_t stream);
// gemm_w8.hip
hipError_t launch_gemm_w8(void* y, float* workspace, const void* x,
                          const void* q, const float* scale, int M, int N,
                          int K, int nsk, void* residual,
                          const void* norm_weight, float eps, void* out,
                          hipStream_t stream);
hipError_t launch_dequant_w8(void* out, const void* q, const float* scale,
                             int N, int K, hipStream_t stream);
// gemm_w4.hip
hipError_t launch_gemm_w4(void* y, float* workspace, const void* x,
                          const void* q, const void* scale, int M, int N,
                          int K, int nsk, void* residual,
                          const void* norm_weight, float eps, void* out,
                          hipStream_t stream);
hipError_t launch_dequant_w4(void* out, const void* q, const void* scale,
                             int N, int K, hipStream_t stream);
// gemm_w8_m256.hip
hipError_t launch_gemm_w8_m256(void* y, float* workspace, const void* x,
                               const void* q, const float* scale, int M, int N,
                               int K, int nsk, int nf, void* residual,
                               const void* norm_weight, float eps, void* out,
                               hipStream_t stream);
// gemm_w4_m256.hip
hipError_t launch_gemm_w4_m256(void* y, float* workspace, const void* x,
                               const void* q, const void* scale, int M, int N,
                               int K, int nsk, int nf, void* residual,
                               const void* norm_weight, float eps, void* out,
                               hipStream_t stream);
}
