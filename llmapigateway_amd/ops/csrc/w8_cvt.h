// fp8 (e4m3) -> bf16 in registers, shared by the W8A16 decode GEMMs
// (gemm_w8.hip streams the result straight into the MFMA, gemm_w8_m256.hip
// stages it into LDS).
#pragma once

#include "common.h"

// 4 e4m3 bytes -> 4 bf16 (2 packed words). The f32 image of an e4m3 value
// has at most 3 mantissa bits, so its high half IS the bf16 value.
__device__ __forceinline__ void w8_cvt4(uint32_t q, uint32_t& w0, uint32_t& w1) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(q, false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(q, true);
    w0 = pack2_trunc(lo[0], lo[1]);
    w1 = pack2_trunc(hi[0], hi[1]);
}
