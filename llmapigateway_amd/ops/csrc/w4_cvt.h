// MXFP4 (OCP e2m1 elements, e8m0 block scale) -> bf16 in registers, shared
// by the W4A16 decode GEMM and its dequantise kernel (gemm_w4.hip).
#pragma once

#include "common.h"

typedef __attribute__((__vector_size__(2 * sizeof(__bf16)))) __bf16 w4_bf16x2;

// e8m0 scale byte (exponent + 127, in [1, 254]) -> the f32 2^(byte - 127):
// the byte IS the f32 exponent field.
__device__ __forceinline__ float w4_scale(uint32_t byte) {
    union { uint32_t u; float f; } c;
    c.u = byte << 23;
    return c.f;
}

// 8 e2m1 nibbles (one word: k ascending from the low nibble of byte 0) times
// a power-of-two scale -> 8 bf16 in 4 packed words, k ascending. One
// v_cvt_scalef32_pk_bf16_fp4 per byte: it converts the byte's two nibbles
// (low nibble -> low half) and applies the scale. e2m1 has one mantissa bit
// and the scale only shifts the exponent, so the result is exact.
__device__ __forceinline__ void w4_cvt8(uint32_t q, float scale, uint32_t* w) {
    union { w4_bf16x2 v; uint32_t u; } c;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
    w[0] = c.u;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
    w[1] = c.u;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
    w[2] = c.u;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
    w[3] = c.u;
}
