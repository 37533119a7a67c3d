// W8A16 skinny-M streaming GEMM for gfx950:
//   Y[M,N] = X[M,K] · (scale ⊙ Q)[N,K]^T,  X bf16, Q fp8 e4m3fn, fp32 acc.
//
// The decode projections are weight-stream-bound; fp8 weights halve the
// bytes each step has to stream. The kernel is the shared streaming
// pipeline (gemm_stream.h) in k64 steps; this file supplies its fp8
// B-operand policy:
//
// - Q is fragment-major [K/64, N/16, 64, 16] (ops.swizzle_weight_frag_fp8):
//   lane l's 16 bytes are its B-fragments for TWO consecutive 32-deep
//   k-steps (bytes 0-7 then 8-15), so one k64 step of a stripe is four
//   contiguous 1 KiB rows, one 16-byte load per lane each.
// - dequantisation happens in registers: cvt_pk e4m3 -> f32, keep the high
//   16 bits. e4m3 has 3 mantissa bits, so the truncation is exact and the
//   bf16 MFMA sees exactly the fp8 values.
// - the per-output-channel scale multiplies the fp32 accumulator in the
//   epilogue, BEFORE the bf16 store or the slab store, so the shared
//   split-K tail consumes the slabs as they are.
//
// dequant_w8_kernel expands the fp8 twin to a row-major bf16 [N,K] buffer
// for M > 256 (prefill), which then runs on the library GEMM.

#include "gemm_launch.h"
#include "gemm_stream.h"
#include "w8_cvt.h"

struct BFp8Frag {
    static constexpr int KSTEP = 64;
    static constexpr bool SCALED = true;
    struct Regs { u32x4 v[GS_NF]; };
    const uint8_t* p;
    size_t step;
    // the stripe's four fragment rows are adjacent: 1 KiB apart; one k64
    // step further is a whole [N/16, 64, 16] plane = 64*N bytes
    __device__ __forceinline__ void init(const void* q, const void*, int N, int K,
                                         int n0, int k0, int lane) {
        step = (size_t)64 * N;
        p = (const uint8_t*)q + (size_t)(k0 / 64) * step +
            ((size_t)(n0 / 16) * 64 + lane) * 16;
    }
    __device__ __forceinline__ void load(Regs& r, int S) const {
#pragma unroll
        for (int n = 0; n < GS_NF; ++n)
            r.v[n] = gs_gload<u32x4>(p + S * step + n * 1024);
    }
    __device__ __forceinline__ void bump(int steps) { p += steps * step; }
    // words 2h, 2h+1 hold the 8 e4m3 bytes of k32 half h
    static __device__ __forceinline__ bf16x8 frag(const Regs& r, int n, int h) {
        union { uint32_t u[4]; bf16x8 v; } c;
        w8_cvt4(r.v[n][2 * h], c.u[0], c.u[1]);
        w8_cvt4(r.v[n][2 * h + 1], c.u[2], c.u[3]);
        return c.v;
    }
};

// fragment-major fp8 twin + scale -> row-major bf16 [N, K]. One thread per
// 16-byte fragment entry: it owns 8 consecutive k of row n for each of the
// two 32-deep k-steps of its k64 block. Rounding is RNE; with a
// power-of-two scale the product is exact in bf16.
__global__ void dequant_w8_kernel(
    bf16* __restrict__ out,          // [N, K]
    const uint8_t* __restrict__ q,   // [K/64, N/16, 64, 16]
    const float* __restrict__ scale, // [N]
    int N, int K) {
    const int64_t total = (int64_t)(K / 64) * (N / 16) * 64;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    const int64_t frag = t >> 6;
    const int n16 = (int)(frag % (N / 16));
    const int k64 = (int)(frag / (N / 16));
    const int n = n16 * 16 + (lane & 15);
    const int kb = k64 * 64 + (lane >> 4) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(q + t * 16);
    const float s = scale[n];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float f[8];
        fp8x4_to_f32(w[2 * h], f[0], f[1], f[2], f[3]);
        fp8x4_to_f32(w[2 * h + 1], f[4], f[5], f[6], f[7]);
        uint4 o;
        o.x = pack2(f[0] * s, f[1] * s);
        o.y = pack2(f[2] * s, f[3] * s);
        o.z = pack2(f[4] * s, f[5] * s);
        o.w = pack2(f[6] * s, f[7] * s);
        *reinterpret_cast<uint4*>(out + (size_t)n * K + kb + h * 32) = o;
    }
}

extern "C" hipError_t launch_dequant_w8(
    void* out, const void* q, const float* scale, int N, int K,
    hipStream_t stream) {
    if (N <= 0 || K <= 0 || (N % GS_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    const int64_t total = (int64_t)(K / 64) * (N / 16) * 64;
    const int tpb = 256;
    dequant_w8_kernel<<<dim3((unsigned)((total + tpb - 1) / tpb)), dim3(tpb), 0,
                        stream>>>((bf16*)out, (const uint8_t*)q, scale, N, K);
    HIP_CHECK_LAST();
    return hipSuccess;
}

// With residual/norm_weight/out set (split-K only) the slab reduction also
// adds the residual and RMS-normalizes (launch_gemm_reduce_rmsnorm) and y
// is not written.
extern "C" hipError_t launch_gemm_w8(
    void* y, float* workspace, const void* x, const void* q,
    const float* scale, int M, int N, int K, int nsk, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > GS_MAX_M) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % GS_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    if (nsk < 1 || nsk > K / 64) return hipErrorInvalidValue;
    if (nsk > 1 && workspace == nullptr) return hipErrorInvalidValue;
    if (out != nullptr && (nsk < 2 || residual == nullptr || norm_weight == nullptr))
        return hipErrorInvalidValue;
    const hipError_t err = launch_gemm_stream<BFp8Frag>(
        y, workspace, x, q, scale, M, N, K, nsk, stream);
    if (err != hipSuccess) return err;
    return launch_splitk_tail(y, workspace, M, N, nsk, residual, norm_weight,
                              eps, out, stream);
}
