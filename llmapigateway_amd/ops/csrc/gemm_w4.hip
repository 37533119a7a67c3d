// W4A16 skinny-M streaming GEMM for gfx950:
//   Y[M,N] = X[M,K] · dequant(Q, S)[N,K]^T,  X bf16, fp32 accumulation,
//   Q OCP MXFP4: e2m1 elements, one e8m0 power-of-two scale per 32
//   consecutive k of a row (4.25 bits per weight).
//
// The decode projections are weight-stream-bound; MXFP4 streams a quarter
// of the bf16 bytes. The kernel is the shared streaming pipeline
// (gemm_stream.h) in k64 steps; this file supplies its MXFP4 B-operand
// policy:
//
// - Q is fragment-major [K/64, N/16, 64, 8] bytes
//   (ops.swizzle_weight_frag_mxfp4): lane l's 8 bytes are its B-fragments
//   for TWO consecutive 32-deep k-steps (bytes 0-3 then 4-7, two nibbles per
//   byte, even k low), so one k64 step of a stripe is four contiguous 512 B
//   rows, one 8-byte load per lane each.
// - one k32 MFMA step is exactly one MX block, so a lane needs one scale per
//   n-fragment and k32 half: S is fragment-major [K/64, N/64, 16, 8] bytes,
//   [..][lane & 15][n * 2 + h], one 8-byte load per lane and step (the four
//   k-groups of a column read the same 8 bytes).
// - dequantisation happens in registers (w4_cvt.h): the hardware conversion
//   applies the block scale, so the bf16 MFMA sees exactly the dequantised
//   weights and the accumulator needs no scale in the epilogue.
//
// dequant_w4_kernel expands the twin to a row-major bf16 [N,K] buffer for
// M > 256 (prefill), which then runs on the library GEMM.

#include "gemm_launch.h"
#include "gemm_stream.h"
#include "w4_cvt.h"

typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t u32x2;

struct BMxfp4Frag {
    static constexpr int KSTEP = 64;
    static constexpr bool SCALED = false;
    struct Regs {
        u32x2 v[GS_NF];  // word h of v[n]: the 8 nibbles of k32 half h
        u32x2 s;         // byte n*2 + h: the e8m0 scale of that fragment
    };
    const uint8_t* p;
    const uint8_t* ps;
    size_t step, sstep;
    // the stripe's four fragment rows are adjacent, 512 B apart; one k64
    // step further is a whole [N/16, 64, 8] plane = 32*N bytes of nibbles
    // and a [N/64, 16, 8] plane = 2*N bytes of scales
    __device__ __forceinline__ void init(const void* q, const void* s, int N,
                                         int K, int n0, int k0, int lane) {
        step = (size_t)32 * N;
        sstep = (size_t)2 * N;
        p = (const uint8_t*)q + (size_t)(k0 / 64) * step +
            ((size_t)(n0 / 16) * 64 + lane) * 8;
        ps = (const uint8_t*)s + (size_t)(k0 / 64) * sstep +
             ((size_t)(n0 / 64) * 16 + (lane & 15)) * 8;
    }
    __device__ __forceinline__ void load(Regs& r, int S) const {
#pragma unroll
        for (int n = 0; n < GS_NF; ++n)
            r.v[n] = gs_gload<u32x2>(p + S * step + n * 512);
        r.s = gs_gload<u32x2>(ps + S * sstep);
    }
    __device__ __forceinline__ void bump(int steps) {
        p += steps * step;
        ps += steps * sstep;
    }
    static __device__ __forceinline__ bf16x8 frag(const Regs& r, int n, int h) {
        union { uint32_t u[4]; bf16x8 v; } c;
        const uint32_t byte = (r.s[n >> 1] >> (((n & 1) * 2 + h) * 8)) & 0xFFu;
        w4_cvt8(r.v[n][h], w4_scale(byte), c.u);
        return c.v;
    }
};

// fragment-major MXFP4 twin -> row-major bf16 [N, K]. One thread per 8-byte
// fragment entry: it owns 8 consecutive k of row n for each of the two
// 32-deep k-steps of its k64 block. Exact (see w4_cvt.h).
__global__ void dequant_w4_kernel(
    bf16* __restrict__ out,         // [N, K]
    const uint8_t* __restrict__ q,  // [K/64, N/16, 64, 8]
    const uint8_t* __restrict__ s,  // [K/64, N/64, 16, 8]
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
    const uint2 v = *reinterpret_cast<const uint2*>(q + t * 8);
    const uint8_t* sp = s + (size_t)k64 * 2 * N +
                        ((size_t)(n16 / 4) * 16 + (lane & 15)) * 8 + (n16 & 3) * 2;
    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t o[4];
        w4_cvt8(w[h], w4_scale(sp[h]), o);
        *reinterpret_cast<uint4*>(out + (size_t)n * K + kb + h * 32) =
            make_uint4(o[0], o[1], o[2], o[3]);
    }
}

extern "C" hipError_t launch_dequant_w4(
    void* out, const void* q, const void* scale, int N, int K,
    hipStream_t stream) {
    if (N <= 0 || K <= 0 || (N % GS_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    const int64_t total = (int64_t)(K / 64) * (N / 16) * 64;
    const int tpb = 256;
    dequant_w4_kernel<<<dim3((unsigned)((total + tpb - 1) / tpb)), dim3(tpb), 0,
                        stream>>>((bf16*)out, (const uint8_t*)q,
                                  (const uint8_t*)scale, N, K);
    HIP_CHECK_LAST();
    return hipSuccess;
}

// With residual/norm_weight/out set (split-K only) the slab reduction also
// adds the residual and RMS-normalizes (launch_gemm_reduce_rmsnorm) and y
// is not written.
extern "C" hipError_t launch_gemm_w4(
    void* y, float* workspace, const void* x, const void* q,
    const void* scale, int M, int N, int K, int nsk, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > GS_MAX_M) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % GS_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    if (nsk < 1 || nsk > K / 64) return hipErrorInvalidValue;
    if (nsk > 1 && workspace == nullptr) return hipErrorInvalidValue;
    if (out != nullptr && (nsk < 2 || residual == nullptr || norm_weight == nullptr))
        return hipErrorInvalidValue;
    const hipError_t err = launch_gemm_stream<BMxfp4Frag>(
        y, workspace, x, q, scale, M, N, K, nsk, stream);
    if (err != hipSuccess) return err;
    return launch_splitk_tail(y, workspace, M, N, nsk, residual, norm_weight,
                              eps, out, stream);
}
