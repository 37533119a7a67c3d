// Macro-tile W8A16 decode GEMM for gfx950:
//   Y[M,N] = X[M,K] · (scale ⊙ Q)[N,K]^T,  X bf16, Q fp8 e4m3fn, fp32 acc,
//   M <= 256.
//
// The streaming fp8 kernel (gemm_w8.hip) is right for M <= 16 and loses at
// the batch sizes a gateway runs at (profiles/r04_fp8_weights.md): every
// 64-column stripe re-reads all of X, and every wave of a workgroup owns M
// rows, so each wave converts the same fp8 fragments again. This is the
// register-staged macro-tile pipeline of gemm_macro.h with an fp8 W policy:
//
// - Q is the fragment-major fp8 twin [K/64, N/16, 64, 16]
//   (ops.swizzle_weight_frag_fp8): one k64 tile of the stripe is NF
//   contiguous 1-KiB units (one n-fragment, both k32 halves), one 16-B load
//   per lane each. The LOADING wave converts its 16 bytes once (cvt_pk +
//   exact truncation, w8_cvt4) into two bf16x8 — bytes 0-7 are k32 half 0,
//   bytes 8-15 half 1. The fp8 twin's lane order equals the bf16 fragment
//   twin's, so the LDS image and everything after it are the bf16
//   kernel's. Conversion happens once per workgroup instead of once per
//   wave.
// - The per-output-channel scale multiplies the fp32 accumulator in the
//   epilogue, before the bf16 store or the slab store, as in gemm_w8.hip,
//   so launch_splitk_tail consumes the slabs as they are.

#include "gemm_macro.h"
#include "w8_cvt.h"

typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t u32x4;

template <int NF_>
struct WFp8Frag {
    static constexpr int NF = NF_;
    static constexpr int UNITS = NF_;  // unit = n-fragment
    static constexpr bool SCALED = true;
    static constexpr bool SWIGLU = false;
    typedef u32x4 Regs;

    const uint8_t* src;
    size_t step;  // one k64 plane

    __device__ __forceinline__ void init(const void* q, const void*, int N,
                                         int n0, int lane) {
        src = (const uint8_t*)q + ((size_t)(n0 / 16) * 64 + lane) * 16;
        step = (size_t)(N / 16) * 1024;
    }
    __device__ __forceinline__ void load(Regs& r, int unit, int kt) const {
        r = *(const GM_GLOBAL u32x4*)(src + (size_t)kt * step + unit * 1024);
    }
    // words 2h, 2h+1 of a lane's 16 fp8 bytes -> its bf16 B fragment of k32
    // half h
    static __device__ __forceinline__ void write(GM_LDS char* wa, int unit,
                                                 int lane, const Regs& q) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            union { uint32_t u[4]; bf16x8 v; } c;
            w8_cvt4(q[2 * h], c.u[0], c.u[1]);
            w8_cvt4(q[2 * h + 1], c.u[2], c.u[3]);
            *(GM_LDS bf16x8*)(wa + (h * NF + unit) * 1024 + lane * 16) = c.v;
        }
    }
};

extern "C" hipError_t launch_gemm_w8_m256(
    void* y, float* workspace, const void* x, const void* q,
    const float* scale, int M, int N, int K, int nsk, int nf, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    return launch_gemm_macro<WFp8Frag>(y, workspace, x, q, scale, M, N, K, nsk,
                                       nf, 0, residual, norm_weight, eps, out,
                                       stream);
}
