// Macro-tile W4A16 decode GEMM for gfx950:
//   Y[M,N] = X[M,K] · dequant(Q, S)[N,K]^T,  X bf16, fp32 accumulation,
//   Q OCP MXFP4 (e2m1 elements, one e8m0 scale per 32 k of a row), M <= 256.
//
// The streaming MXFP4 kernel (gemm_w4.hip) is right for M <= 16 and grows
// linearly with M (profiles/r07_mxfp4_weights.md): every 64-column stripe
// re-reads all of X, and every wave of a workgroup converts the same weight
// fragments again. This is the register-staged macro-tile pipeline of
// gemm_macro.h with an MXFP4 W policy:
//
// - Q and S are the fragment-major MXFP4 twin, unchanged
//   (ops.swizzle_weight_frag_mxfp4): nibbles [K/64, N/16, 64, 8], scales
//   [K/64, N/64, 16, 8]. One k64 tile of the stripe is NF contiguous 512-B
//   nibble units (one n-fragment, both k32 halves), one 8-byte load per
//   lane each. With it the lane takes the 8 scale bytes of its column:
//   group (n0/16 + n)/4, row lane & 15, byte (n & 3)*2 + h. The LOADING
//   wave converts each k32 half once (w4_cvt8: the hardware conversion
//   applies the block scale, exactly) into the bf16 fragment image the fp8
//   and bf16 policies produce, so everything after it is the bf16 kernel's.
// - The accumulator needs no scale in the epilogue, unlike fp8.

#include "gemm_macro.h"
#include "w4_cvt.h"

typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t u32x2;

template <int NF_>
struct WMxfp4Frag {
    static constexpr int NF = NF_;
    static constexpr int UNITS = NF_;  // unit = n-fragment
    static constexpr bool SCALED = false;
    static constexpr bool SWIGLU = false;
    struct Regs {
        u32x2 q, s;
    };

    const uint8_t* src;   // nibbles
    const uint8_t* ssrc;  // scales
    size_t step, sstep;   // one k64 plane of each

    // n0 is a multiple of 64, so fragment n of the stripe sits in scale
    // group n0/64 + n/4 at bytes (n & 3)*2 + h
    __device__ __forceinline__ void init(const void* q, const void* s, int N,
                                         int n0, int lane) {
        src = (const uint8_t*)q + ((size_t)(n0 / 16) * 64 + lane) * 8;
        ssrc = (const uint8_t*)s + ((size_t)(n0 / 64) * 16 + (lane & 15)) * 8;
        step = (size_t)N * 32;
        sstep = (size_t)N * 2;
    }
    __device__ __forceinline__ void load(Regs& r, int unit, int kt) const {
        r.q = *(const GM_GLOBAL u32x2*)(src + (size_t)kt * step + unit * 512);
        r.s = *(const GM_GLOBAL u32x2*)(ssrc + (size_t)kt * sstep +
                                        (unit >> 2) * 128);
    }
    // word h of a lane's 8 nibble bytes and byte (unit & 3)*2 + h of its
    // column's 8 scales -> its bf16 B fragment of k32 half h
    static __device__ __forceinline__ void write(GM_LDS char* wa, int unit,
                                                 int lane, const Regs& r) {
        const uint64_t s64 = ((uint64_t)r.s[1] << 32) | r.s[0];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            union { uint32_t u[4]; bf16x8 v; } c;
            const uint32_t byte =
                (uint32_t)(s64 >> (((unit & 3) * 2 + h) * 8)) & 0xFFu;
            w4_cvt8(r.q[h], w4_scale(byte), c.u);
            *(GM_LDS bf16x8*)(wa + (h * NF + unit) * 1024 + lane * 16) = c.v;
        }
    }
};

extern "C" hipError_t launch_gemm_w4_m256(
    void* y, float* workspace, const void* x, const void* q, const void* s,
    int M, int N, int K, int nsk, int nf, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    return launch_gemm_macro<WMxfp4Frag>(y, workspace, x, q, s, M, N, K, nsk,
                                         nf, 0, residual, norm_weight, eps, out,
                                         stream);
}
