// Macro-tile W4A16 decode GEMM for gfx950:
//   Y[M,N] = X[M,K] · dequant(Q, S)[N,K]^T,  X bf16, fp32 accumulation,
//   Q OCP MXFP4 (e2m1 elements, one e8m0 scale per 32 k of a row), M <= 256.
//
// The streaming MXFP4 kernel (gemm_w4.hip) is right for M <= 16 and grows
// linearly with M (profiles/r07_mxfp4_weights.md): every 64-column stripe
// re-reads all of X, and every wave of a workgroup converts the same weight
// fragments again. This kernel is gemm_w8_m256_kernel (gemm_w8_m256.hip)
// with an MXFP4 W stage:
//
// - One workgroup owns ALL M rows of a BN = 16*NF column stripe for its
//   K-slice; wave w owns rows [32w, 32w+32): 2 m-fragments x NF
//   n-fragments of v_mfma_f32_16x16x32_bf16, BK = 64, two LDS buffers, the
//   register-staged loads-two-ahead pipeline.
// - X is staged as there: linear 128-B-line loads, XOR swizzle on the
//   ds_write address, per-unit row clamp for rows >= M.
// - Q and S are the fragment-major MXFP4 twin, unchanged
//   (ops.swizzle_weight_frag_mxfp4): nibbles [K/64, N/16, 64, 8], scales
//   [K/64, N/64, 16, 8]. One k64 tile of the stripe is NF contiguous 512-B
//   nibble units (one n-fragment, both k32 halves), one 8-byte load per
//   lane each, dealt round-robin over the waves. With it the lane takes the
//   8 scale bytes of its column: group (n0/16 + n)/4, row lane & 15, byte
//   (n & 3)*2 + h. The LOADING wave converts each k32 half once (w4_cvt8:
//   the hardware conversion applies the block scale, exactly) and writes
//   the two bf16x8 to (h*NF + n)*1024 + lane*16 of the buffer's W area.
//   That is the fp8 kernel's LDS image, so from the barrier on the k-loop
//   is unchanged: lane-linear ds_read_b128 for B, XOR reads for A, the same
//   MFMAs in the same order.
// - The accumulator needs no scale in the epilogue, unlike fp8.
// - split-K over grid.y writes private fp32 slabs; an empty slice writes
//   zeros.

#include "common.h"
#include "gemm_launch.h"
#include "w4_cvt.h"

#define G4_BK 64  // k-depth of one staged tile (2 MFMA k-steps)

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t u32x2;

__device__ __forceinline__ f32x4 g4_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// compiler-only memory fence around the raw s_barrier (see gemm_m256.hip)
__device__ __forceinline__ void g4_cfence() { asm volatile("" ::: "memory"); }

// word h of a lane's 8 nibble bytes and scale byte `sb` of its column's 8
// -> its bf16 B fragment of k32 half h
__device__ __forceinline__ bf16x8 g4_frag(const u32x2& q, const u32x2& s,
                                          int sb, int h) {
    union { uint32_t u[4]; bf16x8 v; } c;
    const uint64_t s64 = ((uint64_t)s[1] << 32) | s[0];
    const uint32_t byte = (uint32_t)(s64 >> ((sb + h) * 8)) & 0xFFu;
    w4_cvt8(q[h], w4_scale(byte), c.u);
    return c.v;
}

// MW = waves per block (BM = 32*MW rows), NF = 16-col n-fragments (BN =
// 16*NF).
template <int MW, int NF, bool SPLITK>
__launch_bounds__(MW * WAVE_SIZE)
__global__ void gemm_w4_m256_kernel(
    bf16* __restrict__ y,           // [M, N] (!SPLITK)
    float* __restrict__ yw,         // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,     // [M, K]
    const uint8_t* __restrict__ q,  // fragment-major [K/64][N/16][64][8]
    const uint8_t* __restrict__ s,  // fragment-major [K/64][N/64][16][8]
    int M, int N, int K, int nsk) {
    constexpr int BM = MW * 32;
    constexpr int BN = NF * 16;
    constexpr int XB = BM * G4_BK * 2;  // X tile bytes (row stride 128)
    constexpr int WB = G4_BK * BN * 2;  // W tile bytes as bf16 (2*NF frags)
    constexpr int BUFB = XB + WB;
    constexpr int XG_W = 4;                   // 1-KiB x units per wave
    constexpr int WG_W = (NF + MW - 1) / MW;  // 512-B nibble units per wave
    static_assert(NF % MW == 0 || MW > NF, "W unit split uneven across waves");

    __shared__ __attribute__((aligned(16))) char smem[2 * BUFB];

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    // uniform in fact, but not provably so to the compiler: the W-unit
    // guard below must be a scalar branch
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = blockIdx.x * BN;

    const int ktiles = K / G4_BK;
    const int kt_per = SPLITK ? (ktiles + nsk - 1) / nsk : ktiles;
    const int kt0 = SPLITK ? blockIdx.y * kt_per : 0;
    const int ntiles = min(ktiles - kt0, kt_per) > 0 ? min(ktiles - kt0, kt_per) : 0;

    // X staging: unit i = rows [32w+8i, +8); lane -> row base+l/8, chunk
    // l%8. Loads are linear (full 128-B lines); the XOR goes on the
    // ds_write address. Per-unit row clamp for M < BM tails.
    const int xrow = wave * 32 + (lane >> 3);
    const bf16* xsrc[XG_W];
#pragma unroll
    for (int i = 0; i < XG_W; ++i) {
        const int r = xrow + i * 8;
        xsrc[i] = x + (size_t)(r < M ? r : 0) * K + (lane & 7) * 8;
    }
    const int xwoff = (xrow & (BM - 1)) * 128 + (((lane & 7) ^ (xrow & 7)) << 4);

    // W staging: unit (= n-fragment) wave + j*MW; with NF < MW the high
    // waves carry none. n0 is a multiple of 64, so fragment n of the
    // stripe sits in scale group n0/64 + n/4 at bytes (n & 3)*2 + h.
    const uint8_t* wsrc = q + ((size_t)(n0 / 16) * 64 + lane) * 8;
    const uint8_t* ssrc = s + ((size_t)(n0 / 64) * 16 + (lane & 15)) * 8;
    const size_t wstep = (size_t)N * 32;  // one k64 plane of nibbles
    const size_t sstep = (size_t)N * 2;   // one k64 plane of scales

    f32x4 acc[2][NF];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    bf16x8 xr[XG_W];  // one in-flight staging tile
    u32x2 wr[WG_W];
    u32x2 sr[WG_W];

#define G4_LOAD(T)                                                             \
    do {                                                                       \
        const int kt__ = kt0 + (T);                                            \
        _Pragma("unroll") for (int i = 0; i < XG_W; ++i) xr[i] =               \
            *(const __attribute__((address_space(1))) bf16x8*)(                \
                xsrc[i] + (size_t)(kt__)*G4_BK);                               \
        _Pragma("unroll") for (int j = 0; j < WG_W; ++j) {                     \
            if (wave + j * MW < NF) {                                          \
                wr[j] = *(const __attribute__((address_space(1))) u32x2*)(     \
                    wsrc + (size_t)(kt__)*wstep + (wave + j * MW) * 512);      \
                sr[j] = *(const __attribute__((address_space(1))) u32x2*)(     \
                    ssrc + (size_t)(kt__)*sstep +                              \
                    ((wave + j * MW) >> 2) * 128);                             \
            }                                                                  \
        }                                                                      \
    } while (0)
#define G4_WRITE(T)                                                            \
    do {                                                                       \
        char* buf__ = smem + ((T)&1) * BUFB;                                   \
        _Pragma("unroll") for (int i = 0; i < XG_W; ++i)                       \
            *(__attribute__((address_space(3))) bf16x8*)(                      \
                (__attribute__((address_space(3))) char*)buf__ + xwoff +       \
                i * 8 * 128) = xr[i];                                          \
        _Pragma("unroll") for (int j = 0; j < WG_W; ++j) {                     \
            if (wave + j * MW < NF) {                                          \
                _Pragma("unroll") for (int h = 0; h < 2; ++h)                  \
                    *(__attribute__((address_space(3))) bf16x8*)(              \
                        (__attribute__((address_space(3))) char*)buf__ + XB +  \
                        (h * NF + wave + j * MW) * 1024 + lane * 16) =         \
                        g4_frag(wr[j], sr[j], ((wave + j * MW) & 3) * 2, h);   \
            }                                                                  \
        }                                                                      \
    } while (0)

    const int arow0 = wave * 32 + (lane & 15);
    const int alk = lane >> 4;

    if (ntiles > 0) {
        G4_LOAD(0);
        G4_WRITE(0);
        if (ntiles > 1) G4_LOAD(1);  // in flight during compute(0)
        // s_barrier waits for no counter: tile 0's ds_writes must have
        // landed before another wave reads them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        g4_cfence();
        for (int t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) {
                // regs hold tile t+1 (issued last iter): convert + write
                // after the barrier, then immediately re-issue for tile
                // t+2 so the loads overlap compute(t). The ds_reads below
                // queue behind these ds_writes, so the writes have landed
                // by the time the MFMAs, and the barrier after them, run.
                G4_WRITE(t + 1);
                if (t + 2 < ntiles) G4_LOAD(t + 2);
            }
            const char* buf = smem + (t & 1) * BUFB;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 a[2], b[NF];
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int row = arow0 + f * 16;
                    const int chunk = (ks * 4 + alk) ^ (row & 7);
                    a[f] = *(const __attribute__((address_space(3))) bf16x8*)(
                        (const __attribute__((address_space(3))) char*)buf +
                        (row & (BM - 1)) * 128 + chunk * 16);
                }
#pragma unroll
                for (int n = 0; n < NF; ++n)
                    b[n] = *(const __attribute__((address_space(3))) bf16x8*)(
                        (const __attribute__((address_space(3))) char*)buf +
                        XB + (ks * NF + n) * 1024 + lane * 16);
#pragma unroll
                for (int n = 0; n < NF; ++n)
#pragma unroll
                    for (int f = 0; f < 2; ++f)
                        acc[f][n] = g4_mfma(a[f], b[n], acc[f][n]);
            }
            g4_cfence();
            __builtin_amdgcn_s_barrier();
            g4_cfence();
        }
    }
#undef G4_LOAD
#undef G4_WRITE

    // ---- epilogue: C fragment row = 4*(lane>>4) + r, col = lane&15; the
    // conversion applied the block scales, so the accumulator is the
    // result ----
    const int m_base = wave * 32;
    float* slab = yw + (size_t)(SPLITK ? blockIdx.y : 0) * M * N;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m_base + f * 16 + (lane >> 4) * 4 + r;
            if (row >= M) continue;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                const float v = acc[f][n][r];
                const size_t at = (size_t)row * N + n0 + n * 16 + (lane & 15);
                if (SPLITK) slab[at] = v;
                else y[at] = f2bf(v);
            }
        }
}

// nf: 4 (BN=64) or 8 (BN=128). 1 <= M <= 256; N % (16*nf) == 0;
// K % 64 == 0. residual/norm_weight/out (all or none, nsk > 1, covered N):
// the split-K reduce becomes the fused reduce + residual-add + RMSNorm, as
// for launch_gemm_w8_m256.
extern "C" hipError_t launch_gemm_w4_m256(
    void* y, float* workspace, const void* x, const void* q, const void* s,
    int M, int N, int K, int nsk, int nf, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > 256) return hipErrorInvalidValue;
    if (nf != 4 && nf != 8) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % (16 * nf)) != 0 || (K % G4_BK) != 0)
        return hipErrorInvalidValue;
    if (nsk < 1 || (nsk > 1 && workspace == nullptr)) return hipErrorInvalidValue;
    const bool fuse_norm =
        residual != nullptr || norm_weight != nullptr || out != nullptr;
    if (fuse_norm && (residual == nullptr || norm_weight == nullptr ||
                      out == nullptr || nsk < 2 || !gemm_reduce_rmsnorm_covers(N)))
        return hipErrorInvalidValue;
    int mw = 1;
    while (mw * 32 < M) mw *= 2;  // 1,2,4,8
    dim3 grid(N / (16 * nf), nsk);
    dim3 block(mw * WAVE_SIZE);
#define G4_L2(MWV, NFV, SPLIT)                                                 \
    gemm_w4_m256_kernel<MWV, NFV, SPLIT><<<grid, block, 0, stream>>>(          \
        (bf16*)y, workspace, (const bf16*)x, (const uint8_t*)q,                \
        (const uint8_t*)s, M, N, K, nsk)
#define G4_L1(MWV, NFV)                                                        \
    do {                                                                       \
        if (nsk > 1) G4_L2(MWV, NFV, true);                                    \
        else G4_L2(MWV, NFV, false);                                           \
    } while (0)
#define G4_L0(MWV)                                                             \
    do {                                                                       \
        if (nf == 4) G4_L1(MWV, 4);                                            \
        else G4_L1(MWV, 8);                                                    \
    } while (0)
    switch (mw) {
        case 1: G4_L0(1); break;
        case 2: G4_L0(2); break;
        case 4: G4_L0(4); break;
        default: G4_L0(8); break;
    }
#undef G4_L0
#undef G4_L1
#undef G4_L2
    HIP_CHECK_LAST();
    return launch_splitk_tail(y, workspace, M, N, nsk, residual, norm_weight,
                              eps, out, stream);
}
