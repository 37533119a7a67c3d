// Macro-tile W8A16 decode GEMM for gfx950:
//   Y[M,N] = X[M,K] · (scale ⊙ Q)[N,K]^T,  X bf16, Q fp8 e4m3fn, fp32 acc,
//   M <= 256.
//
// The streaming fp8 kernel (gemm_w8.hip) is right for M <= 16 and loses at
// the batch sizes a gateway runs at (profiles/r04_fp8_weights.md): every
// 64-column stripe re-reads all of X, and every wave of a workgroup owns M
// rows, so each wave converts the same fp8 fragments again. This kernel is
// gemm_m256r_kernel (gemm_m256.hip, register-staged variant) with an fp8
// W stream:
//
// - One workgroup owns ALL M rows of a BN = 16*NF column stripe for its
//   K-slice; wave w owns rows [32w, 32w+32): 2 m-fragments x NF
//   n-fragments of v_mfma_f32_16x16x32_bf16, BK = 64, two LDS buffers.
// - X is staged as there: linear 128-B-line loads, XOR swizzle on the
//   ds_write address, per-unit row clamp for rows >= M.
// - Q is the fragment-major fp8 twin [K/64, N/16, 64, 16]
//   (ops.swizzle_weight_frag_fp8): one k64 tile of the stripe is NF
//   contiguous 1-KiB units, one 16-B load per lane each, dealt round-robin
//   over the waves. The LOADING wave converts its 16 bytes once (cvt_pk +
//   exact truncation, w8_cvt4) into two bf16x8 — bytes 0-7 are k32 half 0,
//   bytes 8-15 half 1 — and writes them to (h*NF + n)*1024 + lane*16 of
//   the buffer's W area. The fp8 twin's lane order equals the bf16
//   fragment twin's, so from the barrier on the k-loop is
//   gemm_m256r_kernel's: lane-linear ds_read_b128 for B, XOR reads for A,
//   the same MFMAs in the same order. Conversion happens once per
//   workgroup instead of once per wave.
// - The per-output-channel scale multiplies the fp32 accumulator in the
//   epilogue, before the bf16 store or the slab store, as in gemm_w8.hip,
//   so launch_splitk_tail consumes the slabs as they are.
// - split-K over grid.y writes private fp32 slabs; an empty slice writes
//   zeros.

#include "common.h"
#include "gemm_launch.h"
#include "w8_cvt.h"

#define GW_BK 64  // k-depth of one staged tile (2 MFMA k-steps)

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t u32x4;

__device__ __forceinline__ f32x4 gw_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// compiler-only memory fence around the raw s_barrier (see gemm_m256.hip)
__device__ __forceinline__ void gw_cfence() { asm volatile("" ::: "memory"); }

// words 2h, 2h+1 of a lane's 16 fp8 bytes -> its bf16 B fragment of k32
// half h
__device__ __forceinline__ bf16x8 gw_frag(const u32x4& q, int h) {
    union { uint32_t u[4]; bf16x8 v; } c;
    w8_cvt4(q[2 * h], c.u[0], c.u[1]);
    w8_cvt4(q[2 * h + 1], c.u[2], c.u[3]);
    return c.v;
}

// MW = waves per block (BM = 32*MW rows), NF = 16-col n-fragments (BN =
// 16*NF).
template <int MW, int NF, bool SPLITK>
__launch_bounds__(MW * WAVE_SIZE)
__global__ void gemm_w8_m256_kernel(
    bf16* __restrict__ y,             // [M, N] (!SPLITK)
    float* __restrict__ yw,           // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,       // [M, K]
    const uint8_t* __restrict__ q,    // fragment-major [K/64][N/16][64][16]
    const float* __restrict__ scale,  // [N]
    int M, int N, int K, int nsk) {
    constexpr int BM = MW * 32;
    constexpr int BN = NF * 16;
    constexpr int XB = BM * GW_BK * 2;  // X tile bytes (row stride 128)
    constexpr int WB = GW_BK * BN * 2;  // W tile bytes as bf16 (2*NF frags)
    constexpr int BUFB = XB + WB;
    constexpr int XG_W = 4;                   // 1-KiB x units per wave
    constexpr int WG_W = (NF + MW - 1) / MW;  // 1-KiB fp8 units per wave
    static_assert(NF % MW == 0 || MW > NF, "W unit split uneven across waves");

    __shared__ __attribute__((aligned(16))) char smem[2 * BUFB];

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    // uniform in fact, but not provably so to the compiler: the W-unit
    // guard below must be a scalar branch
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = blockIdx.x * BN;
    const int n16 = N / 16;

    const int ktiles = K / GW_BK;
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
    // waves carry none
    const uint8_t* wsrc = q + ((size_t)(n0 / 16) * 64 + lane) * 16;
    const size_t wstep = (size_t)n16 * 1024;  // one k64 plane

    f32x4 acc[2][NF];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    bf16x8 xr[XG_W];  // one in-flight staging tile
    u32x4 wr[WG_W];

#define GW_LOAD(T)                                                             \
    do {                                                                       \
        const int kt__ = kt0 + (T);                                            \
        _Pragma("unroll") for (int i = 0; i < XG_W; ++i) xr[i] =               \
            *(const __attribute__((address_space(1))) bf16x8*)(                \
                xsrc[i] + (size_t)(kt__)*GW_BK);                               \
        _Pragma("unroll") for (int j = 0; j < WG_W; ++j) {                     \
            if (wave + j * MW < NF)                                            \
                wr[j] = *(const __attribute__((address_space(1))) u32x4*)(     \
                    wsrc + (size_t)(kt__)*wstep + (wave + j * MW) * 1024);     \
        }                                                                      \
    } while (0)
#define GW_WRITE(T)                                                            \
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
                        gw_frag(wr[j], h);                                     \
            }                                                                  \
        }                                                                      \
    } while (0)

    const int arow0 = wave * 32 + (lane & 15);
    const int alk = lane >> 4;

    if (ntiles > 0) {
        GW_LOAD(0);
        GW_WRITE(0);
        if (ntiles > 1) GW_LOAD(1);  // in flight during compute(0)
        // s_barrier waits for no counter: tile 0's ds_writes must have
        // landed before another wave reads them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        gw_cfence();
        for (int t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) {
                // regs hold tile t+1 (issued last iter): convert + write
                // after the barrier, then immediately re-issue for tile
                // t+2 so the loads overlap compute(t). The ds_reads below
                // queue behind these ds_writes, so the writes have landed
                // by the time the MFMAs, and the barrier after them, run.
                GW_WRITE(t + 1);
                if (t + 2 < ntiles) GW_LOAD(t + 2);
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
                        acc[f][n] = gw_mfma(a[f], b[n], acc[f][n]);
            }
            gw_cfence();
            __builtin_amdgcn_s_barrier();
            gw_cfence();
        }
    }
#undef GW_LOAD
#undef GW_WRITE

    // ---- epilogue: C fragment row = 4*(lane>>4) + r, col = lane&15; the
    // channel scale goes onto the fp32 accumulator before any store ----
    float sc[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) sc[n] = scale[n0 + n * 16 + (lane & 15)];
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
                const float v = acc[f][n][r] * sc[n];
                const size_t at = (size_t)row * N + n0 + n * 16 + (lane & 15);
                if (SPLITK) slab[at] = v;
                else y[at] = f2bf(v);
            }
        }
}

// nf: 4 (BN=64) or 8 (BN=128). 1 <= M <= 256; N % (16*nf) == 0;
// K % 64 == 0. residual/norm_weight/out (all or none, nsk > 1, covered N):
// the split-K reduce becomes the fused reduce + residual-add + RMSNorm, as
// for launch_gemm_m256.
extern "C" hipError_t launch_gemm_w8_m256(
    void* y, float* workspace, const void* x, const void* q,
    const float* scale, int M, int N, int K, int nsk, int nf, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > 256) return hipErrorInvalidValue;
    if (nf != 4 && nf != 8) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % (16 * nf)) != 0 || (K % GW_BK) != 0)
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
#define GW_L2(MWV, NFV, SPLIT)                                                 \
    gemm_w8_m256_kernel<MWV, NFV, SPLIT><<<grid, block, 0, stream>>>(          \
        (bf16*)y, workspace, (const bf16*)x, (const uint8_t*)q, scale, M, N,   \
        K, nsk)
#define GW_L1(MWV, NFV)                                                        \
    do {                                                                       \
        if (nsk > 1) GW_L2(MWV, NFV, true);                                    \
        else GW_L2(MWV, NFV, false);                                           \
    } while (0)
#define GW_L0(MWV)                                                             \
    do {                                                                       \
        if (nf == 4) GW_L1(MWV, 4);                                            \
        else GW_L1(MWV, 8);                                                    \
    } while (0)
    switch (mw) {
        case 1: GW_L0(1); break;
        case 2: GW_L0(2); break;
        case 4: GW_L0(4); break;
        default: GW_L0(8); break;
    }
#undef GW_L0
#undef GW_L1
#undef GW_L2
    HIP_CHECK_LAST();
    return launch_splitk_tail(y, workspace, M, N, nsk, residual, norm_weight,
                              eps, out, stream);
}
