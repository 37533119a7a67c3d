// The register-staged macro-tile GEMM pipeline for gfx950, written once:
//   Y[M,N] = X[M,K] · W[N,K]^T, X bf16, fp32 accumulation, M <= 256.
// gemm_m256.hip (bf16 weights, its variant 1), gemm_w8_m256.hip (fp8 e4m3
// weights) and gemm_w4_m256.hip (MXFP4 weights) instantiate it with a
// W-operand policy each.
//
// - grid = (N/BN column stripes) x (split-K slices), BN = 16*NF. One
//   workgroup owns ALL M rows of its stripe for its K-slice: W is streamed
//   exactly once and X travels the load path once per block in full 128-B
//   lines. MW waves; wave w owns rows [32w, 32w+32): 2 m-fragments x NF
//   n-fragments of v_mfma_f32_16x16x32_bf16 per 32-deep k-step.
// - Both operands are staged through registers into LDS in k64 tiles, two
//   LDS buffers. Ordinary vector loads ride the full per-CU load path
//   (~122 GB/s) where the LDS-DMA of gemm_m256.hip's glds variant lands at
//   ~25-40 GB/s per CU (profiles/r02_gemm_m256_probe.md).
//   X: unit i of a wave is rows [32w+8i, +8), loaded linearly; the
//   bank-conflict XOR goes on the ds_write address and, the same
//   involution, on the A ds_read. Rows >= M re-read row 0, never stored.
//   W: the policy's units, dealt round-robin (unit wave + j*MW); each lands
//   as bf16 B fragments at (h*NF + n)*1024 + lane*16 of the buffer's W area
//   (k32 half h, n-fragment n), so the B ds_read_b128 is lane-linear and
//   the MFMA nest is the same for every weight format — which is what
//   keeps the quantised kernels bit-identical to the bf16 one on equal
//   weights.
// - Loads run two tiles ahead of the MFMAs: the registers hold tile t+1
//   while tile t is computed; after the barrier they are written to the
//   other buffer and re-issued for tile t+2 at once. The ds_reads of tile t
//   queue behind those ds_writes, so the writes have landed by the time the
//   MFMAs, and the barrier after them, run. Barriers are raw s_barriers
//   between compiler fences; s_barrier waits for no counter, hence the
//   explicit lgkmcnt(0) before the first one.
// - no atomics: every workgroup fully writes the stripe it owns, of y or
//   (split-K) of the private fp32 slab blockIdx.y — a slice with no k-tiles
//   writes zeros. launch_splitk_tail reduces the slabs.
//
// A policy W<NF> supplies only what differs between weight formats:
//   NF, UNITS              n-fragments per stripe; W units per k64 tile
//   Regs                   one unit's registers
//   init(w, aux, N, n0, lane)   point at the stripe
//   load(regs, unit, kt)   issue the loads of `unit` of k64 tile kt
//   write(wa, unit, lane, regs)  convert and ds_write the unit's bf16
//                          fragments into the W area `wa` (image above)
//   SCALED                 multiply the accumulator by scale[col] (aux, fp32
//                          [N]) before the store
//   SWIGLU                 the format has a fused gate/up swiglu epilogue
// aux is the launch's second weight operand: the channel scales of a
// SCALED policy, or whatever else a policy streams beside w
// (gemm_w4_m256.hip: the e8m0 block scales).
#pragma once

#include "common.h"
#include "gemm_launch.h"

#define GM_BK 64  // k-depth of one staged tile (2 MFMA k-steps)

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

#define GM_GLOBAL __attribute__((address_space(1)))
#define GM_LDS __attribute__((address_space(3)))

__device__ __forceinline__ f32x4 gm_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// compiler-only memory fence: keeps LDS accesses from being scheduled
// across a raw s_barrier (the builtin is convergent but not a compiler
// memory barrier)
__device__ __forceinline__ void gm_cfence() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ float gm_silu(float g) {
    return g / (1.f + __expf(-g));
}

// Store a wave's 32 x 16*NF accumulator block; C fragment row =
// 4*(lane>>4) + r, col = lane&15. A channel scale goes onto the fp32
// accumulator before any store, so split-K slabs hold finished partial sums.
// SWIGLU: the weight is the block-16 interleaved gate/up twin
// (ops.interleave_gate_up): even fragment n holds the GATE columns,
// fragment n+1 the UP columns of the SAME 16 output columns — the pair
// lands in the same lane, so silu(g)*u needs no cross-lane traffic and y is
// [M, N/2].
template <int NF, bool SPLITK, bool SWIGLU, bool SCALED>
__device__ __forceinline__ void gm_epilogue(
    const f32x4 (&acc)[2][NF], bf16* __restrict__ y, float* __restrict__ yw,
    const float* __restrict__ scale, int M, int N, int n0, int wave, int lane) {
    static_assert(!(SWIGLU && (SPLITK || SCALED)),
                  "fused swiglu epilogue needs nsk=1 and unscaled weights");
    static_assert(!SWIGLU || NF % 2 == 0, "fused swiglu pairs fragments");
    float sc[NF];
    if constexpr (SCALED) {
#pragma unroll
        for (int n = 0; n < NF; ++n) sc[n] = scale[n0 + n * 16 + (lane & 15)];
    }
    float* slab = yw + (size_t)(SPLITK ? blockIdx.y : 0) * M * N;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 32 + f * 16 + (lane >> 4) * 4 + r;
            if (row >= M) continue;
            if constexpr (SWIGLU) {
#pragma unroll
                for (int n = 0; n < NF; n += 2)
                    y[(size_t)row * (N >> 1) + (n0 >> 1) + (n >> 1) * 16 +
                      (lane & 15)] =
                        f2bf(gm_silu(acc[f][n][r]) * acc[f][n + 1][r]);
            } else {
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    float v = acc[f][n][r];
                    if constexpr (SCALED) v *= sc[n];
                    const size_t at = (size_t)row * N + n0 + n * 16 + (lane & 15);
                    if (SPLITK) slab[at] = v;
                    else y[at] = f2bf(v);
                }
            }
        }
}

// MW = waves per block (BM = 32*MW rows); W::NF = 16-col n-fragments (BN =
// 16*NF).
template <class W, int MW, bool SPLITK, bool SWIGLU>
__launch_bounds__(MW * WAVE_SIZE)
__global__ void gemm_macro_kernel(
    bf16* __restrict__ y,          // [M, N] (!SPLITK; [M, N/2] when SWIGLU)
    float* __restrict__ yw,        // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,    // [M, K]
    const void* __restrict__ w,    // the policy's weight layout
    const void* __restrict__ aux,  // [N] fp32 scales (W::SCALED) / policy's own
    int M, int N, int K, int nsk) {
    constexpr int NF = W::NF;
    constexpr int BM = MW * 32;
    constexpr int BN = NF * 16;
    constexpr int XB = BM * GM_BK * 2;  // X tile bytes (row stride 128)
    constexpr int WB = GM_BK * BN * 2;  // W tile bytes as bf16 (2*NF frags)
    constexpr int BUFB = XB + WB;
    constexpr int XG_W = 4;                         // 1-KiB x units per wave
    constexpr int WG_W = (W::UNITS + MW - 1) / MW;  // W units per wave
    // with fewer units than waves the high waves carry none
    constexpr bool W_EVEN = W::UNITS % MW == 0;
    static_assert(W_EVEN || MW > W::UNITS, "W unit split uneven across waves");

    __shared__ __attribute__((aligned(16))) char smem[2 * BUFB];

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    // uniform in fact, but not provably so to the compiler: the W-unit
    // guard below must be a scalar branch
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = blockIdx.x * BN;

    const int ktiles = K / GM_BK;
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
    // ds_write byte offset (swizzled) per unit: row*128 + (c ^ row&7)*16
    const int xwoff = (xrow & (BM - 1)) * 128 + (((lane & 7) ^ (xrow & 7)) << 4);

    W wp;
    wp.init(w, aux, N, n0, lane);

    f32x4 acc[2][NF];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    bf16x8 xr[XG_W];  // one in-flight staging tile
    typename W::Regs wr[WG_W];

    auto load = [&](int T) __attribute__((always_inline)) {
        const int kt = kt0 + T;
#pragma unroll
        for (int i = 0; i < XG_W; ++i)
            xr[i] = *(const GM_GLOBAL bf16x8*)(xsrc[i] + (size_t)kt * GM_BK);
#pragma unroll
        for (int j = 0; j < WG_W; ++j)
            if (W_EVEN || wave + j * MW < W::UNITS)
                wp.load(wr[j], wave + j * MW, kt);
    };
    auto write = [&](int T) __attribute__((always_inline)) {
        GM_LDS char* buf = (GM_LDS char*)(smem + (T & 1) * BUFB);
#pragma unroll
        for (int i = 0; i < XG_W; ++i)
            *(GM_LDS bf16x8*)(buf + xwoff + i * 8 * 128) = xr[i];
#pragma unroll
        for (int j = 0; j < WG_W; ++j)
            if (W_EVEN || wave + j * MW < W::UNITS)
                W::write(buf + XB, wave + j * MW, lane, wr[j]);
    };

    const int arow0 = wave * 32 + (lane & 15);
    const int alk = lane >> 4;

    if (ntiles > 0) {
        load(0);
        write(0);
        if (ntiles > 1) load(1);  // in flight during compute(0)
        // s_barrier waits for no counter: tile 0's ds_writes must have
        // landed before another wave reads them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        gm_cfence();
        for (int t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) {
                // regs hold tile t+1 (issued last iter): convert + write
                // after the barrier, then immediately re-issue for tile
                // t+2 so the loads overlap compute(t)
                write(t + 1);
                if (t + 2 < ntiles) load(t + 2);
            }
            const GM_LDS char* buf = (const GM_LDS char*)(smem + (t & 1) * BUFB);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 a[2], b[NF];
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int row = arow0 + f * 16;
                    const int chunk = (ks * 4 + alk) ^ (row & 7);
                    a[f] = *(const GM_LDS bf16x8*)(buf + (row & (BM - 1)) * 128 +
                                                   chunk * 16);
                }
#pragma unroll
                for (int n = 0; n < NF; ++n)
                    b[n] = *(const GM_LDS bf16x8*)(buf + XB + (ks * NF + n) * 1024 +
                                                   lane * 16);
#pragma unroll
                for (int n = 0; n < NF; ++n)
#pragma unroll
                    for (int f = 0; f < 2; ++f)
                        acc[f][n] = gm_mfma(a[f], b[n], acc[f][n]);
            }
            // all waves done reading buf t&1 before iter t+1 refills it
            gm_cfence();
            __builtin_amdgcn_s_barrier();
            gm_cfence();
        }
    }

    gm_epilogue<NF, SPLITK, SWIGLU, W::SCALED>(acc, y, yw, (const float*)aux, M,
                                               N, n0, wave, lane);
}

struct GemmMacroArgs {
    bf16* y;
    float* yw;
    const bf16* x;
    const void* w;
    const void* aux;
    int M, N, K, nsk;
};

template <class W, int MW>
static void gemm_macro_go(const GemmMacroArgs& a, bool swiglu,
                          hipStream_t stream) {
    const dim3 grid(a.N / (16 * W::NF), a.nsk), block(MW * WAVE_SIZE);
#define GM_GO(SPLIT, SW)                                                       \
    gemm_macro_kernel<W, MW, SPLIT, SW><<<grid, block, 0, stream>>>(           \
        a.y, a.yw, a.x, a.w, a.aux, a.M, a.N, a.K, a.nsk)
    if constexpr (W::SWIGLU) {
        if (swiglu) {
            GM_GO(false, true);
            return;
        }
    }
    if (a.nsk > 1) GM_GO(true, false);
    else GM_GO(false, false);
#undef GM_GO
}

// the fewest waves (1, 2, 4, 8) whose 32 rows each cover M
template <class W>
static void gemm_macro_by_m(const GemmMacroArgs& a, bool swiglu,
                            hipStream_t stream) {
    if (a.M <= 32) gemm_macro_go<W, 1>(a, swiglu, stream);
    else if (a.M <= 64) gemm_macro_go<W, 2>(a, swiglu, stream);
    else if (a.M <= 128) gemm_macro_go<W, 4>(a, swiglu, stream);
    else gemm_macro_go<W, 8>(a, swiglu, stream);
}

// nf: 4 (BN=64) or 8 (BN=128). 1 <= M <= 256; N % (16*nf) == 0;
// K % 64 == 0. swiglu (W::SWIGLU formats, nsk == 1): y is [M, N/2].
// residual/norm_weight/out (all or none, nsk > 1, covered N): the split-K
// reduce becomes the fused reduce + residual-add + RMSNorm
// (gemm_skinny.hip) — residual is updated in place, out receives the
// normed row and y is not written.
template <template <int> class W>
static hipError_t launch_gemm_macro(
    void* y, float* workspace, const void* x, const void* w, const void* aux,
    int M, int N, int K, int nsk, int nf, int swiglu, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > 256) return hipErrorInvalidValue;
    if (nf != 4 && nf != 8) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % (16 * nf)) != 0 || (K % GM_BK) != 0)
        return hipErrorInvalidValue;
    if (nsk < 1 || (nsk > 1 && workspace == nullptr)) return hipErrorInvalidValue;
    const bool fuse_norm =
        residual != nullptr || norm_weight != nullptr || out != nullptr;
    if (fuse_norm && (residual == nullptr || norm_weight == nullptr ||
                      out == nullptr || nsk < 2 || !gemm_reduce_rmsnorm_covers(N)))
        return hipErrorInvalidValue;
    // the fp32 split-K slabs hold pre-activation partials — no fusion point
    if (swiglu && (!W<4>::SWIGLU || nsk != 1)) return hipErrorInvalidValue;
    const GemmMacroArgs a{(bf16*)y, workspace, (const bf16*)x, w, aux,
                          M,        N,         K,              nsk};
    if (nf == 4) gemm_macro_by_m<W<4>>(a, swiglu != 0, stream);
    else gemm_macro_by_m<W<8>>(a, swiglu != 0, stream);
    HIP_CHECK_LAST();
    return launch_splitk_tail(y, workspace, M, N, nsk, residual, norm_weight,
                              eps, out, stream);
}
