// Grouped expert GEMM with MXFP4 expert weights (W4A16) for gfx950: the
// grouped GEMM of moe.hip (same tile walk over moe_align's sorted_pairs /
// tile_expert, same BM = 16·MF row tiles, same two epilogues, same
// v_mfma_f32_16x16x32_bf16) with a 4.25-bit weight stream.
//
// Resident layout (ops.moe_pack_weights_mxfp4), k grouped by 128 so that a
// lane's share of one 16x16 B fragment over four k32 steps is ONE 16-byte
// load:
//   nibbles [E][K/128][N/16][64 lanes][16 B]  lane = (k chunk of 8)·16 +
//           column, as in the bf16 panel; dword j of the 16 bytes holds the
//           lane's 8 nibbles of k32 step j of the group (k ascending from
//           the low nibble of byte 0)
//   scales  [E][K/128][N/16][16 columns][4 B]  byte j = the e8m0 block scale
//           of that column for k32 step j: one dword per (column, group)
//
// Every wave streams the nibbles and scale dwords of its own n-fragments
// from HBM straight into a register ring, MW_D - 1 groups ahead, and converts a
// k32 step with w4_cvt8 (v_cvt_scalef32_pk_bf16_fp4, exact) immediately
// before its MFMAs. Waves own disjoint columns, so nothing is converted
// twice and weights never pass through LDS. A rows are gathered through
// sorted_pairs and staged in LDS once per group for the four waves (double
// buffered); they ride the same register ring, issued before the group's
// weights, so the wait that precedes staging a tile leaves every weight load
// issued after it in flight.
//
// One fp32 accumulator per (m-fragment, n-fragment), k-steps ascending: the
// MFMA inputs and order of moe_gemm_kernel, so the result is bit-identical
// to that kernel run on the dequantised weights.
//
// A group of one fragment costs 5 VGPRs per lane (16 for bf16 over the same
// k), an A group 4·MF. The ring is MW_D = 4 groups deep: depths 2, 4, 6 and 8
// were timed on the card (profiles/r12_moe_mxfp4.md) and the deeper rings
// lost more in resident waves than they gained in bytes in flight per wave.
//
// As in moe.hip: nothing is read on the host, no float atomic, plain vector
// stores; an unused tile returns uniformly before any barrier; a padding
// row reads row 0 of `a` (in bounds) and is never stored.

#include "common.h"
#include "w4_cvt.h"

// see moe.hip: new kernels are compiled without the packed fp32 VALU forms
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int EPI_SWIGLU = 0;
constexpr int EPI_DOWN = 1;
constexpr int MW_WAVES = 4;
constexpr int MW_THREADS = MW_WAVES * WAVE_SIZE;
constexpr int MW_GK = 128;          // k of one group: four MFMA k-steps
constexpr int MW_ROW = MW_GK * 2;   // bytes of one staged A row
constexpr int MW_D = 4;             // register ring: MW_D - 1 groups of loads ahead

__device__ __forceinline__ float mw_silu(float g) {
    return g / (1.f + __expf(-g));
}

// grid (max_tiles, N / BN). out, a, sorted_pairs, tile_expert, rweights as
// in moe_gemm_kernel. wq: [E][K/128][N/16][64][16] nibble bytes, ws:
// [E][K/128][N/16][16][4] scale bytes.
template <int MF, int EPI>
__global__ __launch_bounds__(MW_THREADS) void moe_gemm_w4_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ a,
    const uint8_t* __restrict__ wq, const uint8_t* __restrict__ ws,
    const int* __restrict__ sorted_pairs, const int* __restrict__ tile_expert,
    const float* __restrict__ rweights, int N, int K, int k) {
    constexpr int D = MW_D;
    static_assert(D % 2 == 0, "the A buffer parity follows the ring slot");
    constexpr int BM = 16 * MF;
    constexpr int NFW = EPI == EPI_SWIGLU ? 2 : 1;  // n-fragments per wave
    constexpr int BN = MW_WAVES * NFW * 16;
    constexpr int ABUF = BM * MW_ROW;  // bytes of one staged A tile

    __shared__ __attribute__((aligned(16))) char as[2 * ABUF];
    __shared__ int pairs[BM];

    const int tile = blockIdx.x;
    const int e = tile_expert[tile];
    if (e < 0) return;  // uniform: an unused tile
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE_SIZE - 1);
    const int wave = tid >> 6;
    if (tid < BM) pairs[tid] = sorted_pairs[tile * BM + tid];
    __syncthreads();

    // A staging: a row of the tile is 16 chunks of 16 bytes; thread -> row
    // tid/16 (+16 per chunk c < MF), chunk tid%16. Rows are 256 bytes, a
    // whole turn of the banks, so the LDS chunk is XORed with the row and
    // the 16 rows of a fragment read spread over all of them. A padding row
    // reads row 0 of `a` (in bounds) and is never stored.
    const bf16* asrc[MF];
    int adst[MF];
#pragma unroll
    for (int c = 0; c < MF; ++c) {
        const int r = (tid >> 4) + 16 * c;
        const int pair = pairs[r];
        size_t src = 0;
        if (pair >= 0)
            src = EPI == EPI_SWIGLU ? (size_t)(pair / k) : (size_t)tile * BM + r;
        asrc[c] = a + src * K + (tid & 15) * 8;
        adst[c] = r * MW_ROW + (((tid & 15) ^ (r & 15)) << 4);
    }

    // B: this wave's NFW fragments; per group a fragment is 1 KiB of
    // nibbles (16 bytes per lane) and 64 bytes of scales (a dword per column)
    const size_t frag0 = (size_t)blockIdx.y * (BN / 16) + wave * NFW;
    const size_t qstride = (size_t)N * 64;  // nibble bytes between groups
    const size_t sstride = (size_t)N * 4;   // scale bytes between groups
    const uint8_t* qsrc = wq + (size_t)e * N * (K / 2) + frag0 * 1024 + lane * 16;
    const uint8_t* ssrc = ws + (size_t)e * N * (K / 32) + frag0 * 64 + (lane & 15) * 4;

    bf16x8 areg[D][MF];
    uint4 qreg[D][NFW];
    uint32_t sreg[D][NFW];
    f32x4 acc[MF][NFW];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int n = 0; n < NFW; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // A first, then B: the wait before an A tile is staged leaves the B
    // loads issued after it in flight
#define MW_LOAD(SLOT, G)                                                       \
    do {                                                                       \
        _Pragma("unroll") for (int c = 0; c < MF; ++c)                         \
            areg[SLOT][c] = *reinterpret_cast<const bf16x8*>(                  \
                asrc[c] + (size_t)(G) * MW_GK);                                \
        _Pragma("unroll") for (int n = 0; n < NFW; ++n) {                      \
            qreg[SLOT][n] = *reinterpret_cast<const uint4*>(                   \
                qsrc + (size_t)(G) * qstride + n * 1024);                      \
            sreg[SLOT][n] = *reinterpret_cast<const uint32_t*>(                \
                ssrc + (size_t)(G) * sstride + n * 64);                        \
        }                                                                      \
    } while (0)
#define MW_STAGE(SLOT, BUF)                                                    \
    do {                                                                       \
        _Pragma("unroll") for (int c = 0; c < MF; ++c)                         \
            *reinterpret_cast<bf16x8*>(as + (BUF) * ABUF + adst[c]) =          \
                areg[SLOT][c];                                                 \
    } while (0)

    const int groups = K / MW_GK;
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
        if (d < groups) MW_LOAD(d, d);
    MW_STAGE(0, 0);
    __syncthreads();

    const int arow = lane & 15;  // fragment row; m-fragment f adds 16 f
    const int akc = lane >> 4;   // 16-byte k-chunk within a k-step
    for (int g0 = 0; g0 < groups; g0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int g = g0 + d;
            if (g >= groups) break;
            if (g + D - 1 < groups) MW_LOAD((d + D - 1) % D, g + D - 1);
            const char* buf = as + (d & 1) * ABUF;  // D is even: g&1 == d&1
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                bf16x8 af[MF];
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const int r = f * 16 + arow;
                    af[f] = *reinterpret_cast<const bf16x8*>(
                        buf + r * MW_ROW + (((ks * 4 + akc) ^ (r & 15)) << 4));
                }
#pragma unroll
                for (int n = 0; n < NFW; ++n) {
                    const uint4 q4 = qreg[d][n];
                    const uint32_t q =
                        ks == 0 ? q4.x : ks == 1 ? q4.y : ks == 2 ? q4.z : q4.w;
                    union { uint32_t u[4]; bf16x8 v; } b;
                    w4_cvt8(q, w4_scale((sreg[d][n] >> (8 * ks)) & 0xffu), b.u);
#pragma unroll
                    for (int f = 0; f < MF; ++f)
                        acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            af[f], b.v, acc[f][n], 0, 0, 0);
                }
            }
            // the other buffer was last read before the previous barrier
            if (g + 1 < groups) MW_STAGE((d + 1) % D, (d + 1) & 1);
            __syncthreads();
        }
    }
#undef MW_LOAD
#undef MW_STAGE

    // C fragment: row 4 (lane / 16) + r, column lane % 16
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rt = f * 16 + (lane >> 4) * 4 + r;
            const int pair = pairs[rt];
            if (pair < 0) continue;
            if constexpr (EPI == EPI_SWIGLU) {
                // fragment 0 is the gate, fragment 1 the up half of the
                // same 16 output columns (block-16 interleave)
                const size_t col =
                    (size_t)blockIdx.y * (BN / 2) + wave * 16 + (lane & 15);
                out[((size_t)tile * BM + rt) * (N / 2) + col] =
                    f2bf(mw_silu(acc[f][0][r]) * acc[f][1][r]);
            } else {
                const size_t col =
                    (size_t)blockIdx.y * BN + wave * 16 + (lane & 15);
                out[(size_t)pair * N + col] =
                    f2bf(rweights[pair] * acc[f][0][r]);
            }
        }
}

template <int EPI>
hipError_t launch_w4_epi(int mf, dim3 grid, hipStream_t stream,
                         bf16* out, const bf16* a, const uint8_t* wq,
                         const uint8_t* ws, const int* sorted_pairs,
                         const int* tile_expert, const float* rweights, int N,
                         int K, int k) {
#define MOE_W4_LAUNCH(MF)                                                      \
    moe_gemm_w4_kernel<MF, EPI><<<grid, MW_THREADS, 0, stream>>>(              \
        out, a, wq, ws, sorted_pairs, tile_expert, rweights, N, K, k)
    switch (mf) {
        case 1: MOE_W4_LAUNCH(1); break;
        case 2: MOE_W4_LAUNCH(2); break;
        case 4: MOE_W4_LAUNCH(4); break;
        default: return hipErrorInvalidValue;
    }
#undef MOE_W4_LAUNCH
    HIP_CHECK_LAST();
    return hipSuccess;
}

}  // namespace

// moe_w4_prefill.hip: the 128-row tile
extern "C" hipError_t launch_moe_gemm_w4_big(
    void* out, const void* a, const void* wq, const void* ws,
    const int* sorted_pairs, const int* tile_expert, const float* rweights,
    int epi, int max_tiles, int N, int K, int k, hipStream_t stream);

// epi 0: act [cap, N/2] = swiglu(gather(x) · dequant(w[e])^T), N = 2I, K = H
// epi 1: y_pair [P, N] = rweights · (act · dequant(w[e])^T),   N = H,  K = I
// mf = 8 is moe_gemm_w4_big (moe_w4_prefill.hip): N % 128 == 0 for both
extern "C" hipError_t launch_moe_gemm_w4(
    void* out, const void* a, const void* wq, const void* ws,
    const int* sorted_pairs, const int* tile_expert, const float* rweights,
    int epi, int mf, int max_tiles, int N, int K, int k,
    hipStream_t stream) {
    if (max_tiles <= 0 || k < 1 || K <= 0 || K % MW_GK != 0)
        return hipErrorInvalidValue;
    if (mf == 8)
        return launch_moe_gemm_w4_big(out, a, wq, ws, sorted_pairs, tile_expert,
                                      rweights, epi, max_tiles, N, K, k, stream);
    if (epi == EPI_SWIGLU) {
        if (N <= 0 || N % 128 != 0) return hipErrorInvalidValue;
        return launch_w4_epi<EPI_SWIGLU>(
            mf, dim3(max_tiles, N / 128), stream, (bf16*)out,
            (const bf16*)a, (const uint8_t*)wq, (const uint8_t*)ws,
            sorted_pairs, tile_expert, rweights, N, K, k);
    }
    if (epi != EPI_DOWN || N <= 0 || N % 64 != 0) return hipErrorInvalidValue;
    return launch_w4_epi<EPI_DOWN>(
        mf, dim3(max_tiles, N / 64), stream, (bf16*)out, (const bf16*)a,
        (const uint8_t*)wq, (const uint8_t*)ws, sorted_pairs, tile_expert,
        rweights, N, K, k);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
