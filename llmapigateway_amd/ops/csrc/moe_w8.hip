// Grouped expert GEMM with fp8 expert weights (W8A16) for gfx950: the grouped
// GEMM of moe.hip (same tile walk over moe_align's sorted_pairs /
// tile_expert, same BM = 16·MF row tiles, same two epilogues, same
// v_mfma_f32_16x16x32_bf16) with an 8-bit weight stream.
//
// Resident layout (ops.moe_pack_weights_fp8), k grouped by 64 so that a
// lane's share of one 16x16 B fragment over two k32 steps is ONE 16-byte
// load, and every shape moe_check_shapes accepts is served:
//   bits   [E][K/64][N/16][64 lanes][16 B]  the per-expert form of
//          swizzle_weight_frag_fp8: lane = (k chunk of 8)·16 + column, as in
//          the bf16 panel; bytes 0-7 are the lane's 8 e4m3 values of the
//          first k32 step of the group (k ascending), bytes 8-15 of the
//          second
//   scales [E][N] fp32, one power of two per output channel
// gate_up rows (bits and scales alike) are in the block-16 gate/up
// interleave of moe_pack_weights.
//
// Every wave streams the bits of its own n-fragments from HBM straight into
// a register ring, MW8_D - 1 groups ahead, and converts a k32 step with
// w8_cvt4 (exact) immediately before its MFMAs. Waves own disjoint columns,
// so nothing is converted twice and weights never pass through LDS. A rows
// are gathered through sorted_pairs and staged in LDS once per group for the
// four waves (double buffered); they ride the same register ring, issued
// before the group's weights, so the wait that precedes staging a tile
// leaves every weight load issued after it in flight. A 16-row tile
// (MF = 1) is 128 chunks of 16 bytes: only half of the 256 threads stage.
//
// The channel scale multiplies the fp32 accumulator in the epilogue (gate
// and up each by their own, before silu(g)·u). One fp32 accumulator per
// (m-fragment, n-fragment), k-steps ascending: the MFMA inputs and order of
// moe_gemm_kernel, and the scales are powers of two, so the result is
// bit-identical to that kernel run on the dequantised weights.
//
// A group of one fragment costs 4 VGPRs per lane (8 for bf16 over the same
// k), an A group 4, 4, 8 at MF = 1, 2, 4. The ring depth MW8_D was picked on
// the card among 2, 4, 6 and 8 groups: profiles/r17_moe_fp8.md.
//
// As in moe.hip: nothing is read on the host, no float atomic, plain vector
// stores; an unused tile returns uniformly before any barrier; a padding
// row reads row 0 of `a` (in bounds) and is never stored.

#include "common.h"
#include "w8_cvt.h"

// see moe.hip: new kernels are compiled without the packed fp32 VALU forms
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int EPI_SWIGLU = 0;
constexpr int EPI_DOWN = 1;
constexpr int MW8_WAVES = 4;
constexpr int MW8_THREADS = MW8_WAVES * WAVE_SIZE;
constexpr int MW8_GK = 64;           // k of one group: two MFMA k-steps
constexpr int MW8_ROW = MW8_GK * 2;  // bytes of one staged A row
constexpr int MW8_D = 4;             // register ring: MW8_D - 1 groups of loads ahead

__device__ __forceinline__ float mw8_silu(float g) {
    return g / (1.f + __expf(-g));
}

// grid (max_tiles, N / BN). out, a, sorted_pairs, tile_expert, rweights as
// in moe_gemm_kernel. wq: [E][K/64][N/16][64][16] e4m3 bytes, scale: [E][N].
template <int MF, int EPI, int D>
__global__ __launch_bounds__(MW8_THREADS) void moe_gemm_w8_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ a,
    const uint8_t* __restrict__ wq, const float* __restrict__ scale,
    const int* __restrict__ sorted_pairs, const int* __restrict__ tile_expert,
    const float* __restrict__ rweights, int N, int K, int k) {
    static_assert(D % 2 == 0, "the A buffer parity follows the ring slot");
    constexpr int BM = 16 * MF;
    constexpr int NFW = EPI == EPI_SWIGLU ? 2 : 1;  // n-fragments per wave
    constexpr int BN = MW8_WAVES * NFW * 16;
    constexpr int ACH = BM > 32 ? BM / 32 : 1;  // 16-byte A chunks per thread
    constexpr int ABUF = BM * MW8_ROW;          // bytes of one staged A tile

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

    // A staging: a row of the tile is 8 chunks of 16 bytes; thread -> row
    // tid/8 (+32 per chunk), chunk tid%8. At MF = 1 the tile has 16 rows and
    // threads 128..255 stage nothing (aon). The LDS chunk is XORed with the
    // row so the fragment reads below spread over the banks. A padding row
    // reads row 0 of `a` (in bounds) and is never stored.
    const bf16* asrc[ACH];
    int adst[ACH];
    bool aon[ACH];
#pragma unroll
    for (int c = 0; c < ACH; ++c) {
        const int r = (tid >> 3) + 32 * c;
        aon[c] = r < BM;
        const int pair = aon[c] ? pairs[r] : -1;
        size_t src = 0;
        if (pair >= 0)
            src = EPI == EPI_SWIGLU ? (size_t)(pair / k) : (size_t)tile * BM + r;
        asrc[c] = a + src * K + (tid & 7) * 8;
        adst[c] = r * MW8_ROW + (((tid & 7) ^ (r & 7)) << 4);
    }

    // B: this wave's NFW fragments; per group a fragment is 1 KiB of e4m3
    // bytes, 16 per lane
    const size_t frag0 = (size_t)blockIdx.y * (BN / 16) + wave * NFW;
    const size_t qstride = (size_t)N * MW8_GK;  // bytes between groups
    const uint8_t* qsrc = wq + (size_t)e * N * K + frag0 * 1024 + lane * 16;

    bf16x8 areg[D][ACH];
    uint4 qreg[D][NFW];
    f32x4 acc[MF][NFW];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int n = 0; n < NFW; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // A first, then B: the wait before an A tile is staged leaves the B
    // loads issued after it in flight
#define MW8_LOAD(SLOT, G)                                                      \
    do {                                                                       \
        _Pragma("unroll") for (int c = 0; c < ACH; ++c) if (aon[c])            \
            areg[SLOT][c] = *reinterpret_cast<const bf16x8*>(                  \
                asrc[c] + (size_t)(G) * MW8_GK);                               \
        _Pragma("unroll") for (int n = 0; n < NFW; ++n)                        \
            qreg[SLOT][n] = *reinterpret_cast<const uint4*>(                   \
                qsrc + (size_t)(G) * qstride + n * 1024);                      \
    } while (0)
#define MW8_STAGE(SLOT, BUF)                                                   \
    do {                                                                       \
        _Pragma("unroll") for (int c = 0; c < ACH; ++c) if (aon[c])            \
            *reinterpret_cast<bf16x8*>(as + (BUF) * ABUF + adst[c]) =          \
                areg[SLOT][c];                                                 \
    } while (0)

    const int groups = K / MW8_GK;
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
        if (d < groups) MW8_LOAD(d, d);
    MW8_STAGE(0, 0);
    __syncthreads();

    const int arow = lane & 15;  // fragment row; m-fragment f adds 16 f
    const int akc = lane >> 4;   // 16-byte k-chunk within a k-step
    for (int g0 = 0; g0 < groups; g0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int g = g0 + d;
            if (g >= groups) break;
            if (g + D - 1 < groups) MW8_LOAD((d + D - 1) % D, g + D - 1);
            const char* buf = as + (d & 1) * ABUF;  // D is even: g&1 == d&1
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[MF];
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const int r = f * 16 + arow;
                    af[f] = *reinterpret_cast<const bf16x8*>(
                        buf + r * MW8_ROW + (((ks * 4 + akc) ^ (r & 7)) << 4));
                }
#pragma unroll
                for (int n = 0; n < NFW; ++n) {
                    // dwords 2 ks, 2 ks + 1: the lane's 8 e4m3 bytes of the step
                    const uint4 q4 = qreg[d][n];
                    union { uint32_t u[4]; bf16x8 v; } b;
                    w8_cvt4(ks == 0 ? q4.x : q4.z, b.u[0], b.u[1]);
                    w8_cvt4(ks == 0 ? q4.y : q4.w, b.u[2], b.u[3]);
#pragma unroll
                    for (int f = 0; f < MF; ++f)
                        acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            af[f], b.v, acc[f][n], 0, 0, 0);
                }
            }
            // the other buffer was last read before the previous barrier
            if (g + 1 < groups) MW8_STAGE((d + 1) % D, (d + 1) & 1);
            __syncthreads();
        }
    }
#undef MW8_LOAD
#undef MW8_STAGE

    // the channel scales of this lane's column in each of its fragments
    float cs[NFW];
#pragma unroll
    for (int n = 0; n < NFW; ++n)
        cs[n] = scale[(size_t)e * N + (frag0 + n) * 16 + (lane & 15)];

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
                    f2bf(mw8_silu(acc[f][0][r] * cs[0]) * (acc[f][1][r] * cs[1]));
            } else {
                const size_t col =
                    (size_t)blockIdx.y * BN + wave * 16 + (lane & 15);
                out[(size_t)pair * N + col] =
                    f2bf(rweights[pair] * (acc[f][0][r] * cs[0]));
            }
        }
}

template <int EPI>
hipError_t launch_w8_epi(int mf, dim3 grid, hipStream_t stream, bf16* out,
                         const bf16* a, const uint8_t* wq, const float* scale,
                         const int* sorted_pairs, const int* tile_expert,
                         const float* rweights, int N, int K, int k) {
#define MOE_W8_LAUNCH(MF)                                                      \
    moe_gemm_w8_kernel<MF, EPI, MW8_D><<<grid, MW8_THREADS, 0, stream>>>(      \
        out, a, wq, scale, sorted_pairs, tile_expert, rweights, N, K, k)
    switch (mf) {
        case 1: MOE_W8_LAUNCH(1); break;
        case 2: MOE_W8_LAUNCH(2); break;
        case 4: MOE_W8_LAUNCH(4); break;
        default: return hipErrorInvalidValue;  // no 128-row fp8 tile (mf = 8)
    }
#undef MOE_W8_LAUNCH
    HIP_CHECK_LAST();
    return hipSuccess;
}

}  // namespace

// epi 0: act [cap, N/2] = swiglu(gather(x) · dequant(w[e])^T), N = 2I, K = H
// epi 1: y_pair [P, N] = rweights · (act · dequant(w[e])^T),   N = H,  K = I
extern "C" hipError_t launch_moe_gemm_w8(
    void* out, const void* a, const void* wq, const float* scale,
    const int* sorted_pairs, const int* tile_expert, const float* rweights,
    int epi, int mf, int max_tiles, int N, int K, int k,
    hipStream_t stream) {
    if (max_tiles <= 0 || k < 1 || K <= 0 || K % MW8_GK != 0)
        return hipErrorInvalidValue;
    if (epi == EPI_SWIGLU) {
        if (N <= 0 || N % 128 != 0) return hipErrorInvalidValue;
        return launch_w8_epi<EPI_SWIGLU>(
            mf, dim3(max_tiles, N / 128), stream, (bf16*)out, (const bf16*)a,
            (const uint8_t*)wq, scale, sorted_pairs, tile_expert, rweights, N,
            K, k);
    }
    if (epi != EPI_DOWN || N <= 0 || N % 64 != 0) return hipErrorInvalidValue;
    return launch_w8_epi<EPI_DOWN>(
        mf, dim3(max_tiles, N / 64), stream, (bf16*)out, (const bf16*)a,
        (const uint8_t*)wq, scale, sorted_pairs, tile_expert, rweights, N, K,
        k);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
