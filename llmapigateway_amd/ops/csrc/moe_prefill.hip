// Compute-bound grouped expert GEMM for MoE prefill on gfx950: the 128-row
// tile of moe.hip's moe_gemm<MF, EPI> (mf = 8), on the same packed expert
// weights, the same moe_align plan and with the same arguments.
//
// moe_gemm is built around the decode weight stream: row tiles of 64 rows at
// most, every wave pulling its own B fragments from HBM into registers. At
// ~1000 rows per expert that re-reads each expert panel 16 times through L2
// and runs at most 8 MFMAs per 2 KiB of B a wave loaded. This kernel shares
// both operands through LDS instead:
//
// - Tile BM = 128 rows x BN = 128 packed columns x BK = 64. Four waves in a
//   2 x 2 arrangement, each owning 64 x 64: 4 m-fragments x 4 n-fragments of
//   v_mfma_f32_16x16x32_bf16 (64 accumulator VGPRs), so every A and every B
//   fragment read from LDS feeds 4 MFMAs. For gate_up the 128 packed columns
//   are 64 act columns; the gate and up accumulators of an act column sit in
//   the same lane of adjacent n-fragments, as in moe_gemm.
// - Grid (max_tiles, N / 128) with the row tile as the fast index: the
//   workgroups resident at the same time share one column panel of an expert
//   in L2.
// - A and B are staged with global_load_lds (16 bytes per lane, no staging
//   VGPRs) into a ring of MB_NBUF k-tiles of 32 KiB (16 KiB A + 16 KiB B),
//   with counted vmcnt waits and raw barriers, the staging of gemm_m256.hip.
//   Every wave issues 4 A and 4 B loads per k-tile, so one count serves all
//   waves.
// - The fragment reads are ds_read_b128 in inline assembly with their own
//   lgkmcnt waits. Written as C++ loads the compiler cannot tell them from
//   the LDS words the DMA writes and puts s_waitcnt vmcnt(0) in front of the
//   first one, which drains the ring once per k-tile. With the reads in hand
//   the k-loop is software-pipelined with ONE barrier per k-tile: the
//   fragments of a k32 step land while the 16 MFMAs of the step before run,
//   across the barrier too. The barrier of k-tile kt says that tile kt + 1
//   has landed and that tile kt - 1 has been read by every wave, so its
//   buffer takes the DMA of tile kt + MB_NBUF - 1: MB_NBUF - 2 k-tiles stay
//   in flight across a barrier.
// - B: the 8 fragments of the tile for one k32 step are 8 KiB contiguous in
//   [E][K/32][N/16][64][8]: a straight copy, and the ds_read_b128 is
//   lane-linear.
// - A: the gather happens in the DMA. A lane supplies the source address of
//   one 16-byte chunk of its row (row pair / k of x, or row tile·BM + r of
//   act); the LDS destination is lane-linear, so moe_gemm's bank XOR
//   (chunk ^ (row & 7)) goes on the SOURCE chunk index. A padding row reads
//   row 0 of `a` (in bounds) and is never stored; an MFMA row never mixes
//   with another row, so nothing else depends on it.
//
// Per output element the k32 steps are accumulated in ascending order by the
// same MFMA and the epilogue arithmetic is moe_gemm's, so the output is
// bit-identical to moe_gemm<4, EPI> on the same pairs.

#include "common.h"

// see moe.hip: new kernels are compiled without the packed fp32 VALU forms
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int EPI_SWIGLU = 0;
constexpr int EPI_DOWN = 1;
constexpr int MB_WAVES = 4;
constexpr int MB_THREADS = MB_WAVES * WAVE_SIZE;
constexpr int MB_BM = 128;
constexpr int MB_BN = 128;
constexpr int MB_BK = 64;
// ring depth: MB_NBUF - 2 k-tiles of DMA in flight across a barrier. 4 x 32
// KiB = 128 KiB, one workgroup per CU (profiles/r14_moe_prefill.md)
constexpr int MB_NBUF = 4;
constexpr int MB_AB = MB_BM * MB_BK * 2;  // bytes of a staged A tile
constexpr int MB_BB = MB_BK * MB_BN * 2;  // bytes of a staged B tile
constexpr int MB_BUFB = MB_AB + MB_BB;
constexpr int MB_GPW = 8;  // global_load_lds per wave and k-tile: 4 A + 4 B
static_assert(MB_AB == MB_WAVES * 4 * 1024 && MB_BB == MB_WAVES * 4 * 1024,
              "every wave stages four 1-KiB units of each operand");

// the epilogue arithmetic of moe_gemm, to the bit
__device__ __forceinline__ float mb_silu(float g) {
    return g / (1.f + __expf(-g));
}

// async 16-byte-per-lane global -> LDS copy: the LDS destination is a
// wave-uniform base + lane * 16 (hardware rule), the global source is per
// lane. The base is uniform in fact (it depends on the wave id only) but not
// provably so to the compiler, hence the readfirstlane.
__device__ __forceinline__ void mb_glds16(const void* g, char* smem, int ldsoff) {
    ldsoff = __builtin_amdgcn_readfirstlane(ldsoff);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)g,
        (__attribute__((address_space(3))) void*)(smem + ldsoff), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void mb_vmwait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most `ahead` k-tiles of this wave's DMA are still in flight
// (vmcnt immediates must be constants)
template <int A = 0>
__device__ __forceinline__ void mb_wait_ahead(int ahead) {
    if constexpr (A < MB_NBUF - 1) {
        if (ahead == A) mb_vmwait<A * MB_GPW>();
        else mb_wait_ahead<A + 1>(ahead);
    }
}

// compiler-only fence: keeps LDS reads and DMA issues on their side of a raw
// s_barrier
__device__ __forceinline__ void mb_cfence() { asm volatile("" ::: "memory"); }

// One fragment: 16 bytes per lane at LDS byte address addr + OFF. The
// register is valid only after mb_lds_wait.
template <int OFF>
__device__ __forceinline__ bf16x8 mb_lds_read(unsigned addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2"
                 : "=v"(v)
                 : "v"(addr), "n"(OFF)
                 : "memory");
    return v;
}

// the 4 A and 4 B fragments of k32 step KS of the k-tile at LDS address
// `buf`: a = buf-relative address of this lane's chunk of fragment row 0,
// b = of its 16 bytes of B fragment (0, 4 wn)
template <int KS>
__device__ __forceinline__ void mb_lds_read_step(bf16x8 (&af)[4], bf16x8 (&bfr)[4],
                                                 unsigned a, unsigned b) {
    af[0] = mb_lds_read<0 * 16 * MB_BK * 2>(a);
    af[1] = mb_lds_read<1 * 16 * MB_BK * 2>(a);
    af[2] = mb_lds_read<2 * 16 * MB_BK * 2>(a);
    af[3] = mb_lds_read<3 * 16 * MB_BK * 2>(a);
    bfr[0] = mb_lds_read<(KS * 8 + 0) * 1024>(b);
    bfr[1] = mb_lds_read<(KS * 8 + 1) * 1024>(b);
    bfr[2] = mb_lds_read<(KS * 8 + 2) * 1024>(b);
    bfr[3] = mb_lds_read<(KS * 8 + 3) * 1024>(b);
}

// All LDS reads issued so far have landed. The fragments pass through as
// operands, so no MFMA that uses them can be scheduled above the wait.
__device__ __forceinline__ void mb_lds_wait(bf16x8 (&af)[4], bf16x8 (&bfr)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(af[0]), "+v"(af[1]), "+v"(af[2]), "+v"(af[3]),
                   "+v"(bfr[0]), "+v"(bfr[1]), "+v"(bfr[2]), "+v"(bfr[3])
                 :
                 : "memory");
}

__device__ __forceinline__ void mb_mfma_step(f32x4 (&acc)[4][4], const bf16x8 (&af)[4],
                                             const bf16x8 (&bfr)[4]) {
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int f = 0; f < 4; ++f)
            acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[f], bfr[n], acc[f][n], 0, 0, 0);
}

// grid (max_tiles, N / 128). Arguments as moe_gemm_kernel: out is act
// [cap, N/2] (SWIGLU) or y_pair [T·k, N] (DOWN); a is x [T, K] gathered by
// pair / k (SWIGLU) or act [cap, K] in sorted order (DOWN); w is
// [E][K/32][N/16][64][8]; sorted_pairs / tile_expert from moe_align at
// BM = 128.
template <int EPI>
__global__ __launch_bounds__(MB_THREADS) void moe_gemm_big_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ a,
    const bf16* __restrict__ w, const int* __restrict__ sorted_pairs,
    const int* __restrict__ tile_expert, const float* __restrict__ rweights,
    int N, int K, int k) {
    __shared__ __attribute__((aligned(16))) char smem[MB_NBUF * MB_BUFB];
    __shared__ int pairs[MB_BM];

    const int tile = blockIdx.x;
    const int e = tile_expert[tile];
    if (e < 0) return;  // uniform, before any barrier: an unused tile
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE_SIZE - 1);
    const int wave = tid >> 6;
    if (tid < MB_BM) pairs[tid] = sorted_pairs[tile * MB_BM + tid];
    __syncthreads();

    // A staging: unit u = 4 wave + i covers LDS rows [8u, 8u + 8); lane ->
    // row 8u + lane / 8, LDS chunk lane % 8, which receives the source chunk
    // (lane % 8) ^ (row & 7) (row & 7 == lane / 8)
    const bf16* asrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + (lane >> 3);
        const int pair = pairs[r];
        size_t src = 0;
        if (pair >= 0)
            src = EPI == EPI_SWIGLU ? (size_t)(pair / k) : (size_t)tile * MB_BM + r;
        asrc[i] = a + src * K + (((lane & 7) ^ (lane >> 3)) << 3);
    }
    // B staging: unit u = 4 wave + j is fragment u % 8 of k32 step u / 8 of
    // the k-tile, 1 KiB contiguous; a k32 step is N * 32 elements further on
    const size_t kstride = (size_t)N * 32;
    const bf16* bsrc = w + (size_t)e * N * K + (size_t)(wave >> 1) * kstride +
                       ((size_t)blockIdx.y * (MB_BN / 16) + (wave & 1) * 4) * 512 +
                       lane * 8;
    const int udst = wave * 4 * 1024;  // this wave's units within A and within B

#define MB_STAGE(KT)                                                           \
    do {                                                                       \
        char* buf__ = smem + ((KT) % MB_NBUF) * MB_BUFB;                       \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
            mb_glds16(asrc[i] + (size_t)(KT) * MB_BK, buf__, udst + i * 1024); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
            mb_glds16(bsrc + (size_t)(KT) * 2 * kstride + j * 512, buf__,      \
                      MB_AB + udst + j * 1024);                                \
    } while (0)

    const int wm = wave >> 1;  // rows [64 wm, +64)
    const int wn = wave & 1;   // packed columns [64 wn, +64)
    f32x4 acc[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment reads: A row 64 wm + 16 f + lane % 16, k-chunk 4 ks + lane / 16
    // at LDS chunk (k-chunk ^ (row & 7)); B fragment (ks, 4 wn + n) is
    // lane-linear
    const int arow = wm * 64 + (lane & 15);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned arow0 = lds0 + arow * (MB_BK * 2);
    const unsigned aoff = arow0 + (((lane >> 4) ^ (arow & 7)) << 4);         // ks 0
    const unsigned aoff1 = arow0 + ((((lane >> 4) + 4) ^ (arow & 7)) << 4);  // ks 1
    const unsigned boff = lds0 + MB_AB + wn * 4 * 1024 + lane * 16;

    // Per output element the k32 steps are added in ascending order: step 0
    // of k-tile kt (fragments s0), then step 1 (fragments s1).
    const int ktiles = K / MB_BK;
    bf16x8 a0[4], b0[4], a1[4], b1[4];
#pragma unroll
    for (int p = 0; p < MB_NBUF - 1; ++p)
        if (p < ktiles) MB_STAGE(p);
    mb_wait_ahead(min(ktiles - 1, MB_NBUF - 2));
    __builtin_amdgcn_s_barrier();  // every wave's share of tile 0 has landed
    mb_cfence();
    mb_lds_read_step<0>(a0, b0, aoff, boff);
    mb_lds_wait(a0, b0);
    for (int kt = 0; kt < ktiles; ++kt) {
        const unsigned cur = (kt % MB_NBUF) * MB_BUFB;
        mb_lds_read_step<1>(a1, b1, aoff1 + cur, boff + cur);
        __builtin_amdgcn_sched_barrier(0);
        mb_mfma_step(acc, a0, b0);  // step 1's fragments land meanwhile
        __builtin_amdgcn_sched_barrier(0);
        mb_lds_wait(a1, b1);
        if (kt + 1 < ktiles) {
            // DMA issued so far: tiles up to kt + MB_NBUF - 2
            mb_wait_ahead(min(ktiles - 2 - kt, MB_NBUF - 3));
            __builtin_amdgcn_s_barrier();
            mb_cfence();
            // tile kt + 1 has landed, and every wave has read tile kt - 1,
            // whose buffer is refilled here
            if (kt + MB_NBUF - 1 < ktiles) MB_STAGE(kt + MB_NBUF - 1);
            const unsigned nxt = ((kt + 1) % MB_NBUF) * MB_BUFB;
            mb_lds_read_step<0>(a0, b0, aoff + nxt, boff + nxt);
        }
        __builtin_amdgcn_sched_barrier(0);
        mb_mfma_step(acc, a1, b1);  // the next tile's step 0 lands meanwhile
        __builtin_amdgcn_sched_barrier(0);
        mb_lds_wait(a0, b0);
    }
#undef MB_STAGE

    // C fragment: row 4 (lane / 16) + r, column lane % 16
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rt = wm * 64 + f * 16 + (lane >> 4) * 4 + r;
            const int pair = pairs[rt];
            if (pair < 0) continue;
            if constexpr (EPI == EPI_SWIGLU) {
                // fragment 2j is the gate, 2j + 1 the up half of the same 16
                // act columns (block-16 interleave)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const size_t col = (size_t)blockIdx.y * (MB_BN / 2) +
                                       (wn * 2 + j) * 16 + (lane & 15);
                    out[((size_t)tile * MB_BM + rt) * (N / 2) + col] = f2bf(
                        mb_silu(acc[f][2 * j][r]) * acc[f][2 * j + 1][r]);
                }
            } else {
                const float rw = rweights[pair];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const size_t col = (size_t)blockIdx.y * MB_BN +
                                       (wn * 4 + n) * 16 + (lane & 15);
                    out[(size_t)pair * N + col] = f2bf(rw * acc[f][n][r]);
                }
            }
        }
}

}  // namespace

// launch_moe_gemm's mf = 8 (moe.hip checks max_tiles, k and the epilogue).
// epi 0: N = 2I, K = H; epi 1: N = H, K = I; N % 128 == 0 and K % 64 == 0
// for both.
extern "C" hipError_t launch_moe_gemm_big(
    void* out, const void* a, const void* w, const int* sorted_pairs,
    const int* tile_expert, const float* rweights, int epi, int max_tiles,
    int N, int K, int k, hipStream_t stream) {
    if (max_tiles <= 0 || k < 1 || K <= 0 || K % MB_BK != 0 || N <= 0 ||
        N % MB_BN != 0)
        return hipErrorInvalidValue;
    const dim3 grid(max_tiles, N / MB_BN);
    if (epi == EPI_SWIGLU)
        moe_gemm_big_kernel<EPI_SWIGLU><<<grid, MB_THREADS, 0, stream>>>(
            (bf16*)out, (const bf16*)a, (const bf16*)w, sorted_pairs,
            tile_expert, rweights, N, K, k);
    else if (epi == EPI_DOWN && rweights != nullptr)
        moe_gemm_big_kernel<EPI_DOWN><<<grid, MB_THREADS, 0, stream>>>(
            (bf16*)out, (const bf16*)a, (const bf16*)w, sorted_pairs,
            tile_expert, rweights, N, K, k);
    else
        return hipErrorInvalidValue;
    HIP_CHECK_LAST();
    return hipSuccess;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
