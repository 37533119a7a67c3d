// Grouped expert GEMM for MoE prefill with MXFP4 expert weights (W4A16) on
// gfx950: the 128-row LDS-shared tile of moe_prefill.hip (mf = 8) on the
// resident panels of moe_w4.hip, unchanged, with the same moe_align plan, the
// same arguments and the same two epilogues.
//
// moe_gemm_w4<MF, EPI> is a decode kernel: 64 rows per tile at most, every
// wave converting its own weight fragments right before its MFMAs, so at
// ~1000 rows per expert an expert panel is re-read and re-converted once per
// 64 rows. Here a fragment is converted ONCE per workgroup and shared by the
// 128 rows of the tile through LDS.
//
// Geometry and MFMA schedule are moe_gemm_big's: tile 128 rows x 128 packed
// columns x k64, four waves 2 x 2 with 4 x 4 fragments of
// v_mfma_f32_16x16x32_bf16 each, grid (max_tiles, N / 128) with the row tile
// as the fast index, a ring of MQ_NBUF k64 slots of 16 KiB A + 16 KiB B,
// fragment reads as ds_read_b128 in inline assembly with their own lgkmcnt
// waits, one raw barrier per k-tile. A arrives by global_load_lds exactly as
// there (row gather in the DMA, bank XOR on the source chunk).
//
// The B stage is new. The LDS image of a slot's B half is the one
// moe_gemm_big reads: unit (k32 step ks, fragment f) is 1 KiB at
// (ks * 8 + f) * 1024, lane-linear, a lane's 16 bytes being its 8 bf16 of
// the 16x16x32 B fragment. A lane's 16 nibble bytes of a 128-k panel group
// hold exactly those 8 values for the group's four k32 steps, dword j for
// step j, so k-tile kt is dwords 2h, 2h + 1 (h = kt & 1) of group kt / 2:
//
// - load: wave w owns fragments 2w and 2w + 1 of the tile's eight. Per
//   k-tile it loads, for each, the 8-byte half of the lane's nibbles and the
//   column's scale dword (read again for the second half of the group: 64
//   bytes per fragment, from L2) into a register stage, together with the
//   tile's A DMA, MQ_NBUF - 1 k-tiles ahead of the MFMAs.
// - convert: two k-tiles later w4_cvt8 / w4_scale (exact) turn a dword into
//   the 16 bytes of bf16, and one ds_write_b128 per (ks, fragment) puts them
//   at lane * 16 of the unit. 8 fragments x 2 steps over 4 waves: every
//   fragment is converted once per workgroup. The VALU work of a unit is
//   issued between the MFMAs of the k32 step that runs meanwhile.
//
// The three hazards of staging B through registers into a DMA-fed ring:
//
// - vmcnt. The register loads count on vmcnt with the DMA, and vm loads
//   complete in order. Every wave issues per k-tile 4 register loads and
//   then 4 DMAs: MQ_GPW = 8 operations, constant, so mq_wait_ahead's "at
//   most n k-tiles in flight" is still vmcnt(8 n). The register loads are
//   inline assembly, so the compiler places no wait of its own for them; the
//   wait that hands a stage to the convert is mq_stage_wait, counted (the 4
//   DMAs of the same tile + 8 if a later tile is issued: vmcnt(12), or
//   vmcnt(4) for the last tile), with the stage registers as operands of the
//   statement right behind the wait so that no convert moves above it. The
//   two stages are named variables of a k-loop unrolled by two (K % 128 ==
//   0: the number of k-tiles is even), never indexed or rotated. The only
//   vmcnt(0) of the k-loop is the counted wait of the last k-tile, behind
//   which nothing is issued.
// - LDS writes. Written as C++ stores the compiler cannot tell them from the
//   words the DMA writes and would drain the ring with vmcnt(0); they are
//   ds_write_b128 in inline assembly. The mq_lds_wait (lgkmcnt(0)) in front
//   of every barrier covers them: they have landed before the barrier that
//   publishes the slot.
// - slot reuse. The barrier of k-tile kt says that every wave has read the
//   tiles up to kt. The A DMA of tile kt + 3 goes into the slot of tile
//   kt - 1 after that barrier (moe_gemm_big's rule); the B half of tile
//   kt + 1 is written during k-tile kt, before the barrier, into the slot
//   that held tile kt - 3, read by all before the barrier of kt - 3.
//
// Per output element the k32 steps are accumulated in ascending order by the
// same MFMA on the same bf16 values and the epilogue arithmetic is
// moe_gemm's, so the output is bit-identical to moe_gemm_big on the
// dequantised weights, and so to moe_gemm_w4<4, EPI>.
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
typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t u32x2;

constexpr int EPI_SWIGLU = 0;
constexpr int EPI_DOWN = 1;
constexpr int MQ_WAVES = 4;
constexpr int MQ_THREADS = MQ_WAVES * WAVE_SIZE;
constexpr int MQ_BM = 128;
constexpr int MQ_BN = 128;
constexpr int MQ_BK = 64;
constexpr int MQ_GK = 128;  // k of one panel group: two k-tiles
// ring depth as in moe_prefill.hip: 4 x 32 KiB = 128 KiB, one workgroup per CU
constexpr int MQ_NBUF = 4;
constexpr int MQ_AB = MQ_BM * MQ_BK * 2;  // bytes of a staged A tile
constexpr int MQ_BB = MQ_BK * MQ_BN * 2;  // bytes of a staged B tile
constexpr int MQ_BUFB = MQ_AB + MQ_BB;
constexpr int MQ_GPW = 8;  // vm operations per wave and k-tile: 4 B + 4 A
static_assert(MQ_AB == MQ_WAVES * 4 * 1024 && MQ_BB == MQ_WAVES * 4 * 1024,
              "every wave stages four 1-KiB units of each operand");
static_assert(MQ_NBUF == 4, "the stage waits count tiles kt + 1 .. kt + 2");

// the epilogue arithmetic of moe_gemm, to the bit
__device__ __forceinline__ float mq_silu(float g) {
    return g / (1.f + __expf(-g));
}

// async 16-byte-per-lane global -> LDS copy, see moe_prefill.hip
__device__ __forceinline__ void mq_glds16(const void* g, char* smem, int ldsoff) {
    ldsoff = __builtin_amdgcn_readfirstlane(ldsoff);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)g,
        (__attribute__((address_space(3))) void*)(smem + ldsoff), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void mq_vmwait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most `ahead` k-tiles of this wave's vm operations are still
// in flight (vmcnt immediates must be constants)
template <int A = 0>
__device__ __forceinline__ void mq_wait_ahead(int ahead) {
    if constexpr (A < MQ_NBUF - 1) {
        if (ahead == A) mq_vmwait<A * MQ_GPW>();
        else mq_wait_ahead<A + 1>(ahead);
    }
}

// compiler-only fence: keeps LDS accesses and vm issues on their side of a
// raw s_barrier
__device__ __forceinline__ void mq_cfence() { asm volatile("" ::: "memory"); }

// The register stage of one k-tile: for this wave's two fragments the lane's
// 8 nibble bytes (two k32 steps) and the column's scale dword of the group.
// Valid only after mq_stage_wait.
struct MqStage {
    u32x2 q0, q1;
    uint32_t s0, s1;
};

// q: this lane's 16 nibble bytes of fragment 0 of the group, + 8 for the
// second k-tile of the group; fragment 1 is 1 KiB further on. s: the scale
// dword of this lane's column of fragment 0; fragment 1 is 64 bytes on.
__device__ __forceinline__ void mq_stage_load(MqStage& st, const uint8_t* q,
                                              const uint8_t* s) {
    asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(st.q0) : "v"(q) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off offset:1024"
                 : "=&v"(st.q1) : "v"(q) : "memory");
    asm volatile("global_load_dword %0, %1, off" : "=v"(st.s0) : "v"(s) : "memory");
    asm volatile("global_load_dword %0, %1, off offset:64"
                 : "=v"(st.s1) : "v"(s) : "memory");
}

// Hands a stage to the convert: at most 4 + 8 `ahead` vm operations issued
// after the stage's loads (the 4 DMAs of its own tile and `ahead` later
// tiles) are in flight. The counted waits stand in the arms of a uniform
// branch without operands, so the stage registers meet no copy on the way
// from their loads; behind them the stage passes through an empty statement
// as operands. asm volatile statements keep their order, so no convert can
// be scheduled above the wait.
__device__ __forceinline__ void mq_stage_wait(MqStage& st, bool wait, int ahead) {
    if (wait) {
        if (ahead) mq_vmwait<4 + MQ_GPW>();
        else mq_vmwait<4>();
    }
    asm volatile(""
                 : "+v"(st.q0), "+v"(st.q1), "+v"(st.s0), "+v"(st.s1)
                 :
                 : "memory");
}

// One fragment: 16 bytes per lane at LDS byte address addr + OFF. The
// register is valid only after mq_lds_wait.
template <int OFF>
__device__ __forceinline__ bf16x8 mq_lds_read(unsigned addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2"
                 : "=v"(v)
                 : "v"(addr), "n"(OFF)
                 : "memory");
    return v;
}

// 16 converted bytes per lane to LDS byte address addr + OFF; landed after
// the next mq_lds_wait
template <int OFF>
__device__ __forceinline__ void mq_lds_write(unsigned addr, bf16x8 v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2"
                 :
                 : "v"(addr), "v"(v), "n"(OFF)
                 : "memory");
}

// the 4 A and 4 B fragments of k32 step KS of the k-tile, see moe_prefill.hip
template <int KS>
__device__ __forceinline__ void mq_lds_read_step(bf16x8 (&af)[4], bf16x8 (&bfr)[4],
                                                 unsigned a, unsigned b) {
    af[0] = mq_lds_read<0 * 16 * MQ_BK * 2>(a);
    af[1] = mq_lds_read<1 * 16 * MQ_BK * 2>(a);
    af[2] = mq_lds_read<2 * 16 * MQ_BK * 2>(a);
    af[3] = mq_lds_read<3 * 16 * MQ_BK * 2>(a);
    bfr[0] = mq_lds_read<(KS * 8 + 0) * 1024>(b);
    bfr[1] = mq_lds_read<(KS * 8 + 1) * 1024>(b);
    bfr[2] = mq_lds_read<(KS * 8 + 2) * 1024>(b);
    bfr[3] = mq_lds_read<(KS * 8 + 3) * 1024>(b);
}

// All LDS reads AND writes issued so far have landed. The fragments pass
// through as operands, so no MFMA that uses them can be scheduled above.
__device__ __forceinline__ void mq_lds_wait(bf16x8 (&af)[4], bf16x8 (&bfr)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(af[0]), "+v"(af[1]), "+v"(af[2]), "+v"(af[3]),
                   "+v"(bfr[0]), "+v"(bfr[1]), "+v"(bfr[2]), "+v"(bfr[3])
                 :
                 : "memory");
}

__device__ __forceinline__ f32x4 mq_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void mq_mfma_step(f32x4 (&acc)[4][4], const bf16x8 (&af)[4],
                                             const bf16x8 (&bfr)[4]) {
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[f][n] = mq_mfma(af[f], bfr[n], acc[f][n]);
}

// mq_mfma_step with the convert of a staged k-tile between the MFMAs: unit
// u = (k32 step u / 2, fragment u % 2) is converted behind the MFMAs of
// column u, at most four VALU operations per MFMA, pinned by scheduling
// barriers. H = the k-tile's half of its group: its k32 steps are dwords
// and scale bytes 2H, 2H + 1.
template <int H>
__device__ __forceinline__ void mq_mfma_cvt_step(
    f32x4 (&acc)[4][4], const bf16x8 (&af)[4], const bf16x8 (&bfr)[4],
    const MqStage& st, bf16x8 (&cv)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int ks = u >> 1;
        const u32x2 q2 = (u & 1) ? st.q1 : st.q0;
        const uint32_t s4 = (u & 1) ? st.s1 : st.s0;
        acc[0][u] = mq_mfma(af[0], bfr[u], acc[0][u]);
        const float scale = w4_scale((s4 >> (8 * (2 * H + ks))) & 0xffu);
        __builtin_amdgcn_sched_barrier(0);
        acc[1][u] = mq_mfma(af[1], bfr[u], acc[1][u]);
        union { uint32_t w[4]; bf16x8 v; } c;
        w4_cvt8(ks ? q2[1] : q2[0], scale, c.w);
        cv[u] = c.v;
        __builtin_amdgcn_sched_barrier(0);
        acc[2][u] = mq_mfma(af[2], bfr[u], acc[2][u]);
        acc[3][u] = mq_mfma(af[3], bfr[u], acc[3][u]);
        __builtin_amdgcn_sched_barrier(0);
    }
    // the converted units are needed HERE: without a use in this block the
    // converts sink into the conditional block of the ds_writes, behind the
    // MFMAs
    asm volatile("" : "+v"(cv[0]), "+v"(cv[1]), "+v"(cv[2]), "+v"(cv[3]));
}

// the four converted units of a k-tile into the B half of its slot; b = LDS
// address of this lane's 16 bytes of unit (0, this wave's fragment 0)
__device__ __forceinline__ void mq_lds_write_tile(unsigned b, const bf16x8 (&cv)[4]) {
    mq_lds_write<(0 * 8 + 0) * 1024>(b, cv[0]);
    mq_lds_write<(0 * 8 + 1) * 1024>(b, cv[1]);
    mq_lds_write<(1 * 8 + 0) * 1024>(b, cv[2]);
    mq_lds_write<(1 * 8 + 1) * 1024>(b, cv[3]);
}

// grid (max_tiles, N / 128). Arguments as moe_gemm_w4_kernel: out is act
// [cap, N/2] (SWIGLU) or y_pair [T·k, N] (DOWN); a is x [T, K] gathered by
// pair / k (SWIGLU) or act [cap, K] in sorted order (DOWN); wq is
// [E][K/128][N/16][64][16] nibble bytes, ws [E][K/128][N/16][16][4] scale
// bytes; sorted_pairs / tile_expert from moe_align at BM = 128.
template <int EPI>
__global__ __launch_bounds__(MQ_THREADS) void moe_gemm_w4_big_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ a,
    const uint8_t* __restrict__ wq, const uint8_t* __restrict__ ws,
    const int* __restrict__ sorted_pairs, const int* __restrict__ tile_expert,
    const float* __restrict__ rweights, int N, int K, int k) {
    __shared__ __attribute__((aligned(16))) char smem[MQ_NBUF * MQ_BUFB];
    __shared__ int pairs[MQ_BM];

    const int tile = blockIdx.x;
    const int e = tile_expert[tile];
    if (e < 0) return;  // uniform, before any barrier: an unused tile
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE_SIZE - 1);
    const int wave = tid >> 6;
    if (tid < MQ_BM) pairs[tid] = sorted_pairs[tile * MQ_BM + tid];
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
            src = EPI == EPI_SWIGLU ? (size_t)(pair / k) : (size_t)tile * MQ_BM + r;
        asrc[i] = a + src * K + (((lane & 7) ^ (lane >> 3)) << 3);
    }
    // B staging: this wave's fragments 2 wave, 2 wave + 1 of the tile's 8;
    // per group a fragment is 1 KiB of nibbles and 64 bytes of scales
    const size_t frag0 = (size_t)blockIdx.y * (MQ_BN / 16) + wave * 2;
    const size_t qstride = (size_t)N * (MQ_GK / 2);   // nibble bytes between groups
    const size_t sstride = (size_t)N * (MQ_GK / 32);  // scale bytes between groups
    const uint8_t* qsrc = wq + (size_t)e * N * (K / 2) + frag0 * 1024 + lane * 16;
    const uint8_t* ssrc = ws + (size_t)e * N * (K / 32) + frag0 * 64 + (lane & 15) * 4;
    const int udst = wave * 4 * 1024;  // this wave's A units

    // the vm operations of k-tile KT: 4 register loads, then 4 DMAs
#define MQ_ISSUE(KT, ST)                                                       \
    do {                                                                       \
        mq_stage_load(ST, qsrc + (size_t)((KT) >> 1) * qstride + ((KT) & 1) * 8, \
                      ssrc + (size_t)((KT) >> 1) * sstride);                   \
        char* buf__ = smem + ((KT) % MQ_NBUF) * MQ_BUFB;                       \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
            mq_glds16(asrc[i] + (size_t)(KT) * MQ_BK, buf__, udst + i * 1024); \
    } while (0)

    const int wm = wave >> 1;  // rows [64 wm, +64)
    const int wn = wave & 1;   // packed columns [64 wn, +64)
    f32x4 acc[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment reads as in moe_prefill.hip; bwr: where this wave's converted
    // units go
    const int arow = wm * 64 + (lane & 15);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned arow0 = lds0 + arow * (MQ_BK * 2);
    const unsigned aoff = arow0 + (((lane >> 4) ^ (arow & 7)) << 4);         // ks 0
    const unsigned aoff1 = arow0 + ((((lane >> 4) + 4) ^ (arow & 7)) << 4);  // ks 1
    const unsigned boff = lds0 + MQ_AB + wn * 4 * 1024 + lane * 16;
    const unsigned bwr = lds0 + MQ_AB + wave * 2 * 1024 + lane * 16;

    const int ktiles = K / MQ_BK;  // even, >= 2
    bf16x8 a0[4], b0[4], a1[4], b1[4], cv[4];
    MqStage st0, st1;  // the stages of the even and of the odd k-tiles

    // Prologue: tiles 0 .. 2 issued, tile 0 converted and published.
    MQ_ISSUE(0, st0);
    MQ_ISSUE(1, st1);
    mq_stage_wait(st0, true, 1);  // behind st0: its 4 DMAs and tile 1
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        union { uint32_t w[4]; bf16x8 v; } c;
        const u32x2 q2 = (u & 1) ? st0.q1 : st0.q0;
        const uint32_t s4 = (u & 1) ? st0.s1 : st0.s0;
        w4_cvt8((u >> 1) ? q2[1] : q2[0], w4_scale((s4 >> (8 * (u >> 1))) & 0xffu), c.w);
        cv[u] = c.v;
    }
    mq_lds_write_tile(bwr, cv);
    if (2 < ktiles) MQ_ISSUE(2, st0);
    mq_wait_ahead(min(ktiles - 1, MQ_NBUF - 2));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the converted units
    __builtin_amdgcn_s_barrier();  // every wave's share of tile 0 has landed
    mq_cfence();
    mq_lds_read_step<0>(a0, b0, aoff, boff);
    mq_lds_wait(a0, b0);

    // K-tile KT; NXT = the stage of tiles KT + 1 and KT + 3, H1 = (KT + 1) & 1.
    // Per output element the k32 steps are added in ascending order: step 0
    // of k-tile KT (fragments s0), then step 1 (fragments s1). While step 0
    // runs, tile KT + 1 is converted; behind the last tile the convert runs
    // on the stale stage (no wait, nothing written), so the MFMA step has
    // one form and the accumulators stay in place.
#define MQ_KTILE(KT, NXT, H1)                                                  \
    do {                                                                       \
        const int kt__ = (KT);                                                 \
        const bool more__ = kt__ + 1 < ktiles;                                 \
        const unsigned cur__ = (kt__ % MQ_NBUF) * MQ_BUFB;                     \
        const unsigned nxt__ = ((kt__ + 1) % MQ_NBUF) * MQ_BUFB;               \
        mq_lds_read_step<1>(a1, b1, aoff1 + cur__, boff + cur__);              \
        __builtin_amdgcn_sched_barrier(0);                                     \
        /* issued so far: tiles up to kt + 2 */                                \
        mq_stage_wait(NXT, more__, min(ktiles - 2 - kt__, 1));                 \
        /* step 1's fragments land meanwhile */                                \
        mq_mfma_cvt_step<H1>(acc, a0, b0, NXT, cv);                            \
        __builtin_amdgcn_sched_barrier(0);                                     \
        /* tile kt + 1's B half goes into the slot of tile kt - 3 */           \
        if (more__) mq_lds_write_tile(bwr + nxt__, cv);                        \
        mq_lds_wait(a1, b1); /* and the ds_writes above */                     \
        if (more__) {                                                          \
            mq_wait_ahead(min(ktiles - 2 - kt__, MQ_NBUF - 3));                \
            __builtin_amdgcn_s_barrier();                                      \
            mq_cfence();                                                       \
            /* tile kt + 1 has landed (A by DMA, B converted by every */       \
            /* wave), and every wave has read tile kt - 1, whose slot takes */ \
            /* the DMA of tile kt + 3; NXT was consumed above */               \
            if (kt__ + MQ_NBUF - 1 < ktiles) MQ_ISSUE(kt__ + MQ_NBUF - 1, NXT); \
            mq_lds_read_step<0>(a0, b0, aoff + nxt__, boff + nxt__);           \
        }                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                     \
        mq_mfma_step(acc, a1, b1); /* the next tile's step 0 lands meanwhile */ \
        __builtin_amdgcn_sched_barrier(0);                                     \
        mq_lds_wait(a0, b0);                                                   \
    } while (0)

    for (int kt = 0; kt < ktiles; kt += 2) {
        MQ_KTILE(kt, st1, 1);
        MQ_KTILE(kt + 1, st0, 0);
    }
#undef MQ_KTILE
#undef MQ_ISSUE

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
                    const size_t col = (size_t)blockIdx.y * (MQ_BN / 2) +
                                       (wn * 2 + j) * 16 + (lane & 15);
                    out[((size_t)tile * MQ_BM + rt) * (N / 2) + col] = f2bf(
                        mq_silu(acc[f][2 * j][r]) * acc[f][2 * j + 1][r]);
                }
            } else {
                const float rw = rweights[pair];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const size_t col = (size_t)blockIdx.y * MQ_BN +
                                       (wn * 4 + n) * 16 + (lane & 15);
                    out[(size_t)pair * N + col] = f2bf(rw * acc[f][n][r]);
                }
            }
        }
}

}  // namespace

// launch_moe_gemm_w4's mf = 8 (moe_w4.hip checks max_tiles and k).
// epi 0: N = 2I, K = H; epi 1: N = H, K = I; N % 128 == 0 and K % 128 == 0
// for both.
extern "C" hipError_t launch_moe_gemm_w4_big(
    void* out, const void* a, const void* wq, const void* ws,
    const int* sorted_pairs, const int* tile_expert, const float* rweights,
    int epi, int max_tiles, int N, int K, int k, hipStream_t stream) {
    if (max_tiles <= 0 || k < 1 || K <= 0 || K % MQ_GK != 0 || N <= 0 ||
        N % MQ_BN != 0)
        return hipErrorInvalidValue;
    const dim3 grid(max_tiles, N / MQ_BN);
    if (epi == EPI_SWIGLU)
        moe_gemm_w4_big_kernel<EPI_SWIGLU><<<grid, MQ_THREADS, 0, stream>>>(
            (bf16*)out, (const bf16*)a, (const uint8_t*)wq, (const uint8_t*)ws,
            sorted_pairs, tile_expert, rweights, N, K, k);
    else if (epi == EPI_DOWN && rweights != nullptr)
        moe_gemm_w4_big_kernel<EPI_DOWN><<<grid, MQ_THREADS, 0, stream>>>(
            (bf16*)out, (const bf16*)a, (const uint8_t*)wq, (const uint8_t*)ws,
            sorted_pairs, tile_expert, rweights, N, K, k);
    else
        return hipErrorInvalidValue;
    HIP_CHECK_LAST();
    return hipSuccess;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
