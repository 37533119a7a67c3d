// The skinny-M weight-streaming GEMM pipeline for gfx950, written once:
//   Y[M,N] = X[M,K] · W[N,K]^T, X bf16, fp32 accumulation, M <= 256.
// gemm_skinny.hip (bf16 weights, row-major or k-major), gemm_w8.hip (fp8
// e4m3 weights) and gemm_w4.hip (MXFP4 weights) instantiate it with a
// B-operand policy each.
//
// - grid = (N/64 n-stripes) x (split-K slices). One workgroup owns ALL M
//   rows of a 64-wide N stripe for its K-slice, so W is streamed exactly
//   once and the X re-read factor is only N/64 (X lives in the per-XCD L2s).
// - up to 8 waves; wave w owns M rows [w*16*MF, ..): MF m-fragments x 4
//   n-fragments of v_mfma_f32_16x16x32_bf16. All fragments are 16 B loads
//   straight from global (W from HBM, X from L2).
// - depth-4 software pipeline over k-steps of B::KSTEP (32 or 64), held in
//   shape by sched_barriers (profiles/r01_gemm_skinny_probe.md has the
//   measured history). Without pipelining ~70% of wave cycles park on the
//   ~900-cycle HBM latency of the W stream (measured SQ_WAIT_ANY).
// - no atomics: every workgroup fully writes the [M x 64] stripe it owns, of
//   y or (split-K) of the private fp32 slab blockIdx.y — a slice with no
//   k-steps writes zeros. launch_splitk_tail reduces the slabs.
//
// A policy B supplies only what differs between weight layouts:
//   KSTEP                  k-depth of one pipeline step (KSTEP/32 MFMAs per
//                          accumulator, issued in increasing k)
//   Regs                   one step's B registers for the stripe
//   init(w, aux, N, K, n0, k0, lane)   point at the slice's first step
//   load(regs, S)          issue the loads of step S (relative)
//   bump(steps)            advance
//   frag(regs, n, h)       MFMA B fragment of n-fragment n, k32 half h
//   SCALED                 multiply the accumulator by scale[col] before
//                          the store
// aux is the launch's second weight operand: the fp32 channel scales of a
// SCALED policy, or whatever else a policy streams beside w (gemm_w4.hip:
// the e8m0 block scales); a policy that needs none ignores it.
#pragma once

#include "common.h"

#define GS_MAX_M 256
#define GS_NF 4             // 16-col n-fragments per stripe
#define GS_NT (GS_NF * 16)  // stripe width = 64 columns

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t u32x4;

__device__ __forceinline__ f32x4 gs_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 16-B load through an explicit global (addrspace 1) pointer: loop-carried
// generic pointers defeat the compiler's addrspace inference and demote
// these to flat_load (which drains lgkmcnt as well — serializing the
// software pipeline into load -> full drain -> mfma).
// NOTE: nt loads on W measured 20-40% SLOWER for row-major bf16: each 128 B
// line spans two k-steps of a row, and nt drops the line before the second
// 64 B hit, doubling the W fetch traffic.
template <class V>
__device__ __forceinline__ V gs_gload(const void* p) {
    return *(const __attribute__((address_space(1))) V*)(unsigned long long)p;
}

// scheduling fence: keep the software-pipeline shape — without it the
// scheduler compresses the depth-4 pipeline back to serial loads (84
// VGPRs observed) and the kernel runs latency-bound
#define GS_FENCE __builtin_amdgcn_sched_barrier(0)

// blockDim = nwaves*64 with nwaves = ceil(M / (16*MF)) <= 8; MF in {1, 2}
// covers M <= 256 (deeper MF spills at this pipeline depth).
template <class B, int MF, bool SPLITK>
__launch_bounds__(8 * WAVE_SIZE)
__global__ void gemm_stream_kernel(
    bf16* __restrict__ y,            // [M, N] (!SPLITK)
    float* __restrict__ yw,          // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,      // [M, K]
    const void* __restrict__ w,      // the policy's weight layout
    const void* __restrict__ aux,    // [N] fp32 scales (B::SCALED) / policy's own
    int M,
    int N,
    int K,
    int nsk) {
    constexpr int KS = B::KSTEP;
    constexpr int KF = KS / 32;  // MFMA k-steps per pipeline step
    const int n0 = blockIdx.x * GS_NT;
    const int kslice = ((K / KS + nsk - 1) / nsk) * KS;
    const int k0 = (SPLITK ? blockIdx.y : 0) * kslice;
    const int k1 = min(K, k0 + kslice);

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x >> 6;
    const int lrow = lane & 15;  // A row / B col within a fragment
    const int lk = lane >> 4;    // k-group of 8 bf16

    const int m_base = wave * (MF * 16);

    f32x4 acc[MF][GS_NF];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int n = 0; n < GS_NF; ++n) acc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bf16* ap[MF];  // rows past M re-read row 0; never stored
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int r = m_base + f * 16 + lrow;
        ap[f] = x + (size_t)(r < M ? r : 0) * K + k0 + lk * 8;
    }
    B bp;
    bp.init(w, aux, N, K, n0, k0, lane);

    const int nsteps = (k1 - k0) / KS;  // K and kslice are KS-aligned
    if (nsteps > 0 && m_base < M) {
        // One register set per pipeline stage: the A fragments and the B
        // registers of one k-step. Four explicit sets, every index
        // compile-time: a [d][..] array indexed by a runtime phase demotes
        // to scratch.
        struct Set {
            bf16x8 a[MF * KF];
            typename B::Regs b;
        };
        Set s0, s1, s2, s3;
        auto load = [&](Set& st, int S) {
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int h = 0; h < KF; ++h)
                    st.a[f * KF + h] = gs_gload<bf16x8>(ap[f] + S * KS + h * 32);
            bp.load(st.b, S);
        };
        auto mfma = [&](const Set& st) {
#pragma unroll
            for (int n = 0; n < GS_NF; ++n) {
                bf16x8 b[KF];
#pragma unroll
                for (int h = 0; h < KF; ++h) b[h] = B::frag(st.b, n, h);
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int h = 0; h < KF; ++h)
                        acc[f][n] = gs_mfma(st.a[f * KF + h], b[h], acc[f][n]);
            }
        };
        auto bump = [&](int steps) {
#pragma unroll
            for (int f = 0; f < MF; ++f) ap[f] += steps * KS;
            bp.bump(steps);
        };

        if (nsteps < 3) {
            for (int s = 0; s < nsteps; ++s) {
                load(s0, 0);
                mfma(s0);
                bump(1);
            }
        } else {
            load(s0, 0);
            load(s1, 1);
            load(s2, 2);
            int s = 0;
            for (; s + 7 <= nsteps; s += 4) {  // prefetches reach s+6
                load(s3, 3);
                GS_FENCE;
                mfma(s0);
                GS_FENCE;
                load(s0, 4);
                GS_FENCE;
                mfma(s1);
                GS_FENCE;
                load(s1, 5);
                GS_FENCE;
                mfma(s2);
                GS_FENCE;
                load(s2, 6);
                GS_FENCE;
                mfma(s3);
                bump(4);
            }
            // tail: r in [3,6]; s0/s1/s2 hold steps s, s+1, s+2
            const int r = nsteps - s;
            if (r >= 4) load(s3, 3);
            mfma(s0);
            if (r >= 5) load(s0, 4);
            mfma(s1);
            if (r >= 6) load(s1, 5);
            mfma(s2);
            if (r >= 4) mfma(s3);
            if (r >= 5) mfma(s0);
            if (r >= 6) mfma(s1);
        }
    }

    // ---- epilogue: C fragment row = lk*4 + r, col = lrow; a channel scale
    // goes onto the fp32 accumulator before any store, so split-K slabs
    // hold finished partial sums ----
    float sc[GS_NF];
#pragma unroll
    for (int n = 0; n < GS_NF; ++n)
        sc[n] = B::SCALED ? ((const float*)aux)[n0 + n * 16 + lrow] : 1.f;
    float* slab = yw + (size_t)(SPLITK ? blockIdx.y : 0) * M * N;
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m_base + f * 16 + lk * 4 + r;
            if (row >= M) continue;
#pragma unroll
            for (int n = 0; n < GS_NF; ++n) {
                const float v = B::SCALED ? acc[f][n][r] * sc[n] : acc[f][n][r];
                const size_t at = (size_t)row * N + n0 + n * 16 + lrow;
                if (SPLITK) slab[at] = v;
                else y[at] = f2bf(v);
            }
        }
}

// Launch for M <= GS_MAX_M; the caller has validated the shape for B.
template <class B>
static hipError_t launch_gemm_stream(
    void* y, float* workspace, const void* x, const void* w,
    const void* aux, int M, int N, int K, int nsk, hipStream_t stream) {
    // prefer more waves over more rows per wave: MF=1 up to 8 waves (M <= 128)
    const int mf = M > 128 ? 2 : 1;
    dim3 grid(N / GS_NT, nsk);
    dim3 block(ceil_div_i(M, 16 * mf) * WAVE_SIZE);
#define GS_LAUNCH(MFV, SPLIT)                                                  \
    gemm_stream_kernel<B, MFV, SPLIT><<<grid, block, 0, stream>>>(             \
        (bf16*)y, workspace, (const bf16*)x, w, aux, M, N, K, nsk)
    if (nsk == 1) {
        if (mf == 1) GS_LAUNCH(1, false);
        else GS_LAUNCH(2, false);
    } else {
        if (mf == 1) GS_LAUNCH(1, true);
        else GS_LAUNCH(2, true);
    }
#undef GS_LAUNCH
    HIP_CHECK_LAST();
    return hipSuccess;
}
