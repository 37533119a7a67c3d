// Skinny-M streaming GEMM for gfx950: Y[M,N] = X[M,K] · W[N,K]^T, bf16.
//
// The decode-step projections (M = batch ≤ 256, W up to 0.5 GB/layer) are
// weight-stream-bound: ideal time is W-bytes / HBM-rate. rocBLAS/hipBLASLt
// run these 3-4x off that bound at skinny M (measured via TunableOp
// cold-cache sweep: down-proj 4096x256x14336 at 66 us vs the ~15 us
// stream bound). This kernel streams W exactly ONCE:
//
// - grid = (N/64 n-stripes) x (split-K slices). One workgroup owns ALL M
//   rows of a 64-wide N stripe for its K-slice, so W is never re-read and
//   the X re-read factor is only N/64 (X lives in the per-XCD L2s).
// - up to 8 waves; wave w owns M rows [w*16*MF, ..): MF m-fragments x
//   NF=4 n-fragments of v_mfma_f32_16x16x32_bf16 per 32-deep k-step. All
//   fragments are 16 B dwordx4 loads straight from global (B/W coalesced
//   by 16 rows x 64 B, or fully contiguous with the opt-in k-major
//   swizzle; A/X from L2).
// - software pipeline up to depth 4, held in shape by sched_barriers
//   (see profiles/r01_gemm_skinny_probe.md for the measured history).
//   Production dispatch is the latency regime (M <= 16, ops/__init__.py);
//   the tuned library keeps M >= 64 (its LDS macro-tiles re-read X less).
// - split-K writes private fp32 slabs (each workgroup fully writes its
//   [M x 64] stripe of slab blockIdx.y — no zero-fill, no atomics, no
//   cross-workgroup visibility hazard); a second tiny kernel reduces the
//   slabs to bf16. Both launches are hipGraph-capturable (static scratch).
//
// Replaces F.linear on the decode hot path (models/llama.py) for
// M <= GS_MAX_M and N <= 28672; prefill, lm_head and big-M stay on the
// TunableOp-tuned library GEMMs.

#include "common.h"

#define GS_MAX_M 256
#define GS_WAVES 4
#define GS_NF 4                    // 16-col n-fragments per stripe
#define GS_NT (GS_NF * 16)         // stripe width = 64 columns

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

__device__ __forceinline__ f32x4 gs_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 16-B load through an explicit global (addrspace 1) pointer: loop-carried
// generic pointers defeat the compiler's addrspace inference and demote
// these to flat_load (which drains lgkmcnt as well — serializing the
// software pipeline into load -> full drain -> mfma).
__device__ __forceinline__ bf16x8 gs_gload(const bf16* p) {
    return *(const __attribute__((address_space(1))) bf16x8*)(unsigned long long)p;
}

// NOTE: nt loads on W measured 20-40% SLOWER here: each 128 B line spans
// two k-steps of a row, and nt drops the line before the second 64 B hit,
// doubling the W fetch traffic.

// scheduling fence: keep the software-pipeline shape — without it the
// scheduler compresses the depth-4 pipeline back to serial loads (84
// VGPRs observed) and the kernel runs latency-bound
#define GS_FENCE __builtin_amdgcn_sched_barrier(0)

// blockDim = nwaves*64 with nwaves = ceil(M / (16*MF)) (<= 8): MF=2 with 8
// waves covers M=256 while the register-feasible depth-4 pipeline applies.
// SWZ: W is pre-swizzled k-major ([K/32, N, 32]) so every B-fragment load
// is part of a contiguous 4 KB (64-row x 64 B) stream per k-step —
// the [N, K] row-major layout reads 16 rows x 64 B per instruction and
// caps at ~3.5 TB/s effective.
template <int MF, bool SPLITK, bool SWZ>
__launch_bounds__(8 * WAVE_SIZE)
__global__ void gemm_skinny_kernel(
    bf16* __restrict__ y,        // [M, N] (!SPLITK)
    float* __restrict__ yw,      // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,  // [M, K]
    const bf16* __restrict__ w,  // [N, K] or swizzled [K/32, N, 32]
    int M,
    int N,
    int K,
    int nsk) {
    const int n0 = blockIdx.x * GS_NT;
    const int kslice = ((K / 32 + nsk - 1) / nsk) * 32;
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

    const bf16* ap[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int r = m_base + f * 16 + lrow;
        ap[f] = x + (size_t)(r < M ? r : 0) * K + k0 + lk * 8;
    }
    // B pointers: row-major [N, K] strides K per n-row and 32 per k-step;
    // swizzled [K/32, N, 32] strides 32 per n-row and 32*N per k-step
    const size_t bstep = SWZ ? (size_t)32 * N : 32;  // elems per k-step
    const bf16* bp[GS_NF];
#pragma unroll
    for (int n = 0; n < GS_NF; ++n)
        bp[n] = SWZ
                    ? w + (size_t)(k0 / 32) * N * 32 +
                          (size_t)(n0 + n * 16 + lrow) * 32 + lk * 8
                    : w + (size_t)(n0 + n * 16 + lrow) * K + k0 + lk * 8;

    const int nsteps = (k1 - k0) / 32;  // K and kslice are 32-aligned
    if (nsteps > 0 && m_base < M) {
        // Explicit buffer sets, all indices compile-time (a [d][..] array
        // indexed by a runtime phase demotes to scratch; depth 4 at MF=4
        // spilled to 280 VGPRs = 1 wave/SIMD). Without pipelining, ~70%
        // of wave cycles park on the ~900-cycle HBM latency of the W
        // stream (measured SQ_WAIT_ANY).
        bf16x8 a0[MF], b0[GS_NF], a1[MF], b1[GS_NF];
        bf16x8 a2[MF], b2[GS_NF], a3[MF], b3[GS_NF];
#define GS_LOAD(AV, BV, S)                                                     \
    do {                                                                       \
        _Pragma("unroll") for (int f = 0; f < MF; ++f) AV[f] =                 \
            gs_gload(ap[f] + (S) * 32);                                        \
        _Pragma("unroll") for (int n = 0; n < GS_NF; ++n) BV[n] =              \
            gs_gload(bp[n] + (S) * (SWZ ? bstep : 32));                        \
    } while (0)
#define GS_MFMA_ALL(AV, BV)                                                    \
    do {                                                                       \
        _Pragma("unroll") for (int n = 0; n < GS_NF; ++n)                      \
            _Pragma("unroll") for (int f = 0; f < MF; ++f) acc[f][n] =         \
                gs_mfma(AV[f], BV[n], acc[f][n]);                              \
    } while (0)
#define GS_BUMP(STEPS)                                                         \
    do {                                                                       \
        _Pragma("unroll") for (int f = 0; f < MF; ++f) ap[f] += (STEPS) * 32;  \
        _Pragma("unroll") for (int n = 0; n < GS_NF; ++n)                      \
            bp[n] += (STEPS) * (SWZ ? bstep : 32);                             \
    } while (0)
        if constexpr (MF <= 2) {
            // depth-4 pipeline: fits registers at MF<=2 and fully covers
            // HBM latency (small-M decode: latency matters most there)
            if (nsteps < 3) {
                for (int s = 0; s < nsteps; ++s) {
                    GS_LOAD(a0, b0, 0);
                    GS_MFMA_ALL(a0, b0);
                    GS_BUMP(1);
                }
            } else {
                GS_LOAD(a0, b0, 0);
                GS_LOAD(a1, b1, 1);
                GS_LOAD(a2, b2, 2);
                int s = 0;
                for (; s + 7 <= nsteps; s += 4) {  // prefetches reach s+6
                    GS_LOAD(a3, b3, 3);
                    GS_FENCE;
                    GS_MFMA_ALL(a0, b0);
                    GS_FENCE;
                    GS_LOAD(a0, b0, 4);
                    GS_FENCE;
                    GS_MFMA_ALL(a1, b1);
                    GS_FENCE;
                    GS_LOAD(a1, b1, 5);
                    GS_FENCE;
                    GS_MFMA_ALL(a2, b2);
                    GS_FENCE;
                    GS_LOAD(a2, b2, 6);
                    GS_FENCE;
                    GS_MFMA_ALL(a3, b3);
                    GS_BUMP(4);
                }
                // tail: r in [3,6]; a0/a1/a2 hold steps s, s+1, s+2
                const int r = nsteps - s;
                if (r >= 4) GS_LOAD(a3, b3, 3);
                GS_MFMA_ALL(a0, b0);
                if (r >= 5) GS_LOAD(a0, b0, 4);
                GS_MFMA_ALL(a1, b1);
                if (r >= 6) GS_LOAD(a1, b1, 5);
                GS_MFMA_ALL(a2, b2);
                if (r >= 4) GS_MFMA_ALL(a3, b3);
                if (r >= 5) GS_MFMA_ALL(a0, b0);
                if (r >= 6) GS_MFMA_ALL(a1, b1);
            }
        } else {
            // depth-2 ping/pong: MF 3-4 spills at deeper pipelines
            GS_LOAD(a0, b0, 0);
            int s = 0;
            for (; s + 2 <= nsteps - 1; s += 2) {
                GS_LOAD(a1, b1, 1);
                GS_FENCE;
                GS_MFMA_ALL(a0, b0);
                GS_FENCE;
                GS_LOAD(a0, b0, 2);
                GS_FENCE;
                GS_MFMA_ALL(a1, b1);
                GS_BUMP(2);
            }
            if (nsteps - s == 2) {
                GS_LOAD(a1, b1, 1);
                GS_MFMA_ALL(a0, b0);
                GS_MFMA_ALL(a1, b1);
            } else {
                GS_MFMA_ALL(a0, b0);
            }
        }
#undef GS_LOAD
#undef GS_MFMA_ALL
#undef GS_BUMP
    }

    // ---- epilogue: C fragment row = lk*4 + r, col = lrow ----
    if (SPLITK) {
        float* slab = yw + (size_t)blockIdx.y * M * N;
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m_base + f * 16 + lk * 4 + r;
                if (row >= M) continue;
#pragma unroll
                for (int n = 0; n < GS_NF; ++n)
                    slab[(size_t)row * N + n0 + n * 16 + lrow] = acc[f][n][r];
            }
    } else {
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m_base + f * 16 + lk * 4 + r;
                if (row >= M) continue;
#pragma unroll
                for (int n = 0; n < GS_NF; ++n)
                    y[(size_t)row * N + n0 + n * 16 + lrow] = f2bf(acc[f][n][r]);
            }
    }
}

// sum the split-K fp32 slabs into bf16 y; float4-vectorized grid-stride
__global__ void gemm_skinny_reduce_kernel(
    bf16* __restrict__ y, const float* __restrict__ yw, int64_t mn, int nsk) {
    const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= mn) return;
    float4 s = *reinterpret_cast<const float4*>(yw + i4);
    for (int k = 1; k < nsk; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(yw + (int64_t)k * mn + i4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    uint2 packed;
    packed.x = pack2(s.x, s.y);
    packed.y = pack2(s.z, s.w);
    *reinterpret_cast<uint2*>(y + i4) = packed;
}

// standalone split-K slab reduction (shared with gemm_m256.hip)
extern "C" hipError_t launch_gemm_reduce(
    void* y, const float* yw, int64_t mn, int nsk, hipStream_t stream) {
    const int64_t thr = mn / 4;  // mn % 4 == 0 (N % 64 == 0)
    const int tpb = 256;
    gemm_skinny_reduce_kernel<<<dim3((thr + tpb - 1) / tpb), dim3(tpb), 0,
                                stream>>>((bf16*)y, yw, mn, nsk);
    HIP_CHECK_LAST();
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// Split-K reduce + residual add + RMSNorm in one pass (decode o/down
// projections): the reduce kernel above writes y only for the norm kernel
// to re-read it one launch later. Per element, in this order:
//   s = slab0 + slab1 + ...      (increasing k, as the reduce kernel)
//   y = bf16(s)                  (the rounding of the y no longer stored)
//   r = bf16(y + residual)       -> residual (in place)
//   out = bf16(r * inv * w),  inv = rsqrt(mean(r^2) + eps)
// so the residual stream is bit-identical to reduce + rmsnorm_residual.
//
// Sized for the slab stream (nsk*M*N*4 B — 33.5 MB for the 8B down-proj
// at M=256), not for the norm: one block of N/8 threads per row (8 waves
// at N=4096, where the wave-per-row norm had one), each thread owning one
// 8-element chunk — a fixed per-thread count, so the row cache and the
// slab batches stay in VGPRs. Slabs are loaded in batches of 4 so a
// batch's loads are all in flight before the adds.
//
// The sum of squares is reduced in the SAME order as the norm kernel this
// replaces (elementwise.hip), so `out` matches the unfused pair bit for
// bit too: r^2 is exact in fp32 (r is a bf16 value), the squares go
// through LDS, and P "virtual lanes" re-add them the way the norm
// kernel's lanes do — lane p takes chunks p, p+P, ... in sequence, then
// the 64-lane butterfly, then the per-wave totals in order. P = 64 is
// rmsnorm_wave_kernel (N <= 4096), P = 256 the block form rmsnorm_kernel.
// ---------------------------------------------------------------------------
#define RN_MAX_N 8192
#define RN_KB 4  // slabs per load batch

__launch_bounds__(RN_MAX_N / 8)
__global__ void gemm_reduce_rmsnorm_kernel(
    bf16* __restrict__ out,            // [M, N]
    bf16* __restrict__ residual,       // [M, N] updated in place
    const float* __restrict__ yw,      // [nsk, M, N] fp32 slabs
    const bf16* __restrict__ weight,   // [N]
    float eps, int M, int N, int nsk) {
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;  // == N / 8: one chunk per thread
    const int col = tid * 8;
    const size_t mn = (size_t)M * N;
    const float* src = yw + (size_t)row * N + col;
    bf16* rrow = residual + (size_t)row * N + col;

    float4 s[2];
    s[0] = *reinterpret_cast<const float4*>(src);
    s[1] = *reinterpret_cast<const float4*>(src + 4);
    const uint4 vr = *reinterpret_cast<const uint4*>(rrow);
    for (int k0 = 1; k0 < nsk; k0 += RN_KB) {
        float4 t[RN_KB][2];
#pragma unroll
        for (int kk = 0; kk < RN_KB; ++kk) {
            const bool on = k0 + kk < nsk;
            const float* p = src + (size_t)(on ? k0 + kk : 0) * mn;
            t[kk][0] = *reinterpret_cast<const float4*>(p);
            t[kk][1] = *reinterpret_cast<const float4*>(p + 4);
        }
#pragma unroll
        for (int kk = 0; kk < RN_KB; ++kk)
            if (k0 + kk < nsk) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    s[h].x += t[kk][h].x;
                    s[h].y += t[kk][h].y;
                    s[h].z += t[kk][h].z;
                    s[h].w += t[kk][h].w;
                }
            }
    }

    float f[8] = {s[0].x, s[0].y, s[0].z, s[0].w, s[1].x, s[1].y, s[1].z, s[1].w};
    float g[8];
    unpack2(vr.x, g[0], g[1]);
    unpack2(vr.y, g[2], g[3]);
    unpack2(vr.z, g[4], g[5]);
    unpack2(vr.w, g[6], g[7]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        // both roundings of the unfused pair: y to bf16, then y + residual
        f[j] = bfbits2f(f2bfbits(bfbits2f(f2bfbits(f[j])) + g[j]));
    uint4 pr;
    pr.x = pack2(f[0], f[1]);  // exact: already bf16 values
    pr.y = pack2(f[2], f[3]);
    pr.z = pack2(f[4], f[5]);
    pr.w = pack2(f[6], f[7]);
    *reinterpret_cast<uint4*>(rrow) = pr;

    __shared__ float4 sq[RN_MAX_N / 4];
    __shared__ float red[4];
    sq[tid * 2] = make_float4(f[0] * f[0], f[1] * f[1], f[2] * f[2], f[3] * f[3]);
    sq[tid * 2 + 1] = make_float4(f[4] * f[4], f[5] * f[5], f[6] * f[6], f[7] * f[7]);
    __syncthreads();
    const int P = N <= 4096 ? WAVE_SIZE : 256;  // the replaced kernel's lanes
    if (tid < P) {
        float ssq = 0.f;
        for (int c = tid; c < nthreads; c += P) {
            const float4 a = sq[c * 2], b = sq[c * 2 + 1];
            ssq += a.x; ssq += a.y; ssq += a.z; ssq += a.w;
            ssq += b.x; ssq += b.y; ssq += b.z; ssq += b.w;
        }
        const float wsum = wave_reduce_sum(ssq);
        if ((tid & (WAVE_SIZE - 1)) == 0) red[tid / WAVE_SIZE] = wsum;
    }
    __syncthreads();
    float total = red[0];
    if (P > WAVE_SIZE) total = 0.f + red[0] + red[1] + red[2] + red[3];
    const float inv = rsqrtf(total / (float)N + eps);

    const uint4 vw = *reinterpret_cast<const uint4*>(weight + col);
    float w8[8];
    unpack2(vw.x, w8[0], w8[1]);
    unpack2(vw.y, w8[2], w8[3]);
    unpack2(vw.z, w8[4], w8[5]);
    unpack2(vw.w, w8[6], w8[7]);
    uint4 vo;
    vo.x = pack2(f[0] * inv * w8[0], f[1] * inv * w8[1]);
    vo.y = pack2(f[2] * inv * w8[2], f[3] * inv * w8[3]);
    vo.z = pack2(f[4] * inv * w8[4], f[5] * inv * w8[5]);
    vo.w = pack2(f[6] * inv * w8[6], f[7] * inv * w8[7]);
    *reinterpret_cast<uint4*>(out + (size_t)row * N + col) = vo;
}

// shapes the fused reduce+norm covers (shared with gemm_m256.hip and
// mirrored by ops._reduce_norm_covers)
extern "C" int gemm_reduce_rmsnorm_covers(int N) {
    return N > 0 && N % 512 == 0 && N <= RN_MAX_N;
}

extern "C" hipError_t launch_gemm_reduce_rmsnorm(
    void* out, void* residual, const float* yw, const void* weight, float eps,
    int M, int N, int nsk, hipStream_t stream) {
    if (M <= 0 || nsk < 2 || !gemm_reduce_rmsnorm_covers(N))
        return hipErrorInvalidValue;
    gemm_reduce_rmsnorm_kernel<<<dim3(M), dim3(N / 8), 0, stream>>>(
        (bf16*)out, (bf16*)residual, yw, (const bf16*)weight, eps, M, N, nsk);
    HIP_CHECK_LAST();
    return hipSuccess;
}

extern "C" hipError_t launch_gemm_skinny(
    void* y, float* workspace, const void* x, const void* w, int M, int N,
    int K, int nsk, int swz, hipStream_t stream) {
    if (M <= 0 || M > GS_MAX_M) return hipErrorInvalidValue;
    if ((N % GS_NT) != 0 || (K % 32) != 0) return hipErrorInvalidValue;
    if (nsk < 1) return hipErrorInvalidValue;
    if (nsk > 1 && workspace == nullptr) return hipErrorInvalidValue;
    const int tiles = N / GS_NT;
    // smallest MF whose wave count fits 8 waves: deeper pipelines only fit
    // registers at MF<=2, so prefer more waves over more rows per wave
    int mf = 1;
    while (ceil_div_i(M, 16 * mf) > 8) mf *= 2;
    const int nwaves = ceil_div_i(M, 16 * mf);
    dim3 grid(tiles, nsk);
    dim3 block(nwaves * WAVE_SIZE);
#define GS_LAUNCH1(MFV, SPLIT, SWZV)                                           \
    gemm_skinny_kernel<MFV, SPLIT, SWZV><<<grid, block, 0, stream>>>(          \
        (bf16*)y, workspace, (const bf16*)x, (const bf16*)w, M, N, K, nsk)
#define GS_LAUNCH(MFV, SPLIT)                                                  \
    do {                                                                       \
        if (swz) GS_LAUNCH1(MFV, SPLIT, true);                                 \
        else GS_LAUNCH1(MFV, SPLIT, false);                                    \
    } while (0)
    if (nsk == 1) {
        switch (mf) {
            case 1: GS_LAUNCH(1, false); break;
            case 2: GS_LAUNCH(2, false); break;
            case 3: GS_LAUNCH(3, false); break;
            default: GS_LAUNCH(4, false); break;
        }
    } else {
        switch (mf) {
            case 1: GS_LAUNCH(1, true); break;
            case 2: GS_LAUNCH(2, true); break;
            case 3: GS_LAUNCH(3, true); break;
            default: GS_LAUNCH(4, true); break;
        }
        const int64_t mn = (int64_t)M * N;  // M*N % 4 == 0 (N % 64 == 0)
        const int64_t thr = mn / 4;
        const int tpb = 256;
        gemm_skinny_reduce_kernel<<<dim3((thr + tpb - 1) / tpb), dim3(tpb), 0,
                                    stream>>>((bf16*)y, workspace, mn, nsk);
    }
#undef GS_LAUNCH
#undef GS_LAUNCH1
    HIP_CHECK_LAST();
    return hipSuccess;
}
