// W8A16 skinny-M streaming GEMM for gfx950:
//   Y[M,N] = X[M,K] · (scale ⊙ Q)[N,K]^T,  X bf16, Q fp8 e4m3fn, fp32 acc.
//
// The decode projections are weight-stream-bound (see gemm_skinny.hip); fp8
// weights halve the bytes each step has to stream. Same structure as
// gemm_skinny.hip, whose pipelining lessons apply unchanged:
//
// - grid = (N/64 n-stripes) x (split-K slices); one workgroup owns ALL M
//   rows of its stripe for its K-slice, so Q is streamed exactly once.
// - up to 8 waves; wave w owns M rows [w*16*MF, ..): MF m-fragments x 4
//   n-fragments of v_mfma_f32_16x16x32_bf16.
// - Q is fragment-major [K/64, N/16, 64, 16] (ops.swizzle_weight_frag_fp8):
//   lane l's 16 bytes are its B-fragments for TWO consecutive 32-deep
//   k-steps (bytes 0-7 then 8-15), so one k64 step of a stripe is four
//   contiguous 1 KiB rows, one 16-byte load per lane each.
// - dequantisation happens in registers: cvt_pk e4m3 -> f32, keep the high
//   16 bits. e4m3 has 3 mantissa bits, so the truncation is exact and the
//   bf16 MFMA sees exactly the fp8 values.
// - the per-output-channel scale multiplies the fp32 accumulator in the
//   epilogue (C-fragment column = lane & 15), BEFORE the bf16 store or the
//   slab store: split-K slabs hold finished partial sums and the existing
//   launch_gemm_reduce / launch_gemm_reduce_rmsnorm consume them as they
//   are.
// - loads go through explicit global-address-space pointers and the
//   depth-4 software pipeline (in k64 steps) is held in shape by
//   sched_barriers.
// - no atomics; every workgroup fully writes the [M x 64] stripe it owns
//   (of y, or of slab blockIdx.y — a slice with no k-steps writes zeros).
//
// dequant_w8_kernel expands the fp8 twin to a row-major bf16 [N,K] buffer
// for M > 256 (prefill), which then runs on the library GEMM.

#include "common.h"

#define W8_MAX_M 256
#define W8_NF 4                  // 16-col n-fragments per stripe
#define W8_NT (W8_NF * 16)       // stripe width = 64 columns

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short w8_bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float w8_f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t w8_u32x4;

extern "C" hipError_t launch_gemm_reduce(void*, const float*, int64_t, int, hipStream_t);
extern "C" hipError_t launch_gemm_reduce_rmsnorm(void*, void*, const float*, const void*, float, int, int, int, hipStream_t);

__device__ __forceinline__ w8_f32x4 w8_mfma(w8_bf16x8 a, w8_bf16x8 b, w8_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 16-B loads through explicit global (addrspace 1) pointers: loop-carried
// generic pointers demote to flat_load, which also drains lgkmcnt
__device__ __forceinline__ w8_bf16x8 w8_gload_a(const bf16* p) {
    return *(const __attribute__((address_space(1))) w8_bf16x8*)(unsigned long long)p;
}
__device__ __forceinline__ w8_u32x4 w8_gload_b(const uint8_t* p) {
    return *(const __attribute__((address_space(1))) w8_u32x4*)(unsigned long long)p;
}

// 4 e4m3 bytes -> 4 bf16 (2 packed words). The f32 image of an e4m3 value
// has at most 3 mantissa bits, so its high half IS the bf16 value.
__device__ __forceinline__ void w8_cvt4(uint32_t q, uint32_t& w0, uint32_t& w1) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(q, false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(q, true);
    w0 = pack2_trunc(lo[0], lo[1]);
    w1 = pack2_trunc(hi[0], hi[1]);
}

// 8 e4m3 bytes (two words) -> one B fragment
__device__ __forceinline__ w8_bf16x8 w8_dequant8(uint32_t q0, uint32_t q1) {
    union { uint32_t u[4]; w8_bf16x8 v; } c;
    w8_cvt4(q0, c.u[0], c.u[1]);
    w8_cvt4(q1, c.u[2], c.u[3]);
    return c.v;
}

#define W8_FENCE __builtin_amdgcn_sched_barrier(0)

// blockDim = nwaves*64 with nwaves = ceil(M / (16*MF)) <= 8; MF in {1, 2}
// covers M <= 256.
template <int MF, bool SPLITK>
__launch_bounds__(8 * WAVE_SIZE)
__global__ void gemm_w8_kernel(
    bf16* __restrict__ y,            // [M, N] (!SPLITK)
    float* __restrict__ yw,          // [nsk, M, N] fp32 slabs (SPLITK)
    const bf16* __restrict__ x,      // [M, K]
    const uint8_t* __restrict__ q,   // [K/64, N/16, 64, 16] e4m3
    const float* __restrict__ scale, // [N]
    int M,
    int N,
    int K,
    int nsk) {
    const int n0 = blockIdx.x * W8_NT;
    const int kslice = ((K / 64 + nsk - 1) / nsk) * 64;
    const int k0 = (SPLITK ? blockIdx.y : 0) * kslice;
    const int k1 = min(K, k0 + kslice);

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x >> 6;
    const int lrow = lane & 15;  // A row / B col within a fragment
    const int lk = lane >> 4;    // k-group of 8

    const int m_base = wave * (MF * 16);

    w8_f32x4 acc[MF][W8_NF];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int n = 0; n < W8_NF; ++n) acc[f][n] = (w8_f32x4){0.f, 0.f, 0.f, 0.f};

    const int nsteps = (k1 - k0) / 64;  // K and kslice are 64-aligned
    if (nsteps > 0 && m_base < M) {
        const bf16* ap[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const int r = m_base + f * 16 + lrow;
            ap[f] = x + (size_t)(r < M ? r : 0) * K + k0 + lk * 8;
        }
        // the stripe's four fragment rows are adjacent: 1 KiB apart; one
        // k64 step further is a whole [N/16, 64, 16] plane = 64*N bytes
        const size_t bstep = (size_t)64 * N;
        const uint8_t* bp = q + (size_t)(k0 / 64) * bstep +
                            ((size_t)(n0 / 16) * 64 + lane) * 16;

        // explicit buffer sets, all indices compile-time (see
        // gemm_skinny.hip); a set is one k64 step: 2*MF A-fragments and
        // four 16-byte Q loads
        w8_bf16x8 a0[2 * MF], a1[2 * MF], a2[2 * MF], a3[2 * MF];
        w8_u32x4 b0[W8_NF], b1[W8_NF], b2[W8_NF], b3[W8_NF];
#define W8_LOAD(AV, BV, S)                                                     \
    do {                                                                       \
        _Pragma("unroll") for (int f = 0; f < MF; ++f) {                       \
            AV[2 * f] = w8_gload_a(ap[f] + (S) * 64);                          \
            AV[2 * f + 1] = w8_gload_a(ap[f] + (S) * 64 + 32);                 \
        }                                                                      \
        _Pragma("unroll") for (int n = 0; n < W8_NF; ++n) BV[n] =              \
            w8_gload_b(bp + (S) * bstep + n * 1024);                           \
    } while (0)
#define W8_MFMA_ALL(AV, BV)                                                    \
    do {                                                                       \
        _Pragma("unroll") for (int n = 0; n < W8_NF; ++n) {                    \
            const w8_bf16x8 blo = w8_dequant8(BV[n][0], BV[n][1]);             \
            const w8_bf16x8 bhi = w8_dequant8(BV[n][2], BV[n][3]);             \
            _Pragma("unroll") for (int f = 0; f < MF; ++f) {                   \
                acc[f][n] = w8_mfma(AV[2 * f], blo, acc[f][n]);                \
                acc[f][n] = w8_mfma(AV[2 * f + 1], bhi, acc[f][n]);            \
            }                                                                  \
        }                                                                      \
    } while (0)
#define W8_BUMP(STEPS)                                                         \
    do {                                                                       \
        _Pragma("unroll") for (int f = 0; f < MF; ++f) ap[f] += (STEPS) * 64;  \
        bp += (STEPS) * bstep;                                                 \
    } while (0)
        if (nsteps < 3) {
            for (int s = 0; s < nsteps; ++s) {
                W8_LOAD(a0, b0, 0);
                W8_MFMA_ALL(a0, b0);
                W8_BUMP(1);
            }
        } else {
            W8_LOAD(a0, b0, 0);
            W8_LOAD(a1, b1, 1);
            W8_LOAD(a2, b2, 2);
            int s = 0;
            for (; s + 7 <= nsteps; s += 4) {  // prefetches reach s+6
                W8_LOAD(a3, b3, 3);
                W8_FENCE;
                W8_MFMA_ALL(a0, b0);
                W8_FENCE;
                W8_LOAD(a0, b0, 4);
                W8_FENCE;
                W8_MFMA_ALL(a1, b1);
                W8_FENCE;
                W8_LOAD(a1, b1, 5);
                W8_FENCE;
                W8_MFMA_ALL(a2, b2);
                W8_FENCE;
                W8_LOAD(a2, b2, 6);
                W8_FENCE;
                W8_MFMA_ALL(a3, b3);
                W8_BUMP(4);
            }
            // tail: r in [3,6]; sets 0/1/2 hold steps s, s+1, s+2
            const int r = nsteps - s;
            if (r >= 4) W8_LOAD(a3, b3, 3);
            W8_MFMA_ALL(a0, b0);
            if (r >= 5) W8_LOAD(a0, b0, 4);
            W8_MFMA_ALL(a1, b1);
            if (r >= 6) W8_LOAD(a1, b1, 5);
            W8_MFMA_ALL(a2, b2);
            if (r >= 4) W8_MFMA_ALL(a3, b3);
            if (r >= 5) W8_MFMA_ALL(a0, b0);
            if (r >= 6) W8_MFMA_ALL(a1, b1);
        }
#undef W8_LOAD
#undef W8_MFMA_ALL
#undef W8_BUMP
    }

    // ---- epilogue: C fragment row = lk*4 + r, col = lrow; the channel
    // scale goes onto the fp32 accumulator before any store ----
    float sc[W8_NF];
#pragma unroll
    for (int n = 0; n < W8_NF; ++n) sc[n] = scale[n0 + n * 16 + lrow];

    if (SPLITK) {
        float* slab = yw + (size_t)blockIdx.y * M * N;
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m_base + f * 16 + lk * 4 + r;
                if (row >= M) continue;
#pragma unroll
                for (int n = 0; n < W8_NF; ++n)
                    slab[(size_t)row * N + n0 + n * 16 + lrow] =
                        acc[f][n][r] * sc[n];
            }
    } else {
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m_base + f * 16 + lk * 4 + r;
                if (row >= M) continue;
#pragma unroll
                for (int n = 0; n < W8_NF; ++n)
                    y[(size_t)row * N + n0 + n * 16 + lrow] =
                        f2bf(acc[f][n][r] * sc[n]);
            }
    }
}

// fragment-major fp8 twin + scale -> row-major bf16 [N, K]. One thread per
// 16-byte fragment entry: it owns 8 consecutive k of row n for each of the
// two 32-deep k-steps of its k64 block. Rounding is RNE; with a
// power-of-two scale the product is exact in bf16.
__global__ void dequant_w8_kernel(
    bf16* __restrict__ out,          // [N, K]
    const uint8_t* __restrict__ q,   // [K/64, N/16, 64, 16]
    const float* __restrict__ scale, // [N]
    int N, int K) {
    const int64_t total = (int64_t)(K / 64) * (N / 16) * 64;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    const int64_t frag = t >> 6;
    const int n16 = (int)(frag % (N / 16));
    const int k64 = (int)(frag / (N / 16));
    const int n = n16 * 16 + (lane & 15);
    const int kb = k64 * 64 + (lane >> 4) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(q + t * 16);
    const float s = scale[n];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float f[8];
        fp8x4_to_f32(w[2 * h], f[0], f[1], f[2], f[3]);
        fp8x4_to_f32(w[2 * h + 1], f[4], f[5], f[6], f[7]);
        uint4 o;
        o.x = pack2(f[0] * s, f[1] * s);
        o.y = pack2(f[2] * s, f[3] * s);
        o.z = pack2(f[4] * s, f[5] * s);
        o.w = pack2(f[6] * s, f[7] * s);
        *reinterpret_cast<uint4*>(out + (size_t)n * K + kb + h * 32) = o;
    }
}

extern "C" hipError_t launch_dequant_w8(
    void* out, const void* q, const float* scale, int N, int K,
    hipStream_t stream) {
    if (N <= 0 || K <= 0 || (N % W8_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    const int64_t total = (int64_t)(K / 64) * (N / 16) * 64;
    const int tpb = 256;
    dequant_w8_kernel<<<dim3((unsigned)((total + tpb - 1) / tpb)), dim3(tpb), 0,
                        stream>>>((bf16*)out, (const uint8_t*)q, scale, N, K);
    HIP_CHECK_LAST();
    return hipSuccess;
}

// With residual/norm_weight/out set (split-K only) the slab reduction also
// adds the residual and RMS-normalizes (launch_gemm_reduce_rmsnorm) and y
// is not written.
extern "C" hipError_t launch_gemm_w8(
    void* y, float* workspace, const void* x, const void* q,
    const float* scale, int M, int N, int K, int nsk, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (M <= 0 || M > W8_MAX_M) return hipErrorInvalidValue;
    if (N <= 0 || K <= 0 || (N % W8_NT) != 0 || (K % 64) != 0)
        return hipErrorInvalidValue;
    if (nsk < 1 || nsk > K / 64) return hipErrorInvalidValue;
    if (nsk > 1 && workspace == nullptr) return hipErrorInvalidValue;
    if (out != nullptr && (nsk < 2 || residual == nullptr || norm_weight == nullptr))
        return hipErrorInvalidValue;
    const int mf = M > 128 ? 2 : 1;
    const int nwaves = ceil_div_i(M, 16 * mf);
    dim3 grid(N / W8_NT, nsk);
    dim3 block(nwaves * WAVE_SIZE);
#define W8_LAUNCH(MFV, SPLIT)                                                  \
    gemm_w8_kernel<MFV, SPLIT><<<grid, block, 0, stream>>>(                    \
        (bf16*)y, workspace, (const bf16*)x, (const uint8_t*)q, scale, M, N,   \
        K, nsk)
    if (nsk == 1) {
        if (mf == 1) W8_LAUNCH(1, false);
        else W8_LAUNCH(2, false);
    } else {
        if (mf == 1) W8_LAUNCH(1, true);
        else W8_LAUNCH(2, true);
    }
#undef W8_LAUNCH
    HIP_CHECK_LAST();
    if (nsk > 1) {
        if (out != nullptr)
            return launch_gemm_reduce_rmsnorm(out, residual, workspace,
                                              norm_weight, eps, M, N, nsk,
                                              stream);
        return launch_gemm_reduce(y, workspace, (int64_t)M * N, nsk, stream);
    }
    return hipSuccess;
}
