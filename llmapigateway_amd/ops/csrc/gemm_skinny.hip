// bf16 weight policies of the skinny-M streaming GEMM (gemm_stream.h), and
// the split-K slab reductions every decode GEMM shares.
//
// Replaces F.linear on the decode hot path (models/llama.py) for
// M <= GS_MAX_M and N <= 28672. Production dispatch is the latency regime
// (ops/__init__.py: M <= 16, M <= 8 beside a fragment twin); the tuned
// library keeps M >= 64 (its LDS macro-tiles re-read X less), prefill and
// lm_head. rocBLAS/hipBLASLt run the skinny shapes 3-4x off the
// weight-stream bound (TunableOp cold-cache sweep: down-proj
// 4096x256x14336 at 66 us vs the ~15 us bound).

#include "gemm_launch.h"
#include "gemm_stream.h"

// - row-major [N, K]: one pointer per 16-row n-fragment, 32 elements per
//   k-step; 16 rows x 64 B per load instruction caps at ~3.5 TB/s
//   effective.
// - k-major [K/32, N, 32] (ops.swizzle_weight): a k-step of the stripe is
//   one contiguous 4 KB (64-row x 64 B) block, so a single pointer serves
//   the four n-fragments (1 KiB apart) and steps by a whole [N, 32] plane.
template <bool KMAJOR>
struct BBf16 {
    static constexpr int KSTEP = 32;
    static constexpr bool SCALED = false;
    struct Regs { bf16x8 v[GS_NF]; };
    const bf16* p[KMAJOR ? 1 : GS_NF];
    size_t step;  // elements per k-step
    __device__ __forceinline__ void init(const void* w, const void*, int N, int K,
                                         int n0, int k0, int lane) {
        const int lrow = lane & 15, lk = lane >> 4;
        if (KMAJOR) {
            step = (size_t)32 * N;
            p[0] = (const bf16*)w + (size_t)(k0 / 32) * step +
                   (size_t)(n0 + lrow) * 32 + lk * 8;
        } else {
            step = 32;
#pragma unroll
            for (int n = 0; n < GS_NF; ++n)
                p[n] = (const bf16*)w + (size_t)(n0 + n * 16 + lrow) * K + k0 +
                       lk * 8;
        }
    }
    __device__ __forceinline__ void load(Regs& r, int S) const {
#pragma unroll
        for (int n = 0; n < GS_NF; ++n)
            r.v[n] = KMAJOR ? gs_gload<bf16x8>(p[0] + S * step + n * 512)
                            : gs_gload<bf16x8>(p[n] + S * 32);
    }
    __device__ __forceinline__ void bump(int steps) {
#pragma unroll
        for (int n = 0; n < (KMAJOR ? 1 : GS_NF); ++n) p[n] += steps * step;
    }
    static __device__ __forceinline__ bf16x8 frag(const Regs& r, int n, int) {
        return r.v[n];
    }
};

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

extern "C" hipError_t launch_splitk_tail(
    void* y, const float* workspace, int M, int N, int nsk, void* residual,
    const void* norm_weight, float eps, void* out, hipStream_t stream) {
    if (out != nullptr)
        return launch_gemm_reduce_rmsnorm(out, residual, workspace, norm_weight,
                                          eps, M, N, nsk, stream);
    if (nsk > 1)
        return launch_gemm_reduce(y, workspace, (int64_t)M * N, nsk, stream);
    return hipSuccess;
}

// nsk may exceed K/32: the surplus slices are empty and write zero slabs
extern "C" hipError_t launch_gemm_skinny(
    void* y, float* workspace, const void* x, const void* w, int M, int N,
    int K, int nsk, int swz, hipStream_t stream) {
    if (M <= 0 || M > GS_MAX_M) return hipErrorInvalidValue;
    if ((N % GS_NT) != 0 || (K % 32) != 0) return hipErrorInvalidValue;
    if (nsk < 1) return hipErrorInvalidValue;
    if (nsk > 1 && workspace == nullptr) return hipErrorInvalidValue;
    const hipError_t err =
        swz ? launch_gemm_stream<BBf16<true>>(y, workspace, x, w, nullptr, M,
                                              N, K, nsk, stream)
            : launch_gemm_stream<BBf16<false>>(y, workspace, x, w, nullptr, M,
                                               N, K, nsk, stream);
    if (err != hipSuccess) return err;
    return launch_splitk_tail(y, workspace, M, N, nsk, nullptr, nullptr, 0.f,
                              nullptr, stream);
}
