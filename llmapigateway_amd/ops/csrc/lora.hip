// Multi-LoRA batched-gather kernels for gfx950: y = W x + scale * B (A x)
// with the adapter chosen per batch row.
//
// Adapter weights sit in slot stacks (A [S, nseg*R, K], B [S, N, R], bf16;
// true rank and alpha/r per slot in device arrays), and adapter_ids[row]
// names the slot of a row (-1 = base model: the row does no work and
// nothing of it is written). One workgroup owns (part of) ONE row, so the
// slot is uniform across the workgroup and every branch on it is too.
// Nothing is read on the host and nothing allocated: both launches are
// hipGraph-capturable, and a replay follows whatever the device buffers
// hold at that time.
//
//   lora_shrink: t[row, s*R + j] = sum_k x[row, k] * A[slot, s*R + j, k]
//                for j < rank[slot] (columns j >= rank are not written).
//                The x row is staged once into LDS; each wave owns rank rows
//                of A, two at a time, streamed with 16-byte loads along K
//                and reduced across the wave in fp32.
//   lora_expand: y[row, n] = bf16(float(y[row, n]) + scale[slot] *
//                sum_j t[row, seg(n)*R + j] * B[slot, n, j]), in place.
//                A lane owns two adjacent columns (one 4-byte y access) and
//                reads their B rows with 16-byte loads; t sits in LDS, zero
//                beyond the rank, so the j loop stops at the rank rounded
//                up to 8 (B is zero-padded there).
//
// These are the plain vector forms: a row's A and B traffic is served from
// L2 when neighbouring rows share its adapter, but no tile is shared
// between rows (docs/ROADMAP.md names the segmented MFMA form).

#include "common.h"

namespace {

constexpr int LORA_THREADS = 256;
constexpr int LORA_WAVES = LORA_THREADS / WAVE_SIZE;
constexpr int LORA_MAX_R = 64;
constexpr int LORA_MAX_SEG = 3;

__device__ __forceinline__ float dot8(const uint4& a, const uint4& b) {
    float a0, a1, b0, b1, s;
    unpack2(a.x, a0, a1); unpack2(b.x, b0, b1); s = a0 * b0; s = fmaf(a1, b1, s);
    unpack2(a.y, a0, a1); unpack2(b.y, b0, b1); s = fmaf(a0, b0, s); s = fmaf(a1, b1, s);
    unpack2(a.z, a0, a1); unpack2(b.z, b0, b1); s = fmaf(a0, b0, s); s = fmaf(a1, b1, s);
    unpack2(a.w, a0, a1); unpack2(b.w, b0, b1); s = fmaf(a0, b0, s); s = fmaf(a1, b1, s);
    return s;
}

// grid (T, nseg); dynamic LDS: the x row (K bf16)
__global__ __launch_bounds__(LORA_THREADS) void lora_shrink_kernel(
    float* __restrict__ t, const bf16* __restrict__ x,
    const bf16* __restrict__ A, const int* __restrict__ ranks,
    const int* __restrict__ adapter_ids, int S, int R, int nseg, int K) {
    extern __shared__ uint4 xs[];
    const int row = blockIdx.x;
    const int seg = blockIdx.y;
    const int slot = adapter_ids[row];
    if (slot < 0 || slot >= S) return;
    const int rank = min(max(ranks[slot], 0), R);
    if (rank == 0) return;

    const int kv = K / 8;  // 16-byte vectors per row
    const uint4* xrow = reinterpret_cast<const uint4*>(x + (size_t)row * K);
    for (int i = threadIdx.x; i < kv; i += LORA_THREADS) xs[i] = xrow[i];
    __syncthreads();

    const int wave = threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x % WAVE_SIZE;
    const bf16* Aseg = A + ((size_t)slot * nseg + seg) * R * (size_t)K;
    float* trow = t + (size_t)row * nseg * R + (size_t)seg * R;
    // two A rows per pass: twice the loads in flight per LDS read of x
    for (int j = 2 * wave; j < rank; j += 2 * LORA_WAVES) {
        const bool two = j + 1 < rank;
        const uint4* a0 = reinterpret_cast<const uint4*>(Aseg + (size_t)j * K);
        const uint4* a1 = reinterpret_cast<const uint4*>(
            Aseg + (size_t)(two ? j + 1 : j) * K);
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 2
        for (int i = lane; i < kv; i += WAVE_SIZE) {
            const uint4 xv = xs[i];
            const uint4 v0 = a0[i];
            const uint4 v1 = a1[i];
            acc0 += dot8(xv, v0);
            acc1 += dot8(xv, v1);
        }
        acc0 = wave_reduce_sum(acc0);
        acc1 = wave_reduce_sum(acc1);
        if (lane == 0) {
            trow[j] = acc0;
            if (two) trow[j + 1] = acc1;
        }
    }
}

// grid (T, ny): blockIdx.y strides over 512-column chunks of the row
__global__ __launch_bounds__(LORA_THREADS) void lora_expand_kernel(
    bf16* __restrict__ y, const float* __restrict__ t,
    const bf16* __restrict__ B, const int* __restrict__ ranks,
    const float* __restrict__ scales, const int* __restrict__ adapter_ids,
    int S, int R, int nseg, int N, int b1, int b2) {
    __shared__ __attribute__((aligned(16))) float ts[LORA_MAX_SEG * LORA_MAX_R];
    const int row = blockIdx.x;
    const int slot = adapter_ids[row];
    if (slot < 0 || slot >= S) return;
    const int rank = min(max(ranks[slot], 0), R);
    if (rank == 0) return;
    const float scale = scales[slot];

    const float* trow = t + (size_t)row * nseg * R;
    for (int i = threadIdx.x; i < nseg * R; i += LORA_THREADS)
        ts[i] = (i % R) < rank ? trow[i] : 0.f;
    __syncthreads();

    const int jv = (rank + 7) / 8;  // 16-byte vectors of a B row in use
    const bf16* Bs = B + (size_t)slot * N * R;
    uint32_t* yrow = reinterpret_cast<uint32_t*>(y + (size_t)row * N);
    for (int n = 2 * (blockIdx.y * LORA_THREADS + threadIdx.x); n < N;
         n += 2 * LORA_THREADS * gridDim.y) {
        // segment bounds are even, so a column pair never straddles one
        const int seg = (n >= b1) + (n >= b2);
        const float4* tv = reinterpret_cast<const float4*>(ts + seg * R);
        const uint4* r0 = reinterpret_cast<const uint4*>(Bs + (size_t)n * R);
        const uint4* r1 = reinterpret_cast<const uint4*>(Bs + (size_t)(n + 1) * R);
        float acc0 = 0.f, acc1 = 0.f;
        for (int j = 0; j < jv; ++j) {
            const uint4 v0 = r0[j];
            const uint4 v1 = r1[j];
            const float4 ta = tv[2 * j];
            const float4 tb = tv[2 * j + 1];
            float lo, hi;
            unpack2(v0.x, lo, hi); acc0 = fmaf(ta.x, lo, acc0); acc0 = fmaf(ta.y, hi, acc0);
            unpack2(v0.y, lo, hi); acc0 = fmaf(ta.z, lo, acc0); acc0 = fmaf(ta.w, hi, acc0);
            unpack2(v0.z, lo, hi); acc0 = fmaf(tb.x, lo, acc0); acc0 = fmaf(tb.y, hi, acc0);
            unpack2(v0.w, lo, hi); acc0 = fmaf(tb.z, lo, acc0); acc0 = fmaf(tb.w, hi, acc0);
            unpack2(v1.x, lo, hi); acc1 = fmaf(ta.x, lo, acc1); acc1 = fmaf(ta.y, hi, acc1);
            unpack2(v1.y, lo, hi); acc1 = fmaf(ta.z, lo, acc1); acc1 = fmaf(ta.w, hi, acc1);
            unpack2(v1.z, lo, hi); acc1 = fmaf(tb.x, lo, acc1); acc1 = fmaf(tb.y, hi, acc1);
            unpack2(v1.w, lo, hi); acc1 = fmaf(tb.z, lo, acc1); acc1 = fmaf(tb.w, hi, acc1);
        }
        float y0, y1;
        unpack2(yrow[n / 2], y0, y1);
        yrow[n / 2] = pack2(y0 + scale * acc0, y1 + scale * acc1);
    }
}

}  // namespace

extern "C" hipError_t launch_lora_shrink(
    float* t, const void* x, const void* A, const int* ranks,
    const int* adapter_ids, int T, int S, int R, int nseg, int K,
    hipStream_t stream) {
    if (T <= 0) return hipSuccess;
    if (R <= 0 || R > LORA_MAX_R || R % 8 != 0) return hipErrorInvalidValue;
    if (nseg < 1 || nseg > LORA_MAX_SEG) return hipErrorInvalidValue;
    // the x row lives in LDS: 64 KiB holds K = 32768
    if (K <= 0 || K % 8 != 0 || K > 32768) return hipErrorInvalidValue;
    lora_shrink_kernel<<<dim3(T, nseg), LORA_THREADS, (size_t)K * sizeof(bf16),
                         stream>>>(t, (const bf16*)x, (const bf16*)A, ranks,
                                   adapter_ids, S, R, nseg, K);
    HIP_CHECK_LAST();
    return hipSuccess;
}

extern "C" hipError_t launch_lora_expand(
    void* y, const float* t, const void* B, const int* ranks,
    const float* scales, const int* adapter_ids, int T, int S, int R, int nseg,
    int N, int b1, int b2, hipStream_t stream) {
    if (T <= 0) return hipSuccess;
    if (R <= 0 || R > LORA_MAX_R || R % 8 != 0) return hipErrorInvalidValue;
    if (nseg < 1 || nseg > LORA_MAX_SEG) return hipErrorInvalidValue;
    if (N <= 0 || N % 2 != 0 || b1 % 2 != 0 || b2 % 2 != 0)
        return hipErrorInvalidValue;
    // memory-bound: about 2048 workgroups in all, grid-striding the rest
    const int chunks = ceil_div_i(N, 2 * LORA_THREADS);
    const int cap = 2048 / T > 1 ? 2048 / T : 1;
    const int ny = chunks < cap ? chunks : cap;
    lora_expand_kernel<<<dim3(T, ny), LORA_THREADS, 0, stream>>>(
        (bf16*)y, t, (const bf16*)B, ranks, scales, adapter_ids, S, R, nseg, N,
        b1, b2);
    HIP_CHECK_LAST();
    return hipSuccess;
}
