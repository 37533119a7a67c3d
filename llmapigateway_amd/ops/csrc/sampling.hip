// Token sampling for gfx950: greedy argmax / Gumbel-max temperature sampling
// over [B, V] fp32 logits (V up to ~128k). Honors the OpenAI temperature
// param routed through the gateway payload (reference chat.py:116-119).
//
// Two-stage split-V reduction: a single workgroup per sequence leaves 3/4
// of the chip idle at B<=64 and runs latency-bound (measured 160 us for
// 64x128k); stage 1 spreads (B x SPLITS) workgroups over the vocab, stage 2
// combines the per-split winners. Gumbel-max: argmax(logits/T +
// -log(-log(u))) samples softmax(logits/T); noise u comes from the caller
// so CPU and GPU paths share one RNG.

#include "common.h"

#define SAMPLE_SPLITS 16

__device__ __forceinline__ void better(
    float v, int i, float& bv, int& bi) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

__launch_bounds__(256)
__global__ void sample_partial_kernel(
    float* __restrict__ part_val,         // [B, SPLITS]
    int* __restrict__ part_idx,           // [B, SPLITS]
    const float* __restrict__ logits,     // [B, V]
    const float* __restrict__ temperature,// [B]
    const float* __restrict__ noise,      // [B, V] or nullptr
    int V) {
    const int b = blockIdx.x;
    const int split = blockIdx.y;
    const int tid = threadIdx.x;
    const float T = temperature[b];
    const bool greedy = (T <= 0.f) || (noise == nullptr);
    const float invT = greedy ? 1.f : 1.f / fmaxf(T, 1e-6f);
    const float* row = logits + (size_t)b * V;
    const float* nrow = noise ? noise + (size_t)b * V : nullptr;

    const int chunk = (V + SAMPLE_SPLITS - 1) / SAMPLE_SPLITS;
    const int lo = split * chunk;
    const int hi = min(V, lo + chunk);

    float best = -INFINITY;
    int best_idx = lo;
    for (int i = lo + tid; i < hi; i += blockDim.x) {
        float val = row[i];
        if (!greedy) {
            const float u = fmaxf(nrow[i], 1e-20f);
            const float g = -logf(fmaxf(-logf(u), 1e-20f));
            val = val * invT + g;
        }
        better(val, i, best, best_idx);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, WAVE_SIZE);
        const int oi = __shfl_xor(best_idx, off, WAVE_SIZE);
        better(ov, oi, best, best_idx);
    }
    __shared__ float sv[4];
    __shared__ int si[4];
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        sv[wave] = best;
        si[wave] = best_idx;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) better(sv[w], si[w], best, best_idx);
        part_val[b * SAMPLE_SPLITS + split] = best;
        part_idx[b * SAMPLE_SPLITS + split] = best_idx;
    }
}

__launch_bounds__(64)
__global__ void sample_combine_kernel(
    int64_t* __restrict__ out,
    const float* __restrict__ part_val,
    const int* __restrict__ part_idx) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    float v = lane < SAMPLE_SPLITS ? part_val[b * SAMPLE_SPLITS + lane] : -INFINITY;
    int i = lane < SAMPLE_SPLITS ? part_idx[b * SAMPLE_SPLITS + lane] : 0x7FFFFFFF;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, WAVE_SIZE);
        const int oi = __shfl_xor(i, off, WAVE_SIZE);
        better(ov, oi, v, i);
    }
    if (lane == 0) out[b] = i;
}

// ---------------------------------------------------------------------------
// top-k / top-p (nucleus) filtering: mask logits outside the kept set to
// -inf, in place, one workgroup per row. No sort: a 2048-bin histogram
// over a 16-logit window below the row max locates the coarse threshold
// bin (counts for top-k, exp-mass for top-p), a second 2048-bin histogram
// WITHIN that bin refines the cut to 16/2048^2 ~= 3.8e-6 logit granularity.
//
// Contract (pinned by tests/elem_cases.py and test_sampling_edges_gpu.py),
// with c the cut logit of the exact semantics of reference.topk_topp_filter
// (the k-th largest / the token at which the softmax mass reaches p):
//  - every logit >= c is kept with its value unchanged, so exact ties at
//    the cut are kept together (torch's sort breaks them arbitrarily);
//  - every logit below c by more than one fine bin plus the fp32 rounding
//    of (max - logit) is masked; anything closer to the cut may be kept;
//  - top_k is honoured wherever the k-th largest finite logit lies within
//    TPF_WINDOWS * (16 - 1/128) ~= 143.9 of the row max: when the crossing
//    is not in the 2047 regular bins of a window, the window is re-based
//    onto its tail bin with the running count and mass carried, at most
//    TPF_WINDOWS - 1 times (one more read pass each). Beyond that depth,
//    or when the row has fewer than k finite logits, nothing is masked;
//  - with top-p alone a crossing in the first window's tail bin (logits
//    >= 16 - 1/128 below the max, < 1.2e-7 of the mass) masks nothing: a
//    superset of the nucleus, and nothing within 16 of the max is lost;
//  - -inf entries stay -inf and never count towards k;
//  - rows with topk[b] == 0 (or >= V) and topp[b] >= 1 are untouched.
// A row whose crossing lies in the first window takes 4 read passes + 1
// write pass over [B, V], vs a full-vocab sort + per-row host loop (the
// round-1 weakness).
// ---------------------------------------------------------------------------

#define TPF_BINS 2048
#define TPF_RANGE 16.0f  // logits below max-16 carry < 1.2e-7 of the mass
#define TPF_WINDOWS 9    // 9 * (16 - 1/128) > 128: top-k depth below the max

__launch_bounds__(256)
__global__ void topk_topp_filter_kernel(
    float* __restrict__ logits,          // [B, V], filtered in place
    const float* __restrict__ topp,      // [B]; >= 1 disables
    const int* __restrict__ topk,        // [B]; 0 disables
    int V) {
    const int b = blockIdx.x;
    const float p = topp[b];
    const int k = topk[b];
    const bool do_p = p < 1.0f;
    const bool do_k = k > 0 && k < V;  // the V largest of V: nothing to mask
    if (!do_p && !do_k) return;
    float* row = logits + (size_t)b * V;
    const int tid = threadIdx.x;

    __shared__ float s_red[4];
    __shared__ int s_cnt[TPF_BINS];
    __shared__ float s_mass[TPF_BINS];
    __shared__ float s_cut;       // mask threshold, relative to the window top
    __shared__ float s_cmass;     // mass above the bin being refined / window
    __shared__ long long s_ccnt;  // count above it
    __shared__ int s_bstar;       // coarse bin of the crossing
    __shared__ int s_flag;        // 0 keep everything, 1 found, 2 re-base

    // ---- pass 1: row max ----
    float m = -INFINITY;
    for (int i = tid; i < V; i += blockDim.x) m = fmaxf(m, row[i]);
    m = wave_reduce_max(m);
    if ((tid & 63) == 0) s_red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));

    const float scale = TPF_BINS / TPF_RANGE;
    const float window_step = (TPF_BINS - 1) / scale;  // tail bin's lower edge
    float d0 = 0.f;  // distance of the current window's top below the max
    float Z = 0.f;
    if (tid == 0) {
        s_cmass = 0.f;
        s_ccnt = 0;
    }

    // ---- pass 2 (once per window): coarse histogram (+ total softmax mass
    // in the first). -inf entries (d = +inf) carry no mass and no rank ----
    for (int win = 0;; ++win) {
        for (int i = tid; i < TPF_BINS; i += blockDim.x) {
            s_cnt[i] = 0;
            s_mass[i] = 0.f;
        }
        __syncthreads();
        float zloc = 0.f;
        for (int i = tid; i < V; i += blockDim.x) {
            const float d = m - row[i];  // >= 0; +inf for masked entries
            const float rel = d - d0;
            const bool in_win = rel >= 0.f && d < INFINITY;
            if (win == 0 || in_win) {  // a re-based window skips what is above it
                const float e = __expf(-d);
                zloc += e;  // used by the first window only
                if (in_win) {
                    const int bin = min((int)(rel * scale), TPF_BINS - 1);
                    atomicAdd(&s_cnt[bin], 1);
                    atomicAdd(&s_mass[bin], e);
                }
            }
        }
        if (win == 0) {
            zloc = wave_reduce_sum(zloc);
            __syncthreads();  // s_red reuse
            if ((tid & 63) == 0) s_red[tid >> 6] = zloc;
            __syncthreads();
            Z = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        } else {
            __syncthreads();
        }

        // coarse scan (thread 0; crossing is near the top in practice)
        if (tid == 0) {
            const float needZ = do_p ? p * Z : INFINITY;
            const long long needK = do_k ? k : 0x7FFFFFFFLL;
            float cum_mass = s_cmass;
            long long cum_cnt = s_ccnt;
            int bstar = -1;
            for (int i = 0; i < TPF_BINS - 1; ++i) {
                cum_mass += s_mass[i];
                cum_cnt += s_cnt[i];
                if (cum_mass >= needZ || cum_cnt >= needK) {
                    bstar = i;
                    break;
                }
            }
            if (bstar >= 0) {
                s_flag = 1;
                s_bstar = bstar;
                s_cmass = cum_mass - s_mass[bstar];  // mass above bstar
                s_ccnt = cum_cnt - s_cnt[bstar];
            } else if (do_k && s_cnt[TPF_BINS - 1] > 0 && win + 1 < TPF_WINDOWS) {
                s_flag = 2;  // the k-th largest is in the tail bin: re-base
                s_cmass = cum_mass;
                s_ccnt = cum_cnt;
            } else {
                s_flag = 0;  // keep everything
            }
        }
        __syncthreads();
        const int flag = s_flag;
        if (flag == 0) return;
        if (flag == 1) break;
        d0 += window_step;  // exact: a multiple of 1/128 below 2^8
    }
    const int bstar = s_bstar;

    // ---- pass 3: fine histogram within coarse bin bstar ----
    for (int i = tid; i < TPF_BINS; i += blockDim.x) {
        s_cnt[i] = 0;
        s_mass[i] = 0.f;
    }
    __syncthreads();
    const float d_lo = bstar / scale;  // coarse bin lower edge (in-window)
    const float fine_scale = scale * TPF_BINS;
    for (int i = tid; i < V; i += blockDim.x) {
        const float d = m - row[i];
        const float rel = d - d0;
        if (rel >= 0.f && d < INFINITY) {
            const int cb = min((int)(rel * scale), TPF_BINS - 1);
            if (cb == bstar) {
                const int fb =
                    max(0, min((int)((rel - d_lo) * fine_scale), TPF_BINS - 1));
                atomicAdd(&s_cnt[fb], 1);
                atomicAdd(&s_mass[fb], __expf(-d));
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float needZ = do_p ? p * Z : INFINITY;
        const long long needK = do_k ? k : 0x7FFFFFFFLL;
        float cum_mass = s_cmass;
        long long cum_cnt = s_ccnt;
        int fstar = TPF_BINS - 1;
        for (int i = 0; i < TPF_BINS; ++i) {
            cum_mass += s_mass[i];
            cum_cnt += s_cnt[i];
            if (cum_mass >= needZ || cum_cnt >= needK) {
                fstar = i;
                break;
            }
        }
        // keep what lies strictly below the fine bin's upper edge; relative
        // to the window top this is below 16 on a 2^-18 grid, exact in fp32
        s_cut = d_lo + (fstar + 1) / fine_scale;
    }
    __syncthreads();
    const float rel_cut = s_cut;

    // ---- pass 4: mask ----
    for (int i = tid; i < V; i += blockDim.x) {
        if ((m - row[i]) - d0 >= rel_cut) row[i] = -INFINITY;
    }
}

extern "C" hipError_t launch_topk_topp_filter(
    float* logits, const float* topp, const int* topk, int B, int V,
    hipStream_t stream) {
    topk_topp_filter_kernel<<<B, 256, 0, stream>>>(logits, topp, topk, V);
    HIP_CHECK_LAST();
    return hipSuccess;
}

extern "C" hipError_t launch_sample(
    int64_t* out, const float* logits, const float* temperature,
    const float* noise, float* part_val, int* part_idx, int B, int V,
    hipStream_t stream) {
    dim3 grid1(B, SAMPLE_SPLITS);
    sample_partial_kernel<<<grid1, 256, 0, stream>>>(
        part_val, part_idx, logits, temperature, noise, V);
    HIP_CHECK_LAST();
    sample_combine_kernel<<<B, 64, 0, stream>>>(out, part_val, part_idx);
    HIP_CHECK_LAST();
    return hipSuccess;
}
