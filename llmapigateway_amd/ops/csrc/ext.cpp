// Torch extension binding for the gfx950 kernels (built in-tree by
// `python setup.py build_ext --inplace` with PYTORCH_ROCM_ARCH=gfx950).
// The kernels themselves live in the .hip files (torch-free, raw pointers);
// this file validates tensors, extracts strides and dispatches on the
// current HIP stream.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "gemm_launch.h"
#include "kv_manager.cpp"

extern "C" {
hipError_t launch_rmsnorm(void*, const void*, const void*, float, int, int, hipStream_t);
hipError_t launch_rmsnorm_residual(void*, const void*, void*, const void*, float, int, int, hipStream_t);
hipError_t launch_rope(void*, void*, const int64_t*, const float*, int, int64_t, int64_t, int, int, int, hipStream_t);
hipError_t launch_swiglu(void*, const void*, int, int, hipStream_t);
hipError_t launch_kv_cache_write(const void*, const void*, void*, void*, float*, float*, const int64_t*, int, int64_t, int64_t, int, int, int, hipStream_t);
hipError_t launch_rope_kv(void*, void*, const void*, void*, void*, float*, float*, const int64_t*, const float*, const int64_t*, int, int64_t, int64_t, int64_t, int, int, int, int, hipStream_t);
hipError_t launch_attention_decode(void*, const void*, const void*, const void*, const float*, const float*, const int*, const int*, float, int, int, int, int, int, int, int64_t, float*, float*, int, int, int, hipStream_t);
hipError_t launch_attention_prefill(void*, const void*, const void*, const void*, const int*, const int*, const int*, int, float, int, int, int, int64_t, int64_t, int64_t, const void*, const void*, const float*, const float*, const int*, const int*, int, int, int, hipStream_t);
hipError_t launch_sample(int64_t*, const float*, const float*, const float*, float*, int*, int, int, hipStream_t);
hipError_t launch_topk_topp_filter(float*, const float*, const int*, int, int, hipStream_t);
hipError_t launch_lora_shrink(float*, const void*, const void*, const int*, const int*, int, int, int, int, int, hipStream_t);
hipError_t launch_lora_expand(void*, const float*, const void*, const int*, const float*, const int*, int, int, int, int, int, int, int, hipStream_t);
int lora_pick_mf(int, int);
int lora_pick_nsk(int, int, int, int);
hipError_t launch_lora_align(int*, int*, const int*, const int*, int, int, int, int, hipStream_t);
hipError_t launch_lora_shrink_seg(float*, const void*, const void*, const int*, const int*, const int*, int, int, int, int, int, int, int, hipStream_t);
hipError_t launch_lora_expand_seg(void*, const float*, const void*, const int*, const int*, const int*, const float*, int, int, int, int, int, int, int, int, int, hipStream_t);
int moe_pick_mf(int, int, int);
hipError_t launch_moe_route(int*, float*, const void*, const void*, int, int, int, int, hipStream_t);
hipError_t launch_moe_align(int*, int*, const int*, int, int, int, int, hipStream_t);
hipError_t launch_moe_gemm(void*, const void*, const void*, const int*, const int*, const float*, int, int, int, int, int, int, hipStream_t);
hipError_t launch_moe_combine_norm(void*, void*, const void*, const void*, float, int, int, int, hipStream_t);
hipError_t launch_moe_gemm_w4(void*, const void*, const void*, const void*, const int*, const int*, const float*, int, int, int, int, int, int, hipStream_t);
hipError_t launch_moe_gemm_w8(void*, const void*, const void*, const float*, const int*, const int*, const float*, int, int, int, int, int, int, hipStream_t);
}

namespace {

#define CHECK_HIP(call)                                                        \
    do {                                                                       \
        hipError_t err = (call);                                               \
        TORCH_CHECK(err == hipSuccess, "HIP kernel failed: ",                  \
                    hipGetErrorString(err));                                   \
    } while (0)

hipStream_t current_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

void check_bf16(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
}

// fp8 KV caches are stored as uint8 (e4m3 bits) with fp32 row scales
void check_cache(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16 ||
                t.scalar_type() == torch::kUInt8,
                name, " must be bf16 or uint8(e4m3)");
}

float* scale_ptr(const c10::optional<torch::Tensor>& s) {
    if (!s.has_value() || !s->defined()) return nullptr;
    TORCH_CHECK(s->scalar_type() == torch::kFloat32 && s->is_contiguous());
    return s->data_ptr<float>();
}

// Shared host-side contract of the two rmsnorm bindings: every tensor bf16
// on the GPU and contiguous, weight exactly one row wide, out (and the
// residual) shaped like x. The kernels index all of them by x's T and H.
void check_rmsnorm_args(const torch::Tensor& out, const torch::Tensor& x,
                        const torch::Tensor* residual,
                        const torch::Tensor& weight) {
    check_bf16(x, "x");
    check_bf16(out, "out");
    check_bf16(weight, "weight");
    TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "x must be [..., H] with H > 0");
    TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && weight.is_contiguous(),
                "x, out and weight must be contiguous");
    TORCH_CHECK(weight.numel() == x.size(-1),
                "weight must have H = ", x.size(-1), " elements, got ",
                weight.numel());
    TORCH_CHECK(out.sizes() == x.sizes(), "out must have the shape of x");
    if (residual != nullptr) {
        check_bf16(*residual, "residual");
        TORCH_CHECK(residual->is_contiguous(), "residual must be contiguous");
        TORCH_CHECK(residual->sizes() == x.sizes(),
                    "residual must have the shape of x");
    }
}

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor weight, double eps) {
    check_rmsnorm_args(out, x, nullptr, weight);
    const int H = x.size(-1);
    const int T = x.numel() / H;
    CHECK_HIP(launch_rmsnorm(out.data_ptr(), x.data_ptr(), weight.data_ptr(),
                             (float)eps, T, H, current_stream()));
}

void rmsnorm_residual(torch::Tensor out, torch::Tensor x, torch::Tensor residual,
                      torch::Tensor weight, double eps) {
    check_rmsnorm_args(out, x, &residual, weight);
    const int H = x.size(-1);
    const int T = x.numel() / H;
    CHECK_HIP(launch_rmsnorm_residual(out.data_ptr(), x.data_ptr(),
                                      residual.data_ptr(), weight.data_ptr(),
                                      (float)eps, T, H, current_stream()));
}

void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor positions,
                  torch::Tensor cos_sin) {
    check_bf16(q, "q");
    check_bf16(k, "k");
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q/k must be [T, H, D]");
    TORCH_CHECK(q.stride(2) == 1 && k.stride(2) == 1, "head_dim must be contiguous");
    TORCH_CHECK(q.stride(1) == q.size(2) && k.stride(1) == k.size(2),
                "heads must be contiguous within a row");
    TORCH_CHECK(positions.scalar_type() == torch::kInt64);
    TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_contiguous());
    const int T = q.size(0);
    CHECK_HIP(launch_rope(q.data_ptr(), k.data_ptr(),
                          positions.data_ptr<int64_t>(),
                          cos_sin.data_ptr<float>(), T, q.stride(0), k.stride(0),
                          q.size(1), k.size(1), q.size(2), current_stream()));
}

void swiglu(torch::Tensor out, torch::Tensor x) {
    check_bf16(x, "x");
    TORCH_CHECK(x.is_contiguous() && out.is_contiguous());
    const int I = out.size(-1);
    TORCH_CHECK(x.size(-1) == 2 * I, "x last dim must be 2*I");
    const int T = x.numel() / (2 * I);
    CHECK_HIP(launch_swiglu(out.data_ptr(), x.data_ptr(), T, I, current_stream()));
}

void kv_cache_write(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                    torch::Tensor v_cache, torch::Tensor slot_mapping,
                    c10::optional<torch::Tensor> k_scale,
                    c10::optional<torch::Tensor> v_scale) {
    check_bf16(k, "k");
    check_cache(k_cache, "k_cache");
    TORCH_CHECK(k.dim() == 3 && k_cache.dim() == 4);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == k.size(2));
    TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == v.size(2));
    TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
    TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
    const int T = k.size(0);
    const int Hkv = k_cache.size(1);
    const int block_size = k_cache.size(2);
    const int D = k_cache.size(3);
    TORCH_CHECK((k_cache.scalar_type() == torch::kUInt8) ==
                (k_scale.has_value() && k_scale->defined()),
                "fp8 cache needs scales; bf16 cache must not have them");
    CHECK_HIP(launch_kv_cache_write(
        k.data_ptr(), v.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        scale_ptr(k_scale), scale_ptr(v_scale),
        slot_mapping.data_ptr<int64_t>(), T, k.stride(0), v.stride(0), Hkv,
        block_size, D, current_stream()));
}

void rope_kv_write(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                   torch::Tensor k_cache, torch::Tensor v_cache,
                   torch::Tensor positions, torch::Tensor cos_sin,
                   torch::Tensor slot_mapping,
                   c10::optional<torch::Tensor> k_scale,
                   c10::optional<torch::Tensor> v_scale) {
    check_bf16(q, "q");
    check_bf16(k, "k");
    check_cache(k_cache, "k_cache");
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3 && k_cache.dim() == 4);
    TORCH_CHECK(q.stride(2) == 1 && k.stride(2) == 1 && v.stride(2) == 1);
    TORCH_CHECK(q.stride(1) == q.size(2) && k.stride(1) == k.size(2) &&
                v.stride(1) == v.size(2));
    TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
    TORCH_CHECK(positions.scalar_type() == torch::kInt64);
    TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
    TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_contiguous());
    const int T = q.size(0);
    CHECK_HIP(launch_rope_kv(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), k_cache.data_ptr(),
        v_cache.data_ptr(), scale_ptr(k_scale), scale_ptr(v_scale),
        positions.data_ptr<int64_t>(),
        cos_sin.data_ptr<float>(), slot_mapping.data_ptr<int64_t>(), T,
        q.stride(0), k.stride(0), v.stride(0), q.size(1), k_cache.size(1),
        q.size(2), k_cache.size(2), current_stream()));
}

void attention_decode(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                      torch::Tensor v_cache, torch::Tensor block_tables,
                      torch::Tensor context_lens, double scale,
                      c10::optional<torch::Tensor> part_acc,
                      c10::optional<torch::Tensor> part_ml, int64_t nsplit,
                      c10::optional<torch::Tensor> k_scale,
                      c10::optional<torch::Tensor> v_scale, int64_t version,
                      int64_t window) {
    TORCH_CHECK(window >= 0 && window <= INT32_MAX, "window must be >= 0");
    check_cache(k_cache, "k_cache");
    TORCH_CHECK((k_cache.scalar_type() == torch::kUInt8) ==
                (k_scale.has_value() && k_scale->defined()),
                "fp8 cache needs scales; bf16 cache must not have them");
    check_bf16(q, "q");
    check_bf16(out, "out");
    TORCH_CHECK(out.is_contiguous());
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
    TORCH_CHECK(block_tables.scalar_type() == torch::kInt32 && block_tables.is_contiguous());
    TORCH_CHECK(context_lens.scalar_type() == torch::kInt32);
    const int B = q.size(0);
    const int Hq = q.size(1);
    const int D = q.size(2);
    const int Hkv = k_cache.size(1);
    const int block_size = k_cache.size(2);
    const int max_blocks = block_tables.size(1);
    float* pa = nullptr;
    float* pm = nullptr;
    if (nsplit > 1) {
        TORCH_CHECK(part_acc.has_value() && part_ml.has_value());
        TORCH_CHECK(part_acc->scalar_type() == torch::kFloat32 &&
                    part_acc->numel() >= (int64_t)B * Hq * nsplit * D);
        TORCH_CHECK(part_ml->scalar_type() == torch::kFloat32 &&
                    part_ml->numel() >= (int64_t)B * Hq * nsplit * 2);
        pa = part_acc->data_ptr<float>();
        pm = part_ml->data_ptr<float>();
    }
    CHECK_HIP(launch_attention_decode(
        out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        scale_ptr(k_scale), scale_ptr(v_scale),
        block_tables.data_ptr<int>(), context_lens.data_ptr<int>(), (float)scale,
        B, Hq, Hkv, block_size, max_blocks, D, q.stride(0), pa, pm, (int)nsplit,
        (int)version, (int)window, current_stream()));
}

void attention_prefill(torch::Tensor out, torch::Tensor q, torch::Tensor k,
                       torch::Tensor v, torch::Tensor cu_seqlens,
                       torch::Tensor tile_seq, torch::Tensor tile_off,
                       double scale,
                       c10::optional<torch::Tensor> k_cache,
                       c10::optional<torch::Tensor> v_cache,
                       c10::optional<torch::Tensor> block_tables,
                       c10::optional<torch::Tensor> cached_lens,
                       c10::optional<torch::Tensor> k_scale,
                       c10::optional<torch::Tensor> v_scale, int64_t window) {
    TORCH_CHECK(window >= 0 && window <= INT32_MAX, "window must be >= 0");
    check_bf16(q, "q");
    check_bf16(out, "out");
    TORCH_CHECK(out.is_contiguous());
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == k.size(2));
    TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == v.size(2));
    TORCH_CHECK(cu_seqlens.scalar_type() == torch::kInt32);
    TORCH_CHECK(tile_seq.scalar_type() == torch::kInt32 &&
                tile_off.scalar_type() == torch::kInt32);
    const int ntiles = tile_seq.size(0);
    const void* kc = nullptr;
    const void* vc = nullptr;
    const int* bt = nullptr;
    const int* cl = nullptr;
    int block_size = 0, max_blocks = 0;
    if (cached_lens.has_value() && cached_lens->defined()) {
        TORCH_CHECK(k_cache.has_value() && block_tables.has_value());
        TORCH_CHECK(cached_lens->scalar_type() == torch::kInt32);
        TORCH_CHECK(block_tables->scalar_type() == torch::kInt32 &&
                    block_tables->is_contiguous());
        TORCH_CHECK(k_cache->is_contiguous() && v_cache->is_contiguous());
        kc = k_cache->data_ptr();
        vc = v_cache->data_ptr();
        bt = block_tables->data_ptr<int>();
        cl = cached_lens->data_ptr<int>();
        block_size = k_cache->size(2);
        max_blocks = block_tables->size(1);
    }
    CHECK_HIP(launch_attention_prefill(
        out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        cu_seqlens.data_ptr<int>(), tile_seq.data_ptr<int>(),
        tile_off.data_ptr<int>(), ntiles, (float)scale, q.size(1), k.size(1),
        q.size(2), q.stride(0), k.stride(0), v.stride(0), kc, vc,
        kc ? scale_ptr(k_scale) : nullptr, vc ? scale_ptr(v_scale) : nullptr,
        bt, cl, block_size, max_blocks, (int)window, current_stream()));
}

void sample(torch::Tensor out, torch::Tensor logits, torch::Tensor temperature,
            c10::optional<torch::Tensor> noise) {
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32 &&
                logits.is_contiguous());
    TORCH_CHECK(out.scalar_type() == torch::kInt64);
    TORCH_CHECK(temperature.scalar_type() == torch::kFloat32);
    const float* noise_ptr = nullptr;
    if (noise.has_value() && noise->defined()) {
        TORCH_CHECK(noise->is_contiguous() && noise->scalar_type() == torch::kFloat32);
        noise_ptr = noise->data_ptr<float>();
    }
    const int B = logits.size(0);
    auto part_val = torch::empty(
        {B, 16}, torch::TensorOptions().dtype(torch::kFloat32).device(logits.device()));
    auto part_idx = torch::empty(
        {B, 16}, torch::TensorOptions().dtype(torch::kInt32).device(logits.device()));
    CHECK_HIP(launch_sample(out.data_ptr<int64_t>(), logits.data_ptr<float>(),
                            temperature.data_ptr<float>(), noise_ptr,
                            part_val.data_ptr<float>(), part_idx.data_ptr<int>(),
                            B, logits.size(1), current_stream()));
}

void topk_topp_filter(torch::Tensor logits, torch::Tensor topp, torch::Tensor topk) {
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32 &&
                logits.is_contiguous() && logits.dim() == 2);
    TORCH_CHECK(topp.scalar_type() == torch::kFloat32 && topp.is_contiguous());
    TORCH_CHECK(topk.scalar_type() == torch::kInt32 && topk.is_contiguous());
    const int B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(topp.numel() == B && topk.numel() == B);
    CHECK_HIP(launch_topk_topp_filter(logits.data_ptr<float>(),
                                      topp.data_ptr<float>(),
                                      topk.data_ptr<int>(), B, V,
                                      current_stream()));
}

// optional fp32 split-K slab workspace: nullptr when absent
float* workspace_ptr(const c10::optional<torch::Tensor>& ws, int64_t numel) {
    if (!ws.has_value() || !ws->defined()) return nullptr;
    TORCH_CHECK(ws->is_cuda() && ws->scalar_type() == torch::kFloat32 &&
                ws->is_contiguous() && ws->numel() >= numel,
                "workspace must be fp32 with >= nsk*M*N elements");
    return ws->data_ptr<float>();
}

// The fused split-K reduce + residual add + RMSNorm tail: residual is
// updated in place, out receives the normed rows and y is not written.
// All three tensors or none; all pointers null when absent.
struct NormTail {
    void* residual = nullptr;
    void* norm_weight = nullptr;
    void* out = nullptr;
};

NormTail norm_tail(const c10::optional<torch::Tensor>& residual,
                   const c10::optional<torch::Tensor>& norm_weight,
                   const c10::optional<torch::Tensor>& out, int M, int N,
                   int64_t nsk, const float* ws) {
    NormTail t;
    if (!residual.has_value() && !norm_weight.has_value() && !out.has_value())
        return t;
    TORCH_CHECK(residual.has_value() && norm_weight.has_value() &&
                out.has_value(),
                "residual, norm_weight and out go together");
    TORCH_CHECK(nsk > 1 && ws != nullptr,
                "fused reduce+norm needs split-K (nsk > 1) slabs");
    check_bf16(*residual, "residual");
    check_bf16(*norm_weight, "norm_weight");
    check_bf16(*out, "out");
    TORCH_CHECK(residual->is_contiguous() && out->is_contiguous() &&
                norm_weight->is_contiguous());
    TORCH_CHECK(residual->dim() == 2 && residual->size(0) == M &&
                residual->size(1) == N && out->dim() == 2 &&
                out->size(0) == M && out->size(1) == N &&
                norm_weight->numel() == N,
                "residual/out must be [M, N], norm_weight [N]");
    TORCH_CHECK(gemm_reduce_rmsnorm_covers(N),
                "fused reduce+norm covers N % 512 == 0, N <= 8192");
    t.residual = residual->data_ptr();
    t.norm_weight = norm_weight->data_ptr();
    t.out = out->data_ptr();
    return t;
}

void gemm_skinny(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                 c10::optional<torch::Tensor> workspace, int64_t nsk,
                 bool swizzled) {
    check_bf16(x, "x");
    check_bf16(w, "w");
    check_bf16(y, "y");
    TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
    const int M = x.size(0), K = x.size(1);
    int N;
    if (swizzled) {  // w is [K/32, N, 32]
        TORCH_CHECK(w.dim() == 3 && w.size(0) == K / 32 && w.size(2) == 32);
        N = w.size(1);
    } else {
        TORCH_CHECK(w.dim() == 2 && w.size(1) == K);
        N = w.size(0);
    }
    TORCH_CHECK(y.size(0) == M && y.size(1) == N);
    float* ws = workspace_ptr(workspace, nsk * (int64_t)M * N);
    CHECK_HIP(launch_gemm_skinny(y.data_ptr(), ws, x.data_ptr(), w.data_ptr(),
                                 M, N, K, (int)nsk, swizzled ? 1 : 0,
                                 current_stream()));
}

void gemm_m256(torch::Tensor y, torch::Tensor x, torch::Tensor w_frag,
               c10::optional<torch::Tensor> workspace, int64_t nsk,
               int64_t nf, int64_t variant, int64_t pipe, int64_t swiglu,
               c10::optional<torch::Tensor> residual,
               c10::optional<torch::Tensor> norm_weight, double eps,
               c10::optional<torch::Tensor> out) {
    check_bf16(x, "x");
    check_bf16(w_frag, "w_frag");
    check_bf16(y, "y");
    TORCH_CHECK(x.is_contiguous() && w_frag.is_contiguous() && y.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
    const int M = x.size(0), K = x.size(1);
    // fragment-major twin: [K/32, N/16, 64, 8]
    TORCH_CHECK(w_frag.dim() == 4 && w_frag.size(0) == K / 32 &&
                w_frag.size(2) == 64 && w_frag.size(3) == 8,
                "w_frag must be the fragment-major [K/32, N/16, 64, 8] twin");
    const int N = w_frag.size(1) * 16;
    // fused swiglu epilogue: w_frag is the block-16 interleaved gate/up
    // twin and y holds silu(gate)*up, half the columns
    TORCH_CHECK(y.size(0) == M && y.size(1) == (swiglu ? N / 2 : N));
    float* ws = workspace_ptr(workspace, nsk * (int64_t)M * N);
    TORCH_CHECK(!(swiglu && (residual.has_value() || norm_weight.has_value() ||
                             out.has_value())),
                "fused reduce+norm needs split-K (nsk > 1) slabs");
    const NormTail t = norm_tail(residual, norm_weight, out, M, N, nsk, ws);
    CHECK_HIP(launch_gemm_m256(y.data_ptr(), ws, x.data_ptr(),
                               w_frag.data_ptr(), M, N, K, (int)nsk, (int)nf,
                               (int)variant, (int)pipe, (int)swiglu,
                               t.residual, t.norm_weight, (float)eps, t.out,
                               current_stream()));
}

// fragment-major fp8 weight twin [K/64, N/16, 64, 16] (uint8 e4m3 bits) and
// its per-output-channel fp32 scale [N]; returns N
int check_w8(const torch::Tensor& q_frag, const torch::Tensor& scale, int K) {
    TORCH_CHECK(q_frag.is_cuda() && scale.is_cuda(), "q_frag/scale must be on GPU");
    TORCH_CHECK(q_frag.scalar_type() == torch::kUInt8,
                "q_frag must be uint8 (e4m3 bits)");
    TORCH_CHECK(scale.scalar_type() == torch::kFloat32, "scale must be fp32");
    TORCH_CHECK(q_frag.is_contiguous() && scale.is_contiguous());
    TORCH_CHECK(K > 0 && K % 64 == 0, "K must be a positive multiple of 64");
    TORCH_CHECK(q_frag.dim() == 4 && q_frag.size(0) == K / 64 &&
                q_frag.size(2) == 64 && q_frag.size(3) == 16,
                "q_frag must be the fragment-major [K/64, N/16, 64, 16] twin");
    const int N = q_frag.size(1) * 16;
    TORCH_CHECK(N > 0 && N % 64 == 0, "N must be a positive multiple of 64");
    TORCH_CHECK(scale.dim() == 1 && scale.numel() == N,
                "scale must hold one fp32 per output channel ([N])");
    return N;
}

void gemm_w8(torch::Tensor y, torch::Tensor x, torch::Tensor q_frag,
             torch::Tensor scale, c10::optional<torch::Tensor> workspace,
             int64_t nsk, c10::optional<torch::Tensor> residual,
             c10::optional<torch::Tensor> norm_weight, double eps,
             c10::optional<torch::Tensor> out) {
    check_bf16(x, "x");
    check_bf16(y, "y");
    TORCH_CHECK(x.is_contiguous() && y.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
    const int M = x.size(0), K = x.size(1);
    TORCH_CHECK(M >= 1 && M <= 256, "gemm_w8 covers 1 <= M <= 256");
    const int N = check_w8(q_frag, scale, K);
    TORCH_CHECK(y.size(0) == M && y.size(1) == N);
    TORCH_CHECK(nsk >= 1 && nsk <= K / 64, "nsk must be in [1, K/64]");
    float* ws = workspace_ptr(workspace, nsk * (int64_t)M * N);
    TORCH_CHECK(nsk == 1 || ws != nullptr, "split-K needs a workspace");
    const NormTail t = norm_tail(residual, norm_weight, out, M, N, nsk, ws);
    CHECK_HIP(launch_gemm_w8(y.data_ptr(), ws, x.data_ptr(), q_frag.data_ptr(),
                             scale.data_ptr<float>(), M, N, K, (int)nsk,
                             t.residual, t.norm_weight, (float)eps, t.out,
                             current_stream()));
}

// The macro-tile quantised bindings differ in the weight check and the
// launcher only: q_frag with its second operand w2 (fp8: channel scales,
// MXFP4: block scales).
template <class Launch>
void gemm_quant_m256(const char* op,
                     int (*check_w)(const torch::Tensor&, const torch::Tensor&, int),
                     Launch launch, torch::Tensor& y, const torch::Tensor& x,
                     const torch::Tensor& q_frag, const torch::Tensor& w2,
                     const c10::optional<torch::Tensor>& workspace, int64_t nsk,
                     int64_t nf, const c10::optional<torch::Tensor>& residual,
                     const c10::optional<torch::Tensor>& norm_weight, double eps,
                     const c10::optional<torch::Tensor>& out) {
    check_bf16(x, "x");
    check_bf16(y, "y");
    TORCH_CHECK(x.is_contiguous() && y.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
    const int M = x.size(0), K = x.size(1);
    TORCH_CHECK(M >= 1 && M <= 256, op, " covers 1 <= M <= 256");
    const int N = check_w(q_frag, w2, K);
    TORCH_CHECK(y.size(0) == M && y.size(1) == N);
    TORCH_CHECK(nf == 4 || nf == 8, "nf must be 4 or 8");
    TORCH_CHECK(N % (16 * nf) == 0, "N must be a multiple of 16*nf");
    // nsk may exceed K/64: a slice without k-tiles writes zeros
    TORCH_CHECK(nsk >= 1 && nsk <= 64, "nsk must be in [1, 64]");
    float* ws = workspace_ptr(workspace, nsk * (int64_t)M * N);
    TORCH_CHECK(nsk == 1 || ws != nullptr, "split-K needs a workspace");
    const NormTail t = norm_tail(residual, norm_weight, out, M, N, nsk, ws);
    CHECK_HIP(launch(y.data_ptr(), ws, x.data_ptr(), q_frag.data_ptr(),
                     w2.data_ptr(), M, N, K, (int)nsk, (int)nf, t.residual,
                     t.norm_weight, (float)eps, t.out, current_stream()));
}

void gemm_w8_m256(torch::Tensor y, torch::Tensor x, torch::Tensor q_frag,
                  torch::Tensor scale, c10::optional<torch::Tensor> workspace,
                  int64_t nsk, int64_t nf,
                  c10::optional<torch::Tensor> residual,
                  c10::optional<torch::Tensor> norm_weight, double eps,
                  c10::optional<torch::Tensor> out) {
    gemm_quant_m256(
        "gemm_w8_m256", check_w8,
        [](void* y, float* ws, const void* x, const void* q, const void* s,
           auto... rest) {
            return launch_gemm_w8_m256(y, ws, x, q, (const float*)s, rest...);
        },
        y, x, q_frag, scale, workspace, nsk, nf, residual, norm_weight, eps, out);
}

void dequant_w8(torch::Tensor out, torch::Tensor q_frag, torch::Tensor scale) {
    check_bf16(out, "out");
    TORCH_CHECK(out.is_contiguous() && out.dim() == 2);
    const int K = out.size(1);
    const int N = check_w8(q_frag, scale, K);
    TORCH_CHECK(out.size(0) == N, "out must be [N, K]");
    CHECK_HIP(launch_dequant_w8(out.data_ptr(), q_frag.data_ptr(),
                                scale.data_ptr<float>(), N, K,
                                current_stream()));
}

// fragment-major MXFP4 weight twin: nibbles [K/64, N/16, 64, 8] (two e2m1
// per byte) and e8m0 block scales [K/64, N/64, 16, 8], both uint8; returns N
int check_w4(const torch::Tensor& q_frag, const torch::Tensor& s_frag, int K) {
    TORCH_CHECK(q_frag.is_cuda() && s_frag.is_cuda(), "q_frag/s_frag must be on GPU");
    TORCH_CHECK(q_frag.scalar_type() == torch::kUInt8,
                "q_frag must be uint8 (packed e2m1 nibbles)");
    TORCH_CHECK(s_frag.scalar_type() == torch::kUInt8,
                "s_frag must be uint8 (e8m0 block scales)");
    TORCH_CHECK(q_frag.is_contiguous() && s_frag.is_contiguous());
    TORCH_CHECK(K > 0 && K % 64 == 0, "K must be a positive multiple of 64");
    TORCH_CHECK(q_frag.dim() == 4 && q_frag.size(0) == K / 64 &&
                q_frag.size(2) == 64 && q_frag.size(3) == 8,
                "q_frag must be the fragment-major [K/64, N/16, 64, 8] twin");
    const int N = q_frag.size(1) * 16;
    TORCH_CHECK(N > 0 && N % 64 == 0, "N must be a positive multiple of 64");
    TORCH_CHECK(s_frag.dim() == 4 && s_frag.size(0) == K / 64 &&
                s_frag.size(1) == N / 64 && s_frag.size(2) == 16 &&
                s_frag.size(3) == 8,
                "s_frag must hold one scale per 32 k of every row "
                "([K/64, N/64, 16, 8])");
    return N;
}

void gemm_w4(torch::Tensor y, torch::Tensor x, torch::Tensor q_frag,
             torch::Tensor s_frag, c10::optional<torch::Tensor> workspace,
             int64_t nsk, c10::optional<torch::Tensor> residual,
             c10::optional<torch::Tensor> norm_weight, double eps,
             c10::optional<torch::Tensor> out) {
    check_bf16(x, "x");
    check_bf16(y, "y");
    TORCH_CHECK(x.is_contiguous() && y.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
    const int M = x.size(0), K = x.size(1);
    TORCH_CHECK(M >= 1 && M <= 256, "gemm_w4 covers 1 <= M <= 256");
    const int N = check_w4(q_frag, s_frag, K);
    TORCH_CHECK(y.size(0) == M && y.size(1) == N);
    TORCH_CHECK(nsk >= 1 && nsk <= K / 64, "nsk must be in [1, K/64]");
    float* ws = workspace_ptr(workspace, nsk * (int64_t)M * N);
    TORCH_CHECK(nsk == 1 || ws != nullptr, "split-K needs a workspace");
    const NormTail t = norm_tail(residual, norm_weight, out, M, N, nsk, ws);
    CHECK_HIP(launch_gemm_w4(y.data_ptr(), ws, x.data_ptr(), q_frag.data_ptr(),
                             s_frag.data_ptr(), M, N, K, (int)nsk, t.residual,
                             t.norm_weight, (float)eps, t.out,
                             current_stream()));
}

void gemm_w4_m256(torch::Tensor y, torch::Tensor x, torch::Tensor q_frag,
                  torch::Tensor s_frag, c10::optional<torch::Tensor> workspace,
                  int64_t nsk, int64_t nf,
                  c10::optional<torch::Tensor> residual,
                  c10::optional<torch::Tensor> norm_weight, double eps,
                  c10::optional<torch::Tensor> out) {
    gemm_quant_m256("gemm_w4_m256", check_w4, launch_gemm_w4_m256, y, x, q_frag,
                    s_frag, workspace, nsk, nf, residual, norm_weight, eps, out);
}

void dequant_w4(torch::Tensor out, torch::Tensor q_frag, torch::Tensor s_frag) {
    check_bf16(out, "out");
    TORCH_CHECK(out.is_contiguous() && out.dim() == 2);
    const int K = out.size(1);
    const int N = check_w4(q_frag, s_frag, K);
    TORCH_CHECK(out.size(0) == N, "out must be [N, K]");
    CHECK_HIP(launch_dequant_w4(out.data_ptr(), q_frag.data_ptr(),
                                s_frag.data_ptr(), N, K, current_stream()));
}

// per-slot / per-row int32 metadata of the LoRA kernels
void check_lora_meta(const torch::Tensor& ranks, const torch::Tensor& adapter_ids,
                     int64_t S, int64_t T) {
    TORCH_CHECK(ranks.is_cuda() && adapter_ids.is_cuda(),
                "ranks/adapter_ids must be on GPU");
    TORCH_CHECK(ranks.scalar_type() == torch::kInt32 && ranks.is_contiguous() &&
                ranks.numel() == S, "ranks must be int32 [S]");
    TORCH_CHECK(adapter_ids.scalar_type() == torch::kInt32 &&
                adapter_ids.is_contiguous() && adapter_ids.numel() == T,
                "adapter_ids must be int32 [T]");
}

void lora_shrink(torch::Tensor t, torch::Tensor x, torch::Tensor A,
                 torch::Tensor ranks, torch::Tensor adapter_ids, int64_t nseg) {
    check_bf16(x, "x");
    check_bf16(A, "A");
    TORCH_CHECK(x.is_contiguous() && A.is_contiguous() && t.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && A.dim() == 3 && t.dim() == 2);
    const int64_t T = x.size(0), K = x.size(1), S = A.size(0);
    TORCH_CHECK(nseg >= 1 && nseg <= 3, "nseg must be 1, 2 or 3");
    TORCH_CHECK(A.size(2) == K, "A must be [S, nseg*R, K]");
    TORCH_CHECK(A.size(1) % nseg == 0, "A rows must be nseg * R");
    const int64_t R = A.size(1) / nseg;
    TORCH_CHECK(R >= 8 && R <= 64 && R % 8 == 0,
                "R must be a multiple of 8, at most 64");
    TORCH_CHECK(K % 64 == 0 && K <= 32768,
                "K must be a multiple of 64, at most 32768");
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                t.size(0) == T && t.size(1) == nseg * R,
                "t must be fp32 [T, nseg*R]");
    check_lora_meta(ranks, adapter_ids, S, T);
    CHECK_HIP(launch_lora_shrink(t.data_ptr<float>(), x.data_ptr(), A.data_ptr(),
                                 ranks.data_ptr<int>(),
                                 adapter_ids.data_ptr<int>(), (int)T, (int)S,
                                 (int)R, (int)nseg, (int)K, current_stream()));
}

// b1/b2: first column of segment 1 / 2 (N where the segment does not exist)
void lora_expand(torch::Tensor y, torch::Tensor t, torch::Tensor B,
                 torch::Tensor ranks, torch::Tensor scales,
                 torch::Tensor adapter_ids, int64_t nseg, int64_t b1,
                 int64_t b2) {
    check_bf16(y, "y");
    check_bf16(B, "B");
    TORCH_CHECK(y.is_contiguous() && B.is_contiguous() && t.is_contiguous());
    TORCH_CHECK(y.dim() == 2 && B.dim() == 3 && t.dim() == 2);
    const int64_t T = y.size(0), N = y.size(1), S = B.size(0), R = B.size(2);
    TORCH_CHECK(B.size(1) == N, "B must be [S, N, R]");
    TORCH_CHECK(N % 64 == 0, "N must be a multiple of 64");
    TORCH_CHECK(R >= 8 && R <= 64 && R % 8 == 0,
                "R must be a multiple of 8, at most 64");
    TORCH_CHECK(nseg >= 1 && nseg <= 3, "nseg must be 1, 2 or 3");
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                t.size(0) == T && t.size(1) == nseg * R,
                "t must be fp32 [T, nseg*R]");
    TORCH_CHECK(0 < b1 && b1 <= b2 && b2 <= N && b1 % 8 == 0 && b2 % 8 == 0,
                "segment bounds must be ascending multiples of 8 within N");
    TORCH_CHECK((nseg >= 2 || b1 == N) && (nseg >= 3 || b2 == N),
                "a segment that does not exist starts at N");
    TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat32 &&
                scales.is_contiguous() && scales.numel() == S,
                "scales must be fp32 [S]");
    check_lora_meta(ranks, adapter_ids, S, T);
    CHECK_HIP(launch_lora_expand(y.data_ptr(), t.data_ptr<float>(), B.data_ptr(),
                                 ranks.data_ptr<int>(), scales.data_ptr<float>(),
                                 adapter_ids.data_ptr<int>(), (int)T, (int)S,
                                 (int)R, (int)nseg, (int)N, (int)b1, (int)b2,
                                 current_stream()));
}

// ---- segmented multi-LoRA (lora_seg.hip) ----
void check_i32(const torch::Tensor& t, const char* name);

int64_t lora_pick_mf_py(int64_t T, int64_t S) {
    return lora_pick_mf((int)T, (int)S);
}

int64_t lora_pick_nsk_py(int64_t T, int64_t mf, int64_t nseg, int64_t K) {
    return lora_pick_nsk((int)T, (int)mf, (int)nseg, (int)K);
}

void lora_align(torch::Tensor sorted_rows, torch::Tensor tile_slot,
                torch::Tensor adapter_ids, torch::Tensor ranks, int64_t mf) {
    check_i32(sorted_rows, "sorted_rows");
    check_i32(tile_slot, "tile_slot");
    check_i32(adapter_ids, "adapter_ids");
    check_i32(ranks, "ranks");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4, "mf must be 1, 2 or 4");
    const int64_t T = adapter_ids.numel(), S = ranks.numel(), BM = 16 * mf;
    const int64_t tiles = tile_slot.numel();
    TORCH_CHECK(S >= 1 && S <= 64, "lora_align supports 1 <= S <= 64, got ", S);
    TORCH_CHECK(T > 0 && tiles * BM >= T + S * (BM - 1) &&
                sorted_rows.numel() == tiles * BM,
                "sorted_rows [cap] / tile_slot [cap / BM] too small for ", T,
                " rows of ", S, " slots");
    CHECK_HIP(launch_lora_align(sorted_rows.data_ptr<int>(),
                                tile_slot.data_ptr<int>(),
                                adapter_ids.data_ptr<int>(),
                                ranks.data_ptr<int>(), (int)T, (int)S, (int)mf,
                                (int)tiles, current_stream()));
}

// the plan and the partial-t scratch [nsk, cap, nseg*R] of both kernels
int64_t check_lora_seg(const torch::Tensor& tpart, const torch::Tensor& sorted_rows,
                       const torch::Tensor& tile_slot, const torch::Tensor& ranks,
                       int64_t S, int64_t R, int64_t nseg, int64_t mf) {
    check_i32(sorted_rows, "sorted_rows");
    check_i32(tile_slot, "tile_slot");
    check_i32(ranks, "ranks");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4, "mf must be 1, 2 or 4");
    TORCH_CHECK(nseg >= 1 && nseg <= 3, "nseg must be 1, 2 or 3");
    TORCH_CHECK(R >= 8 && R <= 64 && R % 8 == 0,
                "R must be a multiple of 8, at most 64");
    TORCH_CHECK(S >= 1 && S <= 64 && ranks.numel() == S, "ranks must be int32 [S <= 64]");
    const int64_t tiles = tile_slot.numel();
    TORCH_CHECK(tiles >= 1 && sorted_rows.numel() == tiles * 16 * mf,
                "sorted_rows must be [tiles * 16 * mf]");
    TORCH_CHECK(tpart.is_cuda() && tpart.scalar_type() == torch::kFloat32 &&
                tpart.is_contiguous() && tpart.dim() == 3 &&
                tpart.size(0) >= 1 && tpart.size(1) == tiles * 16 * mf &&
                tpart.size(2) == nseg * R &&
                reinterpret_cast<uintptr_t>(tpart.data_ptr()) % 16 == 0,
                "tpart must be fp32 [nsk, cap, nseg*R], 16-byte aligned");
    return tiles;
}

void lora_shrink_seg(torch::Tensor tpart, torch::Tensor x, torch::Tensor A,
                     torch::Tensor sorted_rows, torch::Tensor tile_slot,
                     torch::Tensor ranks, int64_t nseg, int64_t mf) {
    check_bf16(x, "x");
    check_bf16(A, "A");
    TORCH_CHECK(x.is_contiguous() && A.is_contiguous());
    TORCH_CHECK(x.dim() == 2 && A.dim() == 3 && x.size(0) >= 1);
    const int64_t K = x.size(1), S = A.size(0);
    TORCH_CHECK(nseg >= 1 && A.size(2) == K && A.size(1) % nseg == 0,
                "A must be [S, nseg*R, K]");
    const int64_t R = A.size(1) / nseg;
    TORCH_CHECK(K % 64 == 0, "K must be a multiple of 64");
    const int64_t tiles =
        check_lora_seg(tpart, sorted_rows, tile_slot, ranks, S, R, nseg, mf);
    CHECK_HIP(launch_lora_shrink_seg(
        tpart.data_ptr<float>(), x.data_ptr(), A.data_ptr(),
        sorted_rows.data_ptr<int>(), tile_slot.data_ptr<int>(),
        ranks.data_ptr<int>(), (int)S, (int)R, (int)nseg, (int)K, (int)mf,
        (int)tiles, (int)tpart.size(0), current_stream()));
}

// b1/b2: first column of segment 1 / 2 (N where the segment does not exist)
void lora_expand_seg(torch::Tensor y, torch::Tensor tpart, torch::Tensor B,
                     torch::Tensor sorted_rows, torch::Tensor tile_slot,
                     torch::Tensor ranks, torch::Tensor scales, int64_t nseg,
                     int64_t b1, int64_t b2, int64_t mf) {
    check_bf16(y, "y");
    check_bf16(B, "B");
    TORCH_CHECK(y.is_contiguous() && B.is_contiguous());
    TORCH_CHECK(y.dim() == 2 && B.dim() == 3);
    const int64_t N = y.size(1), S = B.size(0), R = B.size(2);
    TORCH_CHECK(B.size(1) == N, "B must be [S, N, R]");
    TORCH_CHECK(N % 16 == 0, "N must be a multiple of 16");
    TORCH_CHECK(0 < b1 && b1 <= b2 && b2 <= N && b1 % 16 == 0 && b2 % 16 == 0,
                "segment bounds must be ascending multiples of 16 within N");
    TORCH_CHECK((nseg >= 2 || b1 == N) && (nseg >= 3 || b2 == N),
                "a segment that does not exist starts at N");
    TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat32 &&
                scales.is_contiguous() && scales.numel() == S,
                "scales must be fp32 [S]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0,
                "y must be 8-byte aligned");
    const int64_t tiles =
        check_lora_seg(tpart, sorted_rows, tile_slot, ranks, S, R, nseg, mf);
    CHECK_HIP(launch_lora_expand_seg(
        y.data_ptr(), tpart.data_ptr<float>(), B.data_ptr(),
        sorted_rows.data_ptr<int>(), tile_slot.data_ptr<int>(),
        ranks.data_ptr<int>(), scales.data_ptr<float>(), (int)S, (int)R,
        (int)nseg, (int)N, (int)b1, (int)b2, (int)mf, (int)tiles,
        (int)tpart.size(0), current_stream()));
}

// ---- mixture of experts (moe.hip, moe_prefill.hip, moe_w4.hip, moe_w8.hip) ----
void check_moe_shape(int64_t E, int64_t k) {
    TORCH_CHECK(E >= 2 && E <= 64, "MoE kernels support 2 <= num_experts <= 64, got ", E);
    TORCH_CHECK(k >= 1 && k <= 8 && k <= E,
                "MoE kernels support 1 <= experts_per_token <= min(num_experts, 8), got ", k);
}

void check_i32(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous(),
                name, " must be a contiguous int32 GPU tensor");
}

int64_t moe_pick_mf_py(int64_t T, int64_t k, int64_t E) {
    return moe_pick_mf((int)T, (int)k, (int)E);
}

void moe_route(torch::Tensor ids, torch::Tensor weights, torch::Tensor x,
               torch::Tensor w_router) {
    check_bf16(x, "x");
    check_bf16(w_router, "w_router");
    TORCH_CHECK(x.dim() == 2 && w_router.dim() == 2 && x.is_contiguous() &&
                w_router.is_contiguous() && w_router.size(1) == x.size(1),
                "x [T, H] and w_router [E, H] must be contiguous");
    const int64_t T = x.size(0), H = x.size(1), E = w_router.size(0);
    check_i32(ids, "ids");
    TORCH_CHECK(ids.dim() == 2 && ids.size(0) == T, "ids must be int32 [T, k]");
    const int64_t k = ids.size(1);
    check_moe_shape(E, k);
    TORCH_CHECK(H % 64 == 0 && H <= 8192, "moe_route needs H % 64 == 0 and H <= 8192, got ", H);
    TORCH_CHECK(weights.is_cuda() && weights.scalar_type() == torch::kFloat32 &&
                weights.is_contiguous() && weights.sizes() == ids.sizes(),
                "weights must be fp32 [T, k]");
    CHECK_HIP(launch_moe_route(ids.data_ptr<int>(), weights.data_ptr<float>(),
                               x.data_ptr(), w_router.data_ptr(), (int)T, (int)H,
                               (int)E, (int)k, current_stream()));
}

void moe_align(torch::Tensor sorted_pairs, torch::Tensor tile_expert,
               torch::Tensor ids, int64_t E, int64_t mf) {
    check_i32(sorted_pairs, "sorted_pairs");
    check_i32(tile_expert, "tile_expert");
    check_i32(ids, "ids");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4 || mf == 8, "mf must be 1, 2, 4 or 8");
    TORCH_CHECK(E >= 2 && E <= 64, "MoE kernels support 2 <= num_experts <= 64, got ", E);
    const int64_t P = ids.numel(), BM = 16 * mf, tiles = tile_expert.numel();
    TORCH_CHECK(P > 0 && tiles * BM >= P + E * (BM - 1) &&
                sorted_pairs.numel() == tiles * BM,
                "sorted_pairs [cap] / tile_expert [cap / BM] too small for ", P,
                " pairs of ", E, " experts");
    CHECK_HIP(launch_moe_align(sorted_pairs.data_ptr<int>(),
                               tile_expert.data_ptr<int>(), ids.data_ptr<int>(),
                               (int)P, (int)E, (int)mf, (int)tiles,
                               current_stream()));
}

// epi 0: out = act [cap, I], a = x [T, H], w packed [E, H/32, 2I/16, 64, 8]
// epi 1: out = y_pair [P, H], a = act [cap, I], w packed [E, I/32, H/16, 64, 8]
void moe_gemm(torch::Tensor out, torch::Tensor a, torch::Tensor w,
              torch::Tensor sorted_pairs, torch::Tensor tile_expert,
              c10::optional<torch::Tensor> rweights, int64_t epi, int64_t mf,
              int64_t k, int64_t P) {
    check_bf16(out, "out");
    check_bf16(a, "a");
    check_bf16(w, "w");
    check_i32(sorted_pairs, "sorted_pairs");
    check_i32(tile_expert, "tile_expert");
    TORCH_CHECK(epi == 0 || epi == 1, "epi must be 0 (swiglu) or 1 (down)");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4 || mf == 8, "mf must be 1, 2, 4 or 8");
    TORCH_CHECK(out.is_contiguous() && a.is_contiguous() && w.is_contiguous() &&
                out.dim() == 2 && a.dim() == 2);
    TORCH_CHECK(w.dim() == 5 && w.size(3) == 64 && w.size(4) == 8,
                "w must be packed [E, K/32, N/16, 64, 8] (ops.moe_pack_weights)");
    const int64_t E = w.size(0), K = w.size(1) * 32, N = w.size(2) * 16;
    const int64_t BM = 16 * mf, tiles = tile_expert.numel(), cap = tiles * BM;
    check_moe_shape(E, k);
    TORCH_CHECK(sorted_pairs.numel() == cap, "sorted_pairs must be [cap]");
    TORCH_CHECK(K % 64 == 0 && a.size(1) == K, "a must be [rows, K] with K % 64 == 0");
    // P = T * k pairs; only the down epilogue reads the routing weights
    const float* rw = nullptr;
    if (epi == 1) {
        TORCH_CHECK(rweights.has_value() && rweights->is_cuda() &&
                    rweights->scalar_type() == torch::kFloat32 &&
                    rweights->is_contiguous() && rweights->numel() == P,
                    "weights must be fp32 [T, k]");
        rw = rweights->data_ptr<float>();
    }
    TORCH_CHECK(P > 0 && P % k == 0 && cap >= P + E * (BM - 1),
                "cap too small for the pairs");
    if (epi == 0) {
        TORCH_CHECK(N % 128 == 0, "intermediate size must be a multiple of 64");
        TORCH_CHECK(a.size(0) == P / k, "x must be [T, H]");
        TORCH_CHECK(out.size(0) == cap && out.size(1) == N / 2, "act must be [cap, I]");
    } else {
        TORCH_CHECK(N % (mf == 8 ? 128 : 64) == 0, "hidden size must be a multiple of ",
                    mf == 8 ? 128 : 64, " at mf = ", mf);
        TORCH_CHECK(a.size(0) == cap, "act must be [cap, I]");
        TORCH_CHECK(out.size(0) == P && out.size(1) == N, "y_pair must be [T*k, H]");
    }
    CHECK_HIP(launch_moe_gemm(out.data_ptr(), a.data_ptr(), w.data_ptr(),
                              sorted_pairs.data_ptr<int>(),
                              tile_expert.data_ptr<int>(),
                              rw, (int)epi, (int)mf,
                              (int)tiles, (int)N, (int)K, (int)k,
                              current_stream()));
}

// moe_gemm with MXFP4 expert weights (ops.moe_pack_weights_mxfp4):
// wq [E, K/128, N/16, 64, 16] nibble bytes, ws [E, K/128, N/16, 16, 4] scale
// bytes
void moe_gemm_w4(torch::Tensor out, torch::Tensor a, torch::Tensor wq,
                 torch::Tensor ws, torch::Tensor sorted_pairs,
                 torch::Tensor tile_expert,
                 c10::optional<torch::Tensor> rweights, int64_t epi, int64_t mf,
                 int64_t k, int64_t P) {
    check_bf16(out, "out");
    check_bf16(a, "a");
    check_i32(sorted_pairs, "sorted_pairs");
    check_i32(tile_expert, "tile_expert");
    TORCH_CHECK(wq.is_cuda() && ws.is_cuda() && wq.scalar_type() == torch::kUInt8 &&
                ws.scalar_type() == torch::kUInt8 && wq.device() == a.device() &&
                ws.device() == a.device(),
                "wq / ws must be uint8 tensors on the device of a");
    TORCH_CHECK(epi == 0 || epi == 1, "epi must be 0 (swiglu) or 1 (down)");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4 || mf == 8, "mf must be 1, 2, 4 or 8");
    TORCH_CHECK(out.is_contiguous() && a.is_contiguous() && wq.is_contiguous() &&
                ws.is_contiguous() && out.dim() == 2 && a.dim() == 2);
    TORCH_CHECK(wq.dim() == 5 && wq.size(3) == 64 && wq.size(4) == 16,
                "wq must be packed [E, K/128, N/16, 64, 16] (ops.moe_pack_weights_mxfp4)");
    const int64_t E = wq.size(0), K = wq.size(1) * 128, N = wq.size(2) * 16;
    TORCH_CHECK(ws.dim() == 5 && ws.size(0) == E && ws.size(1) == K / 128 &&
                ws.size(2) == N / 16 && ws.size(3) == 16 && ws.size(4) == 4,
                "ws must be packed [E, K/128, N/16, 16, 4] for the E, N, K of wq");
    const int64_t BM = 16 * mf, tiles = tile_expert.numel(), cap = tiles * BM;
    check_moe_shape(E, k);
    TORCH_CHECK(sorted_pairs.numel() == cap, "sorted_pairs must be [cap]");
    TORCH_CHECK(a.size(1) == K, "a must be [rows, K]");
    // P = T * k pairs; only the down epilogue reads the routing weights
    const float* rw = nullptr;
    if (epi == 1) {
        TORCH_CHECK(rweights.has_value() && rweights->is_cuda() &&
                    rweights->scalar_type() == torch::kFloat32 &&
                    rweights->is_contiguous() && rweights->numel() == P,
                    "weights must be fp32 [T, k]");
        rw = rweights->data_ptr<float>();
    }
    TORCH_CHECK(P > 0 && P % k == 0 && cap >= P + E * (BM - 1),
                "cap too small for the pairs");
    if (epi == 0) {
        TORCH_CHECK(N % 128 == 0, "intermediate size must be a multiple of 64");
        TORCH_CHECK(a.size(0) == P / k, "x must be [T, H]");
        TORCH_CHECK(out.size(0) == cap && out.size(1) == N / 2, "act must be [cap, I]");
    } else {
        TORCH_CHECK(N % (mf == 8 ? 128 : 64) == 0, "hidden size must be a multiple of ",
                    mf == 8 ? 128 : 64, " at mf = ", mf);
        TORCH_CHECK(a.size(0) == cap, "act must be [cap, I]");
        TORCH_CHECK(out.size(0) == P && out.size(1) == N, "y_pair must be [T*k, H]");
    }
    CHECK_HIP(launch_moe_gemm_w4(out.data_ptr(), a.data_ptr(), wq.data_ptr(),
                                 ws.data_ptr(), sorted_pairs.data_ptr<int>(),
                                 tile_expert.data_ptr<int>(), rw, (int)epi,
                                 (int)mf, (int)tiles, (int)N, (int)K, (int)k,
                                 current_stream()));
}

// moe_gemm with fp8 expert weights (ops.moe_pack_weights_fp8): wq
// [E, K/64, N/16, 64, 16] e4m3 bytes, scale [E, N] fp32 (one per output
// channel, in the row order of wq). mf is 1, 2 or 4: there is no 128-row tile
void moe_gemm_w8(torch::Tensor out, torch::Tensor a, torch::Tensor wq,
                 torch::Tensor scale, torch::Tensor sorted_pairs,
                 torch::Tensor tile_expert,
                 c10::optional<torch::Tensor> rweights, int64_t epi, int64_t mf,
                 int64_t k, int64_t P) {
    check_bf16(out, "out");
    check_bf16(a, "a");
    check_i32(sorted_pairs, "sorted_pairs");
    check_i32(tile_expert, "tile_expert");
    TORCH_CHECK(wq.is_cuda() && scale.is_cuda() && wq.scalar_type() == torch::kUInt8 &&
                scale.scalar_type() == torch::kFloat32 && wq.device() == a.device() &&
                scale.device() == a.device(),
                "wq must be a uint8 and scale an fp32 tensor on the device of a");
    TORCH_CHECK(epi == 0 || epi == 1, "epi must be 0 (swiglu) or 1 (down)");
    TORCH_CHECK(mf == 1 || mf == 2 || mf == 4, "mf must be 1, 2 or 4 with fp8 experts");
    TORCH_CHECK(out.is_contiguous() && a.is_contiguous() && wq.is_contiguous() &&
                scale.is_contiguous() && out.dim() == 2 && a.dim() == 2);
    TORCH_CHECK(wq.dim() == 5 && wq.size(3) == 64 && wq.size(4) == 16,
                "wq must be packed [E, K/64, N/16, 64, 16] (ops.moe_pack_weights_fp8)");
    const int64_t E = wq.size(0), K = wq.size(1) * 64, N = wq.size(2) * 16;
    TORCH_CHECK(scale.dim() == 2 && scale.size(0) == E && scale.size(1) == N,
                "scale must be [E, N] for the E, N of wq");
    const int64_t BM = 16 * mf, tiles = tile_expert.numel(), cap = tiles * BM;
    check_moe_shape(E, k);
    TORCH_CHECK(sorted_pairs.numel() == cap, "sorted_pairs must be [cap]");
    TORCH_CHECK(a.size(1) == K, "a must be [rows, K]");
    // P = T * k pairs; only the down epilogue reads the routing weights
    const float* rw = nullptr;
    if (epi == 1) {
        TORCH_CHECK(rweights.has_value() && rweights->is_cuda() &&
                    rweights->scalar_type() == torch::kFloat32 &&
                    rweights->is_contiguous() && rweights->numel() == P,
                    "weights must be fp32 [T, k]");
        rw = rweights->data_ptr<float>();
    }
    TORCH_CHECK(P > 0 && P % k == 0 && cap >= P + E * (BM - 1),
                "cap too small for the pairs");
    if (epi == 0) {
        TORCH_CHECK(N % 128 == 0, "intermediate size must be a multiple of 64");
        TORCH_CHECK(a.size(0) == P / k, "x must be [T, H]");
        TORCH_CHECK(out.size(0) == cap && out.size(1) == N / 2, "act must be [cap, I]");
    } else {
        TORCH_CHECK(N % 64 == 0, "hidden size must be a multiple of 64");
        TORCH_CHECK(a.size(0) == cap, "act must be [cap, I]");
        TORCH_CHECK(out.size(0) == P && out.size(1) == N, "y_pair must be [T*k, H]");
    }
    CHECK_HIP(launch_moe_gemm_w8(out.data_ptr(), a.data_ptr(), wq.data_ptr(),
                                 scale.data_ptr<float>(),
                                 sorted_pairs.data_ptr<int>(),
                                 tile_expert.data_ptr<int>(), rw, (int)epi,
                                 (int)mf, (int)tiles, (int)N, (int)K, (int)k,
                                 current_stream()));
}

void moe_combine_norm(torch::Tensor normed, torch::Tensor residual,
                      torch::Tensor y_pair, torch::Tensor norm_w, double eps,
                      int64_t k) {
    check_bf16(normed, "normed");
    check_bf16(residual, "residual");
    check_bf16(y_pair, "y_pair");
    check_bf16(norm_w, "norm_w");
    TORCH_CHECK(normed.is_contiguous() && residual.is_contiguous() &&
                y_pair.is_contiguous() && norm_w.is_contiguous());
    TORCH_CHECK(residual.dim() == 2 && k >= 1 && k <= 8);
    const int64_t T = residual.size(0), H = residual.size(1);
    TORCH_CHECK(H % 8 == 0 && y_pair.numel() == T * k * H &&
                normed.numel() == T * H && norm_w.numel() == H,
                "moe_combine_norm: y_pair [T*k, H], residual/normed [T, H]");
    CHECK_HIP(launch_moe_combine_norm(normed.data_ptr(), residual.data_ptr(),
                                      y_pair.data_ptr(), norm_w.data_ptr(),
                                      (float)eps, (int)T, (int)H, (int)k,
                                      current_stream()));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("moe_pick_mf", &moe_pick_mf_py, "row-tile factor (BM = 16 mf) for T, k, E");
    m.def("moe_route", &moe_route, "MoE router: softmax top-k ids and weights per row");
    m.def("moe_align", &moe_align, "MoE counting sort of the pairs by expert, BM-padded");
    m.def("moe_gemm", &moe_gemm, "grouped expert GEMM (epi 0: gate_up+swiglu, 1: down)");
    m.def("moe_gemm_w4", &moe_gemm_w4,
          "grouped expert GEMM with MXFP4 expert weights (W4A16)");
    m.def("moe_gemm_w8", &moe_gemm_w8,
          "grouped expert GEMM with fp8 expert weights (W8A16)");
    m.def("moe_combine_norm", &moe_combine_norm,
          "sum of a token's k expert rows + residual add + RMSNorm");
    m.def("lora_shrink", &lora_shrink,
          "batched-gather LoRA shrink t = x @ A[slot].T (fp32), slot per row");
    m.def("lora_expand", &lora_expand,
          "batched-gather LoRA expand y += scale[slot] * t @ B[slot].T in "
          "place, slot per row");
    m.def("lora_pick_mf", &lora_pick_mf_py, "row-tile factor (BM = 16 mf) for T rows, S slots");
    m.def("lora_pick_nsk", &lora_pick_nsk_py, "split-K of lora_shrink_seg for T, mf, nseg, K");
    m.def("lora_align", &lora_align,
          "stable counting sort of the rows by adapter slot, BM-padded");
    m.def("lora_shrink_seg", &lora_shrink_seg,
          "segmented MFMA LoRA shrink into split-K partials [nsk, cap, nseg*R]");
    m.def("lora_expand_seg", &lora_expand_seg,
          "segmented MFMA LoRA expand y += scale[slot] * t @ B[slot].T in place");
    m.def("rmsnorm", &rmsnorm, "RMSNorm (gfx950)");
    m.def("rmsnorm_residual", &rmsnorm_residual, "fused residual-add RMSNorm");
    m.def("rope_inplace", &rope_inplace, "rotate-half RoPE in place");
    m.def("swiglu", &swiglu, "fused SiLU-gate multiply");
    m.def("kv_cache_write", &kv_cache_write, "paged KV cache scatter");
    m.def("rope_kv_write", &rope_kv_write, "fused RoPE + paged KV scatter");
    // window (sliding-window attention) is the one defaulted argument, so
    // every argument is named
    m.def("attention_decode", &attention_decode, "paged decode attention",
          py::arg("out"), py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_tables"), py::arg("context_lens"), py::arg("scale"),
          py::arg("part_acc"), py::arg("part_ml"), py::arg("nsplit"),
          py::arg("k_scale"), py::arg("v_scale"), py::arg("version"),
          py::arg("window") = 0);
    m.def("attention_prefill", &attention_prefill, "varlen causal prefill attention",
          py::arg("out"), py::arg("q"), py::arg("k"), py::arg("v"),
          py::arg("cu_seqlens"), py::arg("tile_seq"), py::arg("tile_off"),
          py::arg("scale"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_tables"), py::arg("cached_lens"), py::arg("k_scale"),
          py::arg("v_scale"), py::arg("window") = 0);
    m.def("sample", &sample, "greedy / gumbel-max sampling");
    m.def("topk_topp_filter", &topk_topp_filter,
          "in-place top-k/top-p logit filtering (histogram threshold)");
    m.def("gemm_skinny", &gemm_skinny,
          "skinny-M weight-streaming GEMM y = x @ w.T (decode projections)");
    m.def("gemm_m256", &gemm_m256,
          "macro-tile LDS-staged decode GEMM y = x @ w.T (M <= 256); with "
          "residual/norm_weight/out the split-K reduce also adds the "
          "residual and RMS-normalizes",
          pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("w_frag"),
          pybind11::arg("workspace"), pybind11::arg("nsk"),
          pybind11::arg("nf"), pybind11::arg("variant"),
          pybind11::arg("pipe"), pybind11::arg("swiglu"),
          pybind11::arg("residual") = pybind11::none(),
          pybind11::arg("norm_weight") = pybind11::none(),
          pybind11::arg("eps") = 1e-5,
          pybind11::arg("out") = pybind11::none());
    m.def("gemm_w8", &gemm_w8,
          "W8A16 skinny decode GEMM y = x @ (scale * q).T (1 <= M <= 256), q "
          "the fragment-major fp8 e4m3 twin; with residual/norm_weight/out "
          "the split-K reduce also adds the residual and RMS-normalizes",
          pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("q_frag"),
          pybind11::arg("scale"), pybind11::arg("workspace"),
          pybind11::arg("nsk"),
          pybind11::arg("residual") = pybind11::none(),
          pybind11::arg("norm_weight") = pybind11::none(),
          pybind11::arg("eps") = 1e-5,
          pybind11::arg("out") = pybind11::none());
    m.def("gemm_w8_m256", &gemm_w8_m256,
          "macro-tile W8A16 decode GEMM y = x @ (scale * q).T (1 <= M <= 256): "
          "the fp8 twin is converted once per workgroup into the LDS tile of "
          "the register-staged gemm_m256 structure; residual/norm_weight/out "
          "as for gemm_w8",
          pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("q_frag"),
          pybind11::arg("scale"), pybind11::arg("workspace"),
          pybind11::arg("nsk"), pybind11::arg("nf"),
          pybind11::arg("residual") = pybind11::none(),
          pybind11::arg("norm_weight") = pybind11::none(),
          pybind11::arg("eps") = 1e-5,
          pybind11::arg("out") = pybind11::none());
    m.def("dequant_w8", &dequant_w8,
          "fragment-major fp8 twin + scale -> row-major bf16 [N, K]");
    m.def("gemm_w4", &gemm_w4,
          "W4A16 skinny decode GEMM y = x @ dequant(q, s).T (1 <= M <= 256), "
          "q/s the fragment-major MXFP4 twin (e2m1 nibbles, e8m0 block-32 "
          "scales); residual/norm_weight/out as for gemm_w8",
          pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("q_frag"),
          pybind11::arg("s_frag"), pybind11::arg("workspace"),
          pybind11::arg("nsk"),
          pybind11::arg("residual") = pybind11::none(),
          pybind11::arg("norm_weight") = pybind11::none(),
          pybind11::arg("eps") = 1e-5,
          pybind11::arg("out") = pybind11::none());
    m.def("gemm_w4_m256", &gemm_w4_m256,
          "macro-tile W4A16 decode GEMM y = x @ dequant(q, s).T (1 <= M <= "
          "256): the MXFP4 twin is converted once per workgroup into the LDS "
          "tile of the register-staged gemm_m256 structure; "
          "residual/norm_weight/out as for gemm_w8",
          pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("q_frag"),
          pybind11::arg("s_frag"), pybind11::arg("workspace"),
          pybind11::arg("nsk"), pybind11::arg("nf"),
          pybind11::arg("residual") = pybind11::none(),
          pybind11::arg("norm_weight") = pybind11::none(),
          pybind11::arg("eps") = 1e-5,
          pybind11::arg("out") = pybind11::none());
    m.def("dequant_w4", &dequant_w4,
          "fragment-major MXFP4 twin -> row-major bf16 [N, K]");

    pybind11::class_<BlockAllocator>(m, "BlockAllocator")
        .def(pybind11::init<int64_t>())
        .def("num_free", &BlockAllocator::num_free)
        .def("allocate", &BlockAllocator::allocate)
        .def("free", &BlockAllocator::free_blocks)
        .def_property_readonly("num_blocks", &BlockAllocator::capacity);
}
