"""Cold-cache timing of the multi-LoRA kernels beside the base GEMM they
follow, on the four projection shapes of llama-3-8b: the vector pair
(csrc/lora.hip, one workgroup per row) and the segmented MFMA pair
(csrc/lora_seg.hip, rows sorted by adapter; lora_align is timed on its own:
the model runs it once per forward, not once per projection).

Both pairs run over a stack of S = 8 adapters of the given rank, every row
on an adapter: mix "1" puts all rows on one adapter, mix "8" neighbouring
rows on different ones. As in
tools/gemm_w8_bench.py each route cycles through enough copies of what it
streams (base weights >= 1.5 GB, adapter stacks >= 768 MB) that no copy is
still in the 256 MB L3 when its turn comes again: in the engine a decode
step streams the whole model between two uses of a layer's stacks. Routes
alternate, three rounds each; the median round is reported with the min-max
of the three. Run on the GPU box:

    python tools/lora_bench.py [--ts=16,64,256,1024,4096] [--ranks=16,64]
                               [--mixes=1,8] [--shapes=qkv,o,gate_up,down]
    python tools/lora_bench.py --prefill

--prefill times one 4096-token prefill forward of llama-3-8b (random
weights) with a rank-16 and a rank-64 adapter on all seven targets:
segmented route, vector route (threshold out of reach) and no adapter.
"""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmapigateway_amd import ops

# name, N, K, segment ends
SHAPES = [
    ("8b qkv", 6144, 4096, (4096, 5120, 6144)),
    ("8b o", 4096, 4096, (4096,)),
    ("8b gate_up", 28672, 4096, (14336, 28672)),
    ("8b down", 4096, 14336, (4096,)),
]
TS = (16, 64, 256, 1024, 4096)
RANKS = (16, 64)
S = 8
MIXES = (1, 8)
ROTATE_W = 1536 << 20
ROTATE_L = 768 << 20


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us


def rounds(routes, iters):
    """Three alternating rounds of every route -> [(median, min, max)]."""
    for fn in routes:
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    ts = [[] for _ in routes]
    for _ in range(3):
        for t, fn, n in zip(ts, routes, iters):
            t.append(timed(fn, n))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})"


def prefill(dev, T=4096):
    import copy

    from llmapigateway_amd.engine.kvcache import PagedKVCache
    from llmapigateway_amd.models.configs import get_model_config
    from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel

    cfg = get_model_config("llama-3-8b")
    model = LlamaModel(cfg, device=dev, seed=0, max_loras=1, max_lora_rank=64)
    plain = copy.copy(model)
    plain.max_loras = 0
    kv = PagedKVCache(cfg, T // 16, 16, dev, torch.bfloat16)
    batch = ForwardBatch(
        kind="prefill",
        token_ids=torch.randint(0, cfg.vocab_size, (T,), device=dev),
        positions=torch.arange(T, device=dev),
        slot_mapping=torch.arange(T, device=dev),
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device=dev),
        max_seqlen=T,
        logits_indices=torch.tensor([T - 1], device=dev),
        adapter_ids=torch.zeros(T, dtype=torch.int32, device=dev),
    )
    default = ops.LORA_SEG_MIN_T

    def route(m, min_t):
        def fn(i):
            ops.LORA_SEG_MIN_T = min_t
            return m.forward(batch, kv.k_caches, kv.v_caches)
        return fn

    print(f"prefill T={T} llama-3-8b, ms: rank, no adapter, vector, segmented")
    for rank in (16, 64):
        model.set_adapter(0, model.random_adapter(rank, seed=1), alpha=2.0 * rank)
        res = rounds(
            [route(plain, default), route(model, 1 << 30), route(model, default)],
            [5, 5, 5],
        )
        print(f"{rank}, " + ", ".join(fmt(tuple(v / 1e3 for v in r)) for r in res), flush=True)
    ops.LORA_SEG_MIN_T = default


def main():
    assert torch.cuda.is_available() and ops.have_native()
    dev = "cuda:0"
    if "--prefill" in sys.argv[1:]:
        return prefill(dev)
    ts, ranks, mixes, shapes = TS, RANKS, MIXES, SHAPES
    for a in sys.argv[1:]:
        if a.startswith("--ts="):
            ts = tuple(int(v) for v in a[5:].split(","))
        if a.startswith("--ranks="):
            ranks = tuple(int(v) for v in a[8:].split(","))
        if a.startswith("--mixes="):
            mixes = tuple(int(v) for v in a[8:].split(","))
        if a.startswith("--shapes="):
            shapes = [s for s in SHAPES if s[0].split()[1] in a[9:].split(",")]
    print(
        "shape, T, rank, mix, base GEMM us, shrink us, expand us, "
        "align us, shrink_seg us, expand_seg us, vector/base, seg/base, "
        "vector/seg, max err vector, max err seg"
    )
    for name, N, K, bounds in shapes:
        nseg = len(bounds)
        nw = max(2, -(-ROTATE_W // (N * K * 2)))
        has_twin = ops._m256_config(256, N, K) is not None
        w16 = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(nw)]
        tw = [ops.swizzle_weight_frag(w) if has_twin else None for w in w16]
        for rank in ranks:
            R = ops.lora_padded_rank(rank)
            per = S * (nseg * R * K + N * R) * 2
            nl = max(2, -(-ROTATE_L // per))
            A = (torch.randn(nl * S, nseg * R, K, device=dev) * 0.02).bfloat16()
            B = (torch.randn(nl * S, N, R, device=dev) * 0.02).bfloat16()
            rk = torch.full((S,), rank, dtype=torch.int32, device=dev)
            sc = torch.full((S,), 2.0, dtype=torch.float32, device=dev)
            for T, mix in ((T, mix) for T in ts for mix in mixes):
                x = (torch.randn(T, K, device=dev) * 0.5).bfloat16()
                ids = (torch.arange(T, device=dev) % mix).int()
                y = torch.zeros(T, N, dtype=torch.bfloat16, device=dev)
                t = torch.empty(T, nseg * R, dtype=torch.float32, device=dev)
                plan = ops.lora_align(ids, rk)
                tp = ops.lora_shrink_seg(x, A[:S], rk, ids, nseg, plan).clone()

                def base(i):
                    return ops.linear(x, w16[i % nw], tw[i % nw])

                def shrink(i):
                    j = (i % nl) * S
                    return ops.lora_shrink(x, A[j : j + S], rk, ids, nseg, out=t)

                def expand(i):
                    j = (i % nl) * S
                    return ops.lora_expand(y, t, B[j : j + S], rk, sc, ids, bounds)

                def align(i):
                    return ops.lora_align(ids, rk)

                def shrink_seg(i):
                    j = (i % nl) * S
                    return ops.lora_shrink_seg(x, A[j : j + S], rk, ids, nseg, plan, out=tp)

                def expand_seg(i):
                    j = (i % nl) * S
                    return ops.lora_expand_seg(
                        y, tp, B[j : j + S], rk, sc, ids, bounds, plan
                    )

                stack = ops.LoraStack(A[:S].cpu(), B[:S].cpu(), rk.cpu(), sc.cpu(), bounds)
                ref = ops.lora_add(torch.zeros(T, N), x.cpu(), stack, ids.cpu())
                errs = []
                for sh, ex in ((shrink, expand), (shrink_seg, expand_seg)):
                    y.zero_()
                    sh(0)
                    ex(0)
                    errs.append(
                        ((y.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()
                    )
                n = 2 * nl + 20
                a, b, c, al, d, e = rounds(
                    [base, shrink, expand, align, shrink_seg, expand_seg],
                    [2 * nw + 20, n, n, n, n, n],
                )
                vec, seg = b[0] + c[0], d[0] + e[0]
                print(
                    f"{name} ({N}x{K}), {T}, {rank}, {mix}, {fmt(a)}, {fmt(b)}, {fmt(c)}, "
                    f"{fmt(al)}, {fmt(d)}, {fmt(e)}, {vec / a[0]:.2f}, {seg / a[0]:.2f}, "
                    f"{vec / seg:.2f}, {errs[0]:.4f}, {errs[1]:.4f}",
                    flush=True,
                )
            del A, B
            torch.cuda.empty_cache()
        del w16, tw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
