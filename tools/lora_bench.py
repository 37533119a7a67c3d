"""Cold-cache timing of the multi-LoRA kernels (csrc/lora.hip) beside the
base GEMM they follow, on the four decode projection shapes of llama-3-8b.

lora_shrink and lora_expand run over a stack of S = 4 adapters of the given
rank, every row on an adapter, neighbouring rows on different ones. As in
tools/gemm_w8_bench.py each route cycles through enough copies of what it
streams (base weights >= 1.5 GB, adapter stacks >= 768 MB) that no copy is
still in the 256 MB L3 when its turn comes again: in the engine a decode
step streams the whole model between two uses of a layer's stacks. Routes
alternate, three rounds each; the median round is reported with the min-max
of the three. Run on the GPU box:

    python tools/lora_bench.py [--ts=16,64,256] [--ranks=16,64]
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
TS = (16, 64, 256)
RANKS = (16, 64)
S = 4
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


def main():
    assert torch.cuda.is_available() and ops.have_native()
    dev = "cuda:0"
    ts, ranks = TS, RANKS
    for a in sys.argv[1:]:
        if a.startswith("--ts="):
            ts = tuple(int(v) for v in a[5:].split(","))
        if a.startswith("--ranks="):
            ranks = tuple(int(v) for v in a[8:].split(","))
    print(
        "shape, T, rank, base GEMM us, shrink us, expand us, "
        "(shrink+expand)/base, stack MB streamed, max err"
    )
    for name, N, K, bounds in SHAPES:
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
            for T in ts:
                x = (torch.randn(T, K, device=dev) * 0.5).bfloat16()
                ids = (torch.arange(T, device=dev) % S).int()
                y = torch.zeros(T, N, dtype=torch.bfloat16, device=dev)
                t = torch.empty(T, nseg * R, dtype=torch.float32, device=dev)

                def base(i):
                    return ops.linear(x, w16[i % nw], tw[i % nw])

                def shrink(i):
                    j = (i % nl) * S
                    return ops.lora_shrink(x, A[j : j + S], rk, ids, nseg, out=t)

                def expand(i):
                    j = (i % nl) * S
                    return ops.lora_expand(y, t, B[j : j + S], rk, sc, ids, bounds)

                y.zero_()
                shrink(0)
                expand(0)
                stack = ops.LoraStack(A[:S].cpu(), B[:S].cpu(), rk.cpu(), sc.cpu(), bounds)
                ref = ops.lora_add(torch.zeros(T, N), x.cpu(), stack, ids.cpu())
                err = ((y.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()
                a, b, c = rounds(
                    [base, shrink, expand], [2 * nw + 20, 2 * nl + 20, 2 * nl + 20]
                )
                # every row streams its adapter's A and B once (L2 may dedup)
                used = min(T, S) * (nseg * R * K + N * R) * 2
                print(
                    f"{name} ({N}x{K}), {T}, {rank}, {fmt(a)}, {fmt(b)}, {fmt(c)}, "
                    f"{(b[0] + c[0]) / a[0]:.2f}, {used / 2**20:.1f}, {err:.4f}",
                    flush=True,
                )
            del A, B
            torch.cuda.empty_cache()
        del w16, tw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
