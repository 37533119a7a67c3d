"""Cold-cache timing of the fp8 (W8A16) decode GEMM route against the bf16
route on the decode projection shapes of llama-3-8b and llama-3-70b.

Each route cycles through enough weight copies (>= 1.5 GB) that no copy
is still in the 256 MB L3 when its turn comes again, as in the engine,
where a decode step streams the whole model between two uses of a
matrix. Routes alternate, three rounds each; the median round is
reported, with the bytes each route has to stream and the rate that
implies. Run on the GPU box:

    python tools/gemm_w8_bench.py [M N K]
"""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmapigateway_amd import ops

SHAPES = [
    ("8b qkv", 6144, 4096),
    ("8b o", 4096, 4096),
    ("8b gate_up", 28672, 4096),
    ("8b down", 4096, 14336),
    ("70b qkv", 10240, 8192),
    ("70b o", 8192, 8192),
    ("70b gate_up", 57344, 8192),
    ("70b down", 8192, 28672),
]
MS = (16, 64, 256)
ROTATE_BYTES = 1536 << 20


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us


def main():
    assert torch.cuda.is_available() and ops.have_native()
    dev = "cuda:0"
    shapes = SHAPES
    if len(sys.argv) == 4:
        shapes = [("custom",) + tuple(int(a) for a in sys.argv[2:4])]
    ms = MS if len(sys.argv) != 4 else (int(sys.argv[1]),)
    print("shape, M, bf16 us, fp8 us, fp8/bf16 speedup, bf16 GB/s, fp8 GB/s, max err")
    for name, N, K in shapes:
        n16 = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        n8 = max(2, -(-ROTATE_BYTES // (N * K)))
        w16, tw, q8, s8 = [], [], [], []
        # the twin the bf16 model would build for this shape (None: library)
        has_twin = ops._m256_config(256, N, K) is not None
        for i in range(max(n16, n8)):
            w = (torch.randn(N, K, device=dev) * 0.02).bfloat16()
            if i < n8:
                q, s = ops.fp8_quantize_weight(w)
                q8.append(ops.swizzle_weight_frag_fp8(q))
                s8.append(s)
                if i == 0:
                    deq0 = ops.fp8_dequantize_weight(q, s, torch.float32)
                del q
            if i < n16:
                w16.append(w)
                tw.append(ops.swizzle_weight_frag(w) if has_twin else None)
            del w
        for M in ms:
            x = (torch.randn(M, K, device=dev) * 0.5).bfloat16()
            ref = x.float() @ deq0.T
            got = ops.linear_w8(x, q8[0], s8[0]).float()
            err = ((got - ref).abs().max() / (ref.abs().max() + 1e-3)).item()

            def f16(i):
                return ops.linear(x, w16[i % n16], tw[i % n16])

            def f8(i):
                return ops.linear_w8(x, q8[i % n8], s8[i % n8])

            for fn in (f16, f8):  # warm-up: code objects, library algorithm
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            t16, t8 = [], []
            for _ in range(3):
                t16.append(timed(f16, 2 * n16 + 20))
                t8.append(timed(f8, 2 * n8 + 20))
            a, b = statistics.median(t16), statistics.median(t8)
            by16 = N * K * 2 + M * (K + N) * 2
            by8 = N * K + N * 4 + M * (K + N) * 2
            print(
                f"{name} ({N}x{K}), {M}, {a:.1f}, {b:.1f}, {a / b:.2f}, "
                f"{by16 / a / 1e3:.0f}, {by8 / b / 1e3:.0f}, {err:.4f}",
                flush=True,
            )
        del w16, tw, q8, s8, deq0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
