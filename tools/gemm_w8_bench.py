"""Cold-cache timing of the fp8 (W8A16) decode GEMM routes against the bf16
route on the decode projection shapes of llama-3-8b and llama-3-70b.

Three routes: bf16 (ops.linear with the twin the bf16 model builds), fp8
streaming (csrc/gemm_w8.hip) and fp8 macro-tile (csrc/gemm_w8_m256.hip, with
the configuration ops._w8_m256_config lists for the shape, else the
defaults).

Each route cycles through enough weight copies (>= 1.5 GB) that no copy
is still in the 256 MB L3 when its turn comes again, as in the engine,
where a decode step streams the whole model between two uses of a
matrix. Routes alternate, three rounds each; the median round is
reported with the min-max of the three, with the bytes each route has to
stream and the rate that implies. Run on the GPU box:

    python tools/gemm_w8_bench.py [--ms=96,192] [M N K]
    python tools/gemm_w8_bench.py --sweep [--ms=96,192] [M N K]

--sweep times nf in {4,8} x nsk in {1,2,4,8} of the macro route beside the
other two routes, in the same alternation, on every shape (or the one
given); ops._w8_m256_config is filled from its output.
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
MS = (16, 64, 128, 256)
ROTATE_BYTES = 1536 << 20
SWEEP = [(nf, nsk) for nf in (4, 8) for nsk in (1, 2, 4, 8)]


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
    for fn in routes:  # warm-up: code objects, library algorithm
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
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sweep = "--sweep" in sys.argv
    shapes = SHAPES
    if len(args) == 3:
        shapes = [("custom",) + tuple(int(a) for a in args[1:3])]
    ms = MS if len(args) != 3 else (int(args[0]),)
    for a in sys.argv[1:]:
        if a.startswith("--ms="):  # batch sizes other than MS, all shapes
            ms = tuple(int(m) for m in a[5:].split(","))
    if sweep:
        print(
            "shape, M, bf16 us, fp8 stream us, "
            + ", ".join(f"nf{nf}/nsk{nsk} us" for nf, nsk in SWEEP)
            + ", max err"
        )
    else:
        print(
            "shape, M, bf16 us, fp8 stream us, fp8 macro us, macro cfg, "
            "macro/stream speedup, macro/bf16 speedup, bf16 GB/s, "
            "stream GB/s, macro GB/s, max err stream, max err macro"
        )
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

            def err_of(got):
                return ((got.float() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()

            def f16(i):
                return ops.linear(x, w16[i % n16], tw[i % n16])

            def f8(i):
                return ops.linear_w8(x, q8[i % n8], s8[i % n8])

            def macro(nf, nsk):
                return lambda i: ops.gemm_w8_m256(
                    x, q8[i % n8], s8[i % n8], nf=nf, nsk=nsk
                )

            it16, it8 = 2 * n16 + 20, 2 * n8 + 20
            by16 = N * K * 2 + M * (K + N) * 2
            by8 = N * K + N * 4 + M * (K + N) * 2
            if sweep:
                cfgs = [c for c in SWEEP if N % (16 * c[0]) == 0]
                err = max(err_of(macro(*c)(0)) for c in cfgs)
                ts = rounds(
                    [f16, f8] + [macro(*c) for c in cfgs],
                    [it16, it8] + [it8] * len(cfgs),
                )
                print(
                    f"{name} ({N}x{K}), {M}, "
                    + ", ".join(fmt(t) for t in ts)
                    + f", {err:.4f}",
                    flush=True,
                )
                continue
            cfg = ops._w8_m256_config(M, N, K)
            tag = "table" if cfg is not None else "default"
            if cfg is None:
                cfg = ops._w8_m256_default(M, N, K)
            fm = macro(cfg["nf"], cfg["nsk"])
            a, b, c = rounds([f16, f8, fm], [it16, it8, it8])
            print(
                f"{name} ({N}x{K}), {M}, {fmt(a)}, {fmt(b)}, {fmt(c)}, "
                f"nf{cfg['nf']}/nsk{cfg['nsk']} {tag}, {b[0] / c[0]:.2f}, "
                f"{a[0] / c[0]:.2f}, {by16 / a[0] / 1e3:.0f}, "
                f"{by8 / b[0] / 1e3:.0f}, {by8 / c[0] / 1e3:.0f}, "
                f"{err_of(f8(0)):.4f}, {err_of(fm(0)):.4f}",
                flush=True,
            )
        del w16, tw, q8, s8, deq0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
