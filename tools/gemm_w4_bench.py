"""Cold-cache timing of the MXFP4 (W4A16) decode GEMM routes against the fp8
(W8A16) routes and the bf16 route on the decode projection shapes of
llama-3-8b and llama-3-70b.

Five routes: bf16 (ops.linear with the twin the bf16 model builds), fp8
streaming (csrc/gemm_w8.hip), fp8 macro-tile (csrc/gemm_w8_m256.hip, at the
configuration ops._w8_m256_config lists, else the defaults), mxfp4 streaming
(csrc/gemm_w4.hip) and mxfp4 macro-tile (csrc/gemm_w4_m256.hip, at the
configuration ops._w4_m256_config lists, else the defaults).

Each route cycles through enough weight copies (>= 1.5 GB) that no copy is
still in the 256 MB L3 when its turn comes again, as in the engine, where a
decode step streams the whole model between two uses of a matrix. Copy 0 of
each quantised route is a real quantisation of copy 0 of the bf16 weights
(its error is printed); the other copies are random bytes of the same
layout (finite values only), which stream the same. Routes alternate, three
rounds each; the median round is reported with the min-max of the three,
with the bytes each route has to stream and the rate that implies. Run on
the GPU box:

    python tools/gemm_w4_bench.py [--ms=1,16,64] [M N K]
    python tools/gemm_w4_bench.py --sweep [--ms=96,192] [M N K]

--sweep times nf in {4,8} x nsk in {1,2,4,8} of the mxfp4 macro route beside
the other four routes, in the same alternation, at M in {16,64,128,256} on
every shape (or the one given); ops._W4_M256_TABLE is filled from its
output.
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
MS = (1, 16, 64)
SWEEP_MS = (16, 64, 128, 256)
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


def table_or_default(config, default, M, N, K):
    """(kwargs, tag) of a macro route: its table entry, else its defaults."""
    cfg = config(M, N, K)
    if cfg is not None:
        return cfg, "table"
    return default(M, N, K), "default"


def main():
    assert torch.cuda.is_available() and ops.have_native()
    dev = "cuda:0"
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sweep = "--sweep" in sys.argv
    shapes = SHAPES
    if len(args) == 3:
        shapes = [("custom",) + tuple(int(a) for a in args[1:3])]
    ms = (SWEEP_MS if sweep else MS) if len(args) != 3 else (int(args[0]),)
    for a in sys.argv[1:]:
        if a.startswith("--ms="):
            ms = tuple(int(m) for m in a[5:].split(","))
    if sweep:
        print(
            "shape, M, bf16 us, fp8 stream us, fp8 macro us, fp8 macro cfg, "
            "mxfp4 stream us, "
            + ", ".join(f"nf{nf}/nsk{nsk} us" for nf, nsk in SWEEP)
            + ", max err"
        )
    else:
        print(
            "shape, M, bf16 us, fp8 stream us, fp8 macro us, fp8 macro cfg, "
            "mxfp4 stream us, mxfp4 macro us, mxfp4 macro cfg, "
            "mxfp4 macro/stream speedup, mxfp4 macro/bf16 speedup, "
            "mxfp4 stream/fp8 stream speedup, bf16 GB/s, fp8 stream GB/s, "
            "mxfp4 stream GB/s, mxfp4 macro GB/s, max err fp8, "
            "max err mxfp4 stream, max err mxfp4 macro"
        )
    for name, N, K in shapes:
        n16 = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        n8 = max(2, -(-ROTATE_BYTES // (N * K)))
        n4 = max(2, -(-ROTATE_BYTES // (N * K * 17 // 32)))
        has_twin = ops._m256_config(256, N, K) is not None
        w0 = (torch.randn(N, K, device=dev) * 0.02).bfloat16()
        q, s = ops.fp8_quantize_weight(w0)
        deq8 = ops.fp8_dequantize_weight(q, s, torch.float32)
        q8, s8 = [ops.swizzle_weight_frag_fp8(q)], [s]
        p, sb = ops.mxfp4_quantize_weight(w0)
        deq4 = ops.mxfp4_dequantize_weight(p, sb, torch.float32)
        qf, sf = ops.swizzle_weight_frag_mxfp4(p, sb)
        q4, s4 = [qf], [sf]
        del q, p
        for _ in range(1, n8):  # low 7 bits below 0x7F: no NaN encodings
            q8.append(
                torch.randint(0, 0x7F, q8[0].shape, device=dev, dtype=torch.uint8)
                | (torch.randint(0, 2, q8[0].shape, device=dev, dtype=torch.uint8) << 7)
            )
            s8.append(s8[0])
        for _ in range(1, n4):
            q4.append(torch.randint(0, 256, q4[0].shape, device=dev, dtype=torch.uint8))
            s4.append(torch.randint(118, 123, s4[0].shape, device=dev, dtype=torch.uint8))
        w16 = [w0] + [
            (torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(1, n16)
        ]
        tw = [ops.swizzle_weight_frag(w) if has_twin else None for w in w16]
        for M in ms:
            x = (torch.randn(M, K, device=dev) * 0.5).bfloat16()

            def err_of(got, deq):
                ref = x.float() @ deq.T
                return ((got.float() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()

            def f16(i):
                return ops.linear(x, w16[i % n16], tw[i % n16])

            def f8(i):
                return ops.linear_w8(x, q8[i % n8], s8[i % n8])

            def f4(i):
                return ops.linear_w4(x, q4[i % n4], s4[i % n4])

            def m8(nf, nsk):
                return lambda i: ops.gemm_w8_m256(
                    x, q8[i % n8], s8[i % n8], nf=nf, nsk=nsk
                )

            def m4(nf, nsk):
                return lambda i: ops.gemm_w4_m256(
                    x, q4[i % n4], s4[i % n4], nf=nf, nsk=nsk
                )

            it16, it8, it4 = 2 * n16 + 20, 2 * n8 + 20, 2 * n4 + 20
            c8, tag8 = table_or_default(ops._w8_m256_config, ops._w8_m256_default, M, N, K)
            fm8 = m8(c8["nf"], c8["nsk"])
            if sweep:
                cfgs = [c for c in SWEEP if N % (16 * c[0]) == 0]
                err = max(err_of(m4(*c)(0), deq4) for c in cfgs)
                ts = rounds(
                    [f16, f8, fm8, f4] + [m4(*c) for c in cfgs],
                    [it16, it8, it8, it4] + [it4] * len(cfgs),
                )
                cells = [fmt(t) for t in ts]
                cells.insert(3, f"nf{c8['nf']}/nsk{c8['nsk']} {tag8}")
                print(
                    f"{name} ({N}x{K}), {M}, " + ", ".join(cells) + f", {err:.4f}",
                    flush=True,
                )
                continue
            c4, tag4 = table_or_default(ops._w4_m256_config, ops._w4_m256_default, M, N, K)
            fm4 = m4(c4["nf"], c4["nsk"])
            a, b, bm, c, cm = rounds(
                [f16, f8, fm8, f4, fm4], [it16, it8, it8, it4, it4]
            )
            act = M * (K + N) * 2
            by16 = N * K * 2 + act
            by8 = N * K + N * 4 + act
            by4 = N * K * 17 // 32 + act
            print(
                f"{name} ({N}x{K}), {M}, {fmt(a)}, {fmt(b)}, {fmt(bm)}, "
                f"nf{c8['nf']}/nsk{c8['nsk']} {tag8}, {fmt(c)}, {fmt(cm)}, "
                f"nf{c4['nf']}/nsk{c4['nsk']} {tag4}, {c[0] / cm[0]:.2f}, "
                f"{a[0] / cm[0]:.2f}, {b[0] / c[0]:.2f}, {by16 / a[0] / 1e3:.0f}, "
                f"{by8 / b[0] / 1e3:.0f}, {by4 / c[0] / 1e3:.0f}, "
                f"{by4 / cm[0] / 1e3:.0f}, {err_of(f8(0), deq8):.4f}, "
                f"{err_of(f4(0), deq4):.4f}, {err_of(fm4(0), deq4):.4f}",
                flush=True,
            )
        del w16, tw, q8, s8, q4, s4, deq8, deq4, w0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

