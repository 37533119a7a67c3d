"""Cold-cache timing of the mixture-of-experts MLP (ops.moe_mlp,
csrc/moe.hip) on Mixtral-8x7B's shapes (H 4096, I 14336, 8 experts, top-2)
with uniform-random routing, beside two baselines at the same T:

  (a) the dense llama-3-8b MLP on the existing route (ops.swiglu_linear +
      ops.linear_rmsnorm_residual): one expert's worth of weights, the floor
      a k-of-E layer cannot reach;
  (b) a per-expert loop of library GEMMs on rows PRE-SORTED by expert
      (the sort and the gather are done once, outside the timed call). Timed
      are the read-back of the per-expert row counts, the two library GEMMs
      and the swiglu per expert, and one weighted combine + norm. THE HOST
      SYNCS once per call on the counts, so the route cannot be captured
      into a decode graph.

The last column times moe_align alone (warm, the sort of the T*k pairs).

Where moe_mlp takes the 128-row prefill tile (csrc/moe_prefill.hip; the mf
column shows the tile actually used), the same call is also timed with
LLMAPI_MOE_BIG_MIN_ROWS set high, which forces the 64-row kernels, in the same
alternating rounds.

--weight-dtype=auto,mxfp4 also times moe_mlp on the MXFP4 quantisation of the
same expert weights (csrc/moe_w4.hip) in the same alternating rounds and
prints a second line per T. From 128 pairs per expert it is timed twice: with
LLMAPI_MOE_W4_BIG_MIN_ROWS=128 on the 128-row MXFP4 tile
(csrc/moe_w4_prefill.hip) and with the knob set high on the 64-row kernels
("mxfp4 64-row / new").

--weight-dtype=auto,fp8 (or auto,mxfp4,fp8) likewise times moe_mlp on the fp8
quantisation of the same expert weights (csrc/moe_w8.hip; moe_pick_mf's tile
at every T, there is no 128-row fp8 tile) and prints a line per T.

As in tools/lora_bench.py every route cycles through several layers' worth of
weights (each layer's experts are 2.8 GB, far beyond the 256 MB L3), routes
alternate, three rounds each; the median round is reported with the min-max
of the three. Run on the GPU box:

    python tools/moe_bench.py [--ts=16,64,256,512,1024,2048,4096] [--weight-dtype=auto,mxfp4,fp8]
"""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmapigateway_amd import ops

H, INTER, E, K = 4096, 14336, 8, 2
TS = (16, 64, 256, 512, 1024, 2048, 4096)
MOE_LAYERS = 2    # 5.6 GB of expert weights per form
DENSE_LAYERS = 5  # 1.7 GB of dense MLP weights


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
        for t, fn in zip(ts, routes):
            t.append(timed(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})"


def main():
    assert torch.cuda.is_available() and ops.have_native()
    dev = "cuda:0"
    ts, dtypes = TS, ("auto",)
    for a in sys.argv[1:]:
        if a.startswith("--ts="):
            ts = tuple(int(v) for v in a[5:].split(","))
        elif a.startswith("--weight-dtype="):
            dtypes = tuple(a[15:].split(","))
        else:
            raise SystemExit(f"unknown argument {a}")
    assert set(dtypes) <= {"auto", "mxfp4", "fp8"} and "auto" in dtypes, dtypes

    def rand(*shape):
        return (torch.randn(*shape, device=dev) * 0.02).bfloat16()

    router = rand(E, H)
    norm_w = torch.ones(H, dtype=torch.bfloat16, device=dev)
    gu_plain = [torch.stack([rand(2 * INTER, H) for _ in range(E)]) for _ in range(MOE_LAYERS)]
    dn_plain = [torch.stack([rand(H, INTER) for _ in range(E)]) for _ in range(MOE_LAYERS)]
    gu_pack = [ops.moe_pack_weights(w, True) for w in gu_plain]
    dn_pack = [ops.moe_pack_weights(w, False) for w in dn_plain]

    def pack_w4(w, gate_up):  # expert by expert: the quantiser works in fp32
        qs = [ops.mxfp4_quantize_weight(w[e]) for e in range(E)]
        return ops.moe_pack_weights_mxfp4(
            torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs]), gate_up
        )

    def pack_w8(w, gate_up):
        qs = [ops.fp8_quantize_weight(w[e]) for e in range(E)]
        return ops.moe_pack_weights_fp8(
            torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs]), gate_up
        )

    w8 = "fp8" in dtypes
    gu_w8 = [pack_w8(w, True) for w in gu_plain] if w8 else []
    dn_w8 = [pack_w8(w, False) for w in dn_plain] if w8 else []
    w4 = "mxfp4" in dtypes
    gu_w4 = [pack_w4(w, True) for w in gu_plain] if w4 else []
    dn_w4 = [pack_w4(w, False) for w in dn_plain] if w4 else []
    d_gu = [rand(2 * INTER, H) for _ in range(DENSE_LAYERS)]
    d_dn = [rand(H, INTER) for _ in range(DENSE_LAYERS)]
    d_int = [
        ops.swizzle_weight_frag(ops.interleave_gate_up(w))
        if ops._m256_swiglu_config(256, 2 * INTER, H) is not None else None
        for w in d_gu
    ]
    d_dn_swz = [
        ops.swizzle_weight_frag(w)
        if ops._m256_config(256, H, INTER) is not None else None
        for w in d_dn
    ]
    torch.cuda.empty_cache()

    print("T, mf, moe_mlp us, moe_mlp on the 64-row kernels us, (a) dense 8b MLP us, "
          "(b) host-synced expert loop us, moe/(a), moe/(b), expert weight bytes / "
          "moe_mlp time GB/s, moe_align alone us")
    for T in ts:
        x = (torch.randn(T, H, device=dev) * 0.5).bfloat16()
        res = torch.zeros(T, H, dtype=torch.bfloat16, device=dev)
        # uniform-random routing: k distinct experts per token
        ids = torch.rand(T, E, device=dev).argsort(dim=1)[:, :K].int().contiguous()
        wts = torch.full((T, K), 1.0 / K, device=dev)

        def moe(i):
            j = i % MOE_LAYERS
            return ops.moe_mlp(x, router, gu_pack[j], dn_pack[j], K, res, norm_w,
                               1e-5, ids=ids, weights=wts)

        def moe_old(i):
            os.environ["LLMAPI_MOE_BIG_MIN_ROWS"] = str(10**9)
            try:
                return moe(i)
            finally:
                del os.environ["LLMAPI_MOE_BIG_MIN_ROWS"]

        def moe_w4(i):
            j = i % MOE_LAYERS
            return ops.moe_mlp(x, router, gu_w4[j][0], dn_w4[j][0], K, res, norm_w,
                               1e-5, ids=ids, weights=wts,
                               s_gate_up=gu_w4[j][1], s_down=dn_w4[j][1])

        def moe_w8(i):
            j = i % MOE_LAYERS
            return ops.moe_mlp(x, router, gu_w8[j][0], dn_w8[j][0], K, res, norm_w,
                               1e-5, ids=ids, weights=wts,
                               s_gate_up=gu_w8[j][1], s_down=dn_w8[j][1])

        def w4_knob(min_rows):
            def run(i):
                os.environ["LLMAPI_MOE_W4_BIG_MIN_ROWS"] = str(min_rows)
                try:
                    return moe_w4(i)
                finally:
                    del os.environ["LLMAPI_MOE_W4_BIG_MIN_ROWS"]
            return run

        def dense(i):
            j = i % DENSE_LAYERS
            act = ops.swiglu_linear(x, d_gu[j], None, d_int[j])
            return ops.linear_rmsnorm_residual(act, d_dn[j], d_dn_swz[j], res, norm_w, 1e-5)

        # (b): rows pre-sorted by expert, outside the timed call
        flat = ids.view(-1).long()
        order = flat.argsort(stable=True)
        xs = x[order // K].contiguous()
        counts_dev = torch.bincount(flat, minlength=E)
        # y rows come out in sorted order; the combine reads them back in
        # pair order through the inverse permutation
        inv = order.argsort()
        y = torch.empty(T * K, H, dtype=torch.bfloat16, device=dev)

        def loop(i):
            j = i % MOE_LAYERS
            counts = counts_dev.tolist()  # the host sync
            lo = 0
            for e, n in enumerate(counts):
                if n:
                    act = ops.swiglu(ops.linear(xs[lo : lo + n], gu_plain[j][e]))
                    y[lo : lo + n] = ops.linear(act, dn_plain[j][e])
                lo += n
            s = (y[inv].view(T, K, H).float() * wts.unsqueeze(-1)).sum(1).bfloat16()
            return ops.rmsnorm_residual(s, res, norm_w, 1e-5)

        def align(i):
            return ops.moe_align(ids, E)

        # windows of 0.1-0.3 s per round
        iters = 300 if T <= 256 else 100 if T <= 1024 else 40
        big = ops._moe_big_route(T, K, E, H, INTER, False)
        big4 = w4 and ops.moe_big_serves(H, INTER) and T * K >= 128 * E
        m, a, b, *q = rounds(
            [moe, dense, loop] + ([moe_old] if big else [])
            + ([w4_knob(128 if big4 else 10**9)] if w4 else [])
            + ([w4_knob(10**9)] if big4 else [])
            + ([moe_w8] if w8 else []),
            iters,
        )
        old = fmt(q.pop(0)) if big else "-"
        t8 = q.pop() if w8 else None
        (al,) = rounds([align], 300)
        used = len(torch.unique(ids)) * 3 * H * INTER * 2  # bytes of experts hit
        mf = 8 if big else ops._native().moe_pick_mf(T, K, E)
        print(
            f"{T}, {mf}, {fmt(m)}, {old}, {fmt(a)}, {fmt(b)}, {m[0] / a[0]:.2f}, "
            f"{m[0] / b[0]:.2f}, {used / m[0] / 1e3:.0f}, {fmt(al)}",
            flush=True,
        )
        if q:
            t = q[0]
            # disjoint: the two min-max ranges do not overlap
            line = (
                f"  mxfp4 (mf {8 if big4 else mf}): moe_mlp {fmt(t)} us, bf16/mxfp4 "
                f"{m[0] / t[0]:.2f}, disjoint {t[2] < m[1] or m[2] < t[1]}, expert "
                f"weight bytes / time {used * 4.25 / 16 / t[0] / 1e3:.0f} GB/s"
            )
            if big4:
                o = q[1]
                line += (
                    f", on the 64-row kernels {fmt(o)} us, mxfp4 64-row / new "
                    f"{o[0] / t[0]:.2f}, new wholly below {t[2] < o[1]}, "
                    f"mxfp4 new / (b) {t[0] / b[0]:.2f}"
                )
            print(line, flush=True)
        if t8:
            line = (
                f"  fp8 (mf {ops._native().moe_pick_mf(T, K, E)}): moe_mlp {fmt(t8)} us, "
                f"bf16/fp8 {m[0] / t8[0]:.2f}, disjoint {t8[2] < m[1] or m[2] < t8[1]}, "
                f"expert weight bytes / time {used / 2 / t8[0] / 1e3:.0f} GB/s"
            )
            if q:
                line += f", mxfp4/fp8 {q[0][0] / t8[0]:.2f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
