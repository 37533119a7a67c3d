"""Op dispatch: gfx950 HIP kernels on GPU, PyTorch reference on CPU.

The HIP extension (llmapigateway_amd/ops/_C*.so, built in-tree by
``python setup.py build_ext --inplace`` / __graft_entry__.build) is the ONLY
compute path on GPU tensors — if a CUDA tensor reaches an op and the
extension is missing, we raise instead of silently falling back to eager
PyTorch. CPU tensors use ops.reference (fp32 semantics contract).
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

# Enable the pre-tuned hipBLASLt/rocBLAS GEMM selections for gfx950 (3.2x on
# the decode lm_head GEMM). torch appends the device ordinal before ".csv",
# so the shipped table is tunableop_gfx950<N>.csv and FILENAME names the
# base. Must be set before the first GEMM executes; honor user overrides.
_TUNE_BASE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")
if os.path.exists(_TUNE_BASE.replace(".csv", "0.csv")):
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", _TUNE_BASE)

import torch

# Belt-and-braces: activate TunableOp through the python API too (the env
# vars alone were not picked up when torch was imported first elsewhere).
if torch.version.hip and os.path.exists(_TUNE_BASE.replace(".csv", "0.csv")):
    try:
        import torch.cuda.tunable as _tunable

        _tunable.enable(True)
        # honor an explicit tuning request (tools/tune_gemms.py sets "1");
        # otherwise lock to lookup-only so serving never pays tuning cost
        if os.environ.get("PYTORCH_TUNABLEOP_TUNING") != "1":
            _tunable.tuning_enable(False)
            _tunable.set_filename(_TUNE_BASE, insert_device_ordinal=True)
            _tunable.read_file(_TUNE_BASE.replace(".csv", "0.csv"))
    except Exception:  # pragma: no cover - best effort
        pass

from . import reference
from .reference import build_rope_cache  # re-export (host-side table builder)
from .reference import (  # re-export (fp8 weight quantisation scheme)
    fp8_dequantize_weight,
    fp8_quantize_weight,
    swizzle_weight_frag_fp8,
    unswizzle_weight_frag_fp8,
)
from .reference import (  # re-export (MXFP4 weight quantisation scheme)
    mxfp4_dequantize_weight,
    mxfp4_quantize_weight,
    swizzle_weight_frag_mxfp4,
    unswizzle_weight_frag_mxfp4,
)

_C = None
_C_ERR: Optional[str] = None
try:
    import importlib

    _C = importlib.import_module("._C", __name__)
except ImportError as e:  # extension not built (CPU-only envs are fine)
    _C_ERR = str(e)


def have_native() -> bool:
    return _C is not None


def _native():
    if _C is None:
        raise RuntimeError(
            "llmapigateway_amd.ops._C (gfx950 HIP extension) is not built but a GPU tensor "
            "reached the ops layer. Build it with `python setup.py build_ext --inplace` "
            f"(import error: {_C_ERR})"
        )
    return _C


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().rmsnorm(out, x, weight, eps)
        return out
    return reference.rmsnorm(x, weight, eps)


def rmsnorm_residual(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> Tuple[torch.Tensor, torch.Tensor]:
    if x.is_cuda:
        # fused: residual += x; x_out = rmsnorm(residual) — one HBM pass
        out = torch.empty_like(x)
        _native().rmsnorm_residual(out, x, residual, weight, eps)
        return out, residual
    return reference.rmsnorm_residual(x, residual, weight, eps)


def rope_inplace(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor
) -> None:
    if q.is_cuda:
        _native().rope_inplace(q, k, positions, cos_sin)
        return
    reference.rope_inplace(q, k, positions, cos_sin)


def swiglu(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        inter = x.shape[-1] // 2
        out = torch.empty(
            (*x.shape[:-1], inter), dtype=x.dtype, device=x.device
        )
        _native().swiglu(out, x)
        return out
    return reference.swiglu(x)


def rope_and_kv_write(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    positions: torch.Tensor,
    cos_sin: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> None:
    """Fused rope_inplace(q, k) + kv_cache_write(k, v): one launch on GPU.
    With k_scale/v_scale the cache is fp8 e4m3 (per-row quantization)."""
    if q.is_cuda:
        _native().rope_kv_write(
            q, k, v, k_cache, v_cache, positions, cos_sin, slot_mapping,
            k_scale, v_scale,
        )
        return
    reference.rope_inplace(q, k, positions, cos_sin)
    reference.kv_cache_write(k, v, k_cache, v_cache, slot_mapping, k_scale, v_scale)


def kv_cache_write(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> None:
    if k.is_cuda:
        _native().kv_cache_write(k, v, k_cache, v_cache, slot_mapping, k_scale, v_scale)
        return
    reference.kv_cache_write(k, v, k_cache, v_cache, slot_mapping, k_scale, v_scale)


QTILE = 64  # q rows per prefill workgroup (must match attention_prefill.hip)


def build_prefill_tiles(seqlens, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-side tile map for the prefill kernel: one entry per 64-row q tile."""
    tile_seq, tile_off = [], []
    for i, L in enumerate(seqlens):
        for off in range(0, int(L), QTILE):
            tile_seq.append(i)
            tile_off.append(off)
    return (
        torch.tensor(tile_seq, dtype=torch.int32, device=device),
        torch.tensor(tile_off, dtype=torch.int32, device=device),
    )


def attention_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    scale: Optional[float] = None,
    causal: bool = True,
    tile_seq: Optional[torch.Tensor] = None,
    tile_off: Optional[torch.Tensor] = None,
    k_cache: Optional[torch.Tensor] = None,
    v_cache: Optional[torch.Tensor] = None,
    block_tables: Optional[torch.Tensor] = None,
    cached_lens: Optional[torch.Tensor] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = 0,
) -> torch.Tensor:
    """Varlen causal prefill. With cached_lens set, each sequence also
    attends (unmasked) to its first cached_lens[i] positions read from the
    paged KV cache via block_tables — the prefix-caching / chunked-prefill
    context phase. window = W > 0 is sliding-window attention: the row at
    absolute position p = cached_lens[i] + r attends to keys p - W < j <= p,
    and cache blocks wholly below a sequence's first window are not read;
    0 or None is no window."""
    if scale is None:
        scale = float(q.shape[-1]) ** -0.5
    window = _check_window(window)
    if q.is_cuda:
        if not causal:
            raise NotImplementedError("GPU prefill kernel is causal-only")
        if tile_seq is None or tile_off is None:
            cu = cu_seqlens.cpu().tolist()
            seqlens = [cu[i + 1] - cu[i] for i in range(len(cu) - 1)]
            tile_seq, tile_off = build_prefill_tiles(seqlens, q.device)
        out = torch.empty_like(q)
        _native().attention_prefill(
            out, q, k, v, cu_seqlens.int(), tile_seq, tile_off, float(scale),
            k_cache, v_cache, block_tables, cached_lens, k_scale, v_scale,
            window,
        )
        return out
    return reference.attention_prefill(
        q, k, v, cu_seqlens, scale, causal,
        k_cache=k_cache, v_cache=v_cache,
        block_tables=block_tables, cached_lens=cached_lens,
        k_scale=k_scale, v_scale=v_scale, window=window,
    )


def _check_window(window: Optional[int]) -> int:
    window = int(window or 0)
    if window < 0:
        raise ValueError(f"window must be >= 0, got {window}")
    return window


_SPLIT_SPAN = 2048  # keep in sync with SPLIT_SPAN in attention_decode.hip
# decode-attention geometry: 2 = shared-LDS-chunk / wave-per-head form
# (coalesced staging, no cross-wave combine); 1 = the round-1 form
_DECODE_VER = int(os.environ.get("LLMAPI_DECODE_VER", "2"))


class _Scratch:
    """Grow-only per-device scratch buffer. Kernels fully overwrite what
    they use, so nothing is zeroed and the address is stable across
    hipGraph replays; a buffer is never shrunk, and when one has to grow
    the old one is retired, not freed: a captured graph may still replay
    into it."""

    def __init__(self, dtype: torch.dtype):
        self.dtype = dtype
        self.bufs: dict = {}
        self.retired: list = []

    def get(self, device, numel: int) -> torch.Tensor:
        device = torch.device(device)
        buf = self.bufs.get(device.index)
        if buf is None or buf.numel() < numel:
            if buf is not None:
                self.retired.append(buf)
            buf = torch.empty(numel, dtype=self.dtype, device=device)
            self.bufs[device.index] = buf
        return buf


_decode_acc = _Scratch(torch.float32)  # flash-decode partial accumulators
_decode_ml = _Scratch(torch.float32)   # ... and their (max, sum) pairs
_slabs = _Scratch(torch.float32)       # split-K fp32 slabs of the decode GEMMs
_w8_dq = _Scratch(torch.bfloat16)      # bf16 image of an fp8 / MXFP4 weight (M > 256)


def attention_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: Optional[float] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = 0,
) -> torch.Tensor:
    """Paged single-token decode. window = W > 0 is sliding-window
    attention over the keys [max(0, L - W), L) of each sequence: blocks
    wholly below them are not read (nor their block-table entries), so the
    caller may have released them; 0 or None is no window."""
    if scale is None:
        scale = float(q.shape[-1]) ** -0.5
    window = _check_window(window)
    if q.is_cuda:
        out = torch.empty_like(q)
        # flash-decode context splits when (B x Hkv) underfills the 256 CUs
        # but the block table allows long contexts; derived only from
        # capture-stable shapes so hipGraph replays stay valid. Each split
        # takes _SPLIT_SPAN keys; past 8 * _SPLIT_SPAN positions the count
        # stays 8 and the launcher widens the span to cover the block table
        B, Hq = q.shape[0], q.shape[1]
        max_ctx = block_tables.shape[1] * k_cache.shape[2]
        if window:
            # the kernel measures the splits from the 64-aligned window
            # start: at most window + 63 keys, whatever the context (a
            # constant of the call, never context_lens: capture-stable)
            max_ctx = min(max_ctx, window + 64)
        nsplit = 1
        if B * k_cache.shape[1] < 192 and max_ctx > _SPLIT_SPAN:
            nsplit = min(8, -(-max_ctx // _SPLIT_SPAN))
        if nsplit > 1:
            pa = _decode_acc.get(q.device, B * Hq * nsplit * q.shape[2])
            pm = _decode_ml.get(q.device, B * Hq * nsplit * 2)
            # measured: the v1 geometry wins once the flash-decode split
            # path engages (small-batch long-context), v2 everywhere else
            _native().attention_decode(
                out, q, k_cache, v_cache, block_tables, context_lens,
                float(scale), pa, pm, nsplit, k_scale, v_scale, 1, window,
            )
        else:
            _native().attention_decode(
                out, q, k_cache, v_cache, block_tables, context_lens,
                float(scale), None, None, 1, k_scale, v_scale, _DECODE_VER,
                window,
            )
        return out
    return reference.attention_decode(
        q, k_cache, v_cache, block_tables, context_lens, scale,
        k_scale=k_scale, v_scale=v_scale, window=window,
    )


# The 8-wave MF=2 depth-4 pipeline ties the tuned library when W is
# L3-resident (tools/gemm_probe.py rotates too little data for >100 MB
# weights, so its M>=64 rows are L3-warm and misled an M<=256 dispatch:
# in-engine, where the 16 GB weight cycle is always L3-cold, batch-256
# decode dropped 272 -> 129 req/s). In the true cold regime the library
# keeps winning at M >= 64; the custom kernel stays dispatched for the
# latency regime only.
_SKINNY_MAX_M = int(os.environ.get("SKINNY_GEMM_MAX_M", "16"))
_SKINNY_MAX_N = 28672


def _stream_nsk(N: int, K: int, kstep: int) -> int:
    """Split-K factor of the streaming kernels (csrc/gemm_stream.h), whose
    pipeline steps are kstep deep: target exactly 256 workgroups (one
    8-wave WG fills a CU; extra WGs only queue) — more splits just multiply
    the fp32 slab traffic, which at the old 512-WG target added ~60% to the
    weight stream and halved in-engine decode throughput. A slice keeps at
    least 8 steps."""
    tiles = N // 64
    nsk = max(1, -(-256 // tiles))
    return min(nsk, max(1, (K // kstep) // 8), 8)


def _skinny_nsk(N: int, K: int) -> int:
    return _stream_nsk(N, K, 32)


def _w8_nsk(N: int, K: int) -> int:
    return _stream_nsk(N, K, 64)


def _w4_nsk(N: int, K: int) -> int:
    return _stream_nsk(N, K, 64)


def _gemm_skinny(x: torch.Tensor, w: torch.Tensor, swizzled: bool) -> torch.Tensor:
    """The bf16 streaming kernel on w [N, K], or on its k-major twin."""
    M, K = x.shape
    N = w.shape[1] if swizzled else w.shape[0]
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    nsk = _skinny_nsk(N, K)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_skinny(y, x, w, ws, nsk, swizzled)
    return y


def _splitk_norm(launch, x: torch.Tensor, N: int, nsk: int, residual, norm_w, eps):
    """Run a split-K GEMM whose slab reduction also adds the residual and
    RMS-normalizes. launch(y, ws, *tail) is the binding call; y is not
    written on this path, so `out` stands in for its shape check."""
    M = x.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N)
    launch(out, ws, residual, norm_w, float(eps), out)
    return out, residual


def swizzle_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> k-major [K/32, N, 32] for gemm_skinny's contiguous
    B-tile streams (one 4 KB block per 64-row n-stripe per k-step)."""
    N, K = w.shape
    assert K % 32 == 0 and N % 64 == 0
    return w.view(N, K // 32, 32).permute(1, 0, 2).contiguous()


def swizzle_weight_frag(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> fragment-major [K/32, N/16, 64, 8] for gemm_m256.

    Element [k32][n16][lane][e] = W[n16*16 + (lane&15)][k32*32 + (lane>>4)*8
    + e]: each 1 KiB row is exactly one wave's mfma_f32_16x16x32_bf16
    B-fragment in lane order, so the kernel's global_load_lds staging is a
    straight contiguous copy and its ds_read_b128 is lane-linear
    (conflict-free per the gfx950 b128 lane groups)."""
    N, K = w.shape
    assert K % 64 == 0 and N % 64 == 0
    return (
        w.view(N // 16, 16, K // 32, 4, 8)
        .permute(2, 0, 3, 1, 4)
        .reshape(K // 32, N // 16, 64, 8)
        .contiguous()
    )


def _m256_config(M: int, N: int, K: int) -> Optional[dict]:
    """Measured dispatch table for the decode projections (cold-L3 sweep,
    profiles/r02_gemm_m256_sweep.md). Returns gemm_m256 kwargs, or None
    when the tuned library wins the shape (gate_up N=28672, lm_head)."""
    if M > 256:
        return None
    if N == 8192 and K % 64 == 0 and K >= 8192:
        # 70B-class projections at tp=1 (hidden 8192): o-proj K=8192
        # (51.2 vs library 58.2 us) and down-proj K=28672 (147.5 vs
        # 192.4 us) — register-staged variant wins the deep-K shape
        if K > 8192:
            return {"nf": 8, "nsk": 4, "variant": 1, "pipe": 0}  # 70B down 1.30x
        return {"nf": 8, "nsk": 4, "variant": 0, "pipe": 0}      # 70B o 1.14x
    if N == 7168 and K <= 8192:
        # tp=4 gate_up shard (unfused path): 37.3 vs library 43.4 us
        return {"nf": 4, "nsk": 3, "variant": 0, "pipe": 4}
    if N > 4096:
        # library wins the very wide shapes: gate_up N=28672/57344
        # (custom best 73.3 vs 70.3 us / 287.9 vs 258.0), qkv N=6144
        # (36.4 vs ~28 us — hipBLASLt's MT112x256 kernel is strong
        # exactly there) and N=10240 (77.7 vs 66.7), lm_head
        return None
    if K > 8192 and N % 128 == 0:
        return {"nf": 8, "nsk": 8, "variant": 0, "pipe": 0}  # down 1.34x
    if N < 2048:
        # narrow column shards (tp=4 qkv N=1536): too few tiles to fill
        # the chip — library 1.8x faster (21.7 vs 39.7 us)
        return None
    if K < 2048:
        # shallow-K row shards (tp=4 o-proj K=1024): single-pass
        # register-staged wins 1.67x (12.7 vs 21.2 us); split-K slab
        # traffic would dominate this little work
        return {"nf": 4, "nsk": 1, "variant": 1, "pipe": 0}
    # o-proj class (N<=4096, K<=8192): BK64/NBUF2 2-blocks/CU + split-K
    tiles = N // 64
    nsk = max(1, min(-(-256 // tiles), (K // 64) // 2, 8))
    return {"nf": 4, "nsk": nsk, "variant": 0, "pipe": 4}  # o 1.30x


def _m256_nsk(N: int, K: int, nf: int) -> int:
    """Split-K factor for gemm_m256: fill the 256 CUs (one 8-wave block
    per CU at the 120 KB LDS ring) when the column-tile count alone
    cannot. The fp32 slab traffic (2*nsk*M*N*4 B) is the price, so tiles
    >= 256 never split; smaller-N shapes are load-path/latency-bound and
    the slab round trip is cheap relative to the CU-fill win
    (profiles/r02_gemm_m256_probe.md)."""
    tiles = N // (16 * nf)
    if tiles >= 256:
        return 1
    nsk = -(-256 // tiles)
    return max(1, min(nsk, (K // 64) // 2, 8))


# swizzled weights raise the profitable dispatch ceiling (contiguous
# streams); plain-layout dispatch stays in the latency regime
_SKINNY_SWZ_MAX_M = int(os.environ.get("SKINNY_GEMM_SWZ_MAX_M", "256"))


# 0 = glds-staged, 1 = register-staged T14 (see gemm_m256.hip header)
_M256_VARIANT = int(os.environ.get("LLMAPI_M256_VARIANT", "0"))


def gemm_m256(
    x: torch.Tensor, w_frag: torch.Tensor, nf: Optional[int] = None,
    nsk: Optional[int] = None, variant: Optional[int] = None,
    pipe: Optional[int] = None,
) -> torch.Tensor:
    """y = x @ w.T with w pre-swizzled fragment-major (swizzle_weight_frag).
    The macro-tile LDS-staged decode GEMM (csrc/gemm_m256.hip); M <= 256.
    pipe selects the DMA ring geometry for the glds variant:
    0=(BK64,N3) 1=(BK64,N4,nf4) 2=(BK32,N4,nf8) 3=(BK32,N6,nf8)."""
    M, K = x.shape
    N = w_frag.shape[1] * 16
    if nf is None:
        if N % 128 == 0 and M > 64:
            nf = 8  # deep BK32 ring needs BN=128
        else:
            nf = 8 if N // 64 >= 448 else 4
    if N % (16 * nf) != 0:
        nf = 4
    if nsk is None:
        nsk = _m256_nsk(N, K, nf)
    if variant is None:
        variant = _M256_VARIANT
    if pipe is None:
        pipe = 3 if (variant == 0 and nf == 8 and K % 32 == 0) else 0
    if variant == 0:
        if pipe in (2, 3) and nf != 8:
            pipe = 0
        if pipe in (1, 4, 5) and nf != 4:
            pipe = 0
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_m256(y, x, w_frag, ws, nsk, nf, variant, pipe, 0)
    return y


def _reduce_norm_covers(N: int) -> bool:
    """Row widths the fused split-K reduce + RMSNorm kernel covers (keep in
    sync with gemm_reduce_rmsnorm_covers in csrc/gemm_skinny.hip)."""
    return N % 512 == 0 and 0 < N <= 8192


def gemm_m256_rmsnorm_residual(
    x: torch.Tensor, w_frag: torch.Tensor, residual: torch.Tensor,
    norm_w: torch.Tensor, eps: float, nf: int, nsk: int, variant: int = 0,
    pipe: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rmsnorm_residual(x @ w.T, residual, norm_w) with the residual add and
    the norm fused into the split-K slab reduction of gemm_m256 (one kernel
    instead of reduce + norm; the bf16 y never touches HBM). residual is
    updated in place, bit-identical to the unfused pair. Needs nsk > 1."""
    if nsk < 2:
        raise ValueError("fused reduce+norm needs split-K slabs (nsk > 1)")
    return _splitk_norm(
        lambda y, ws, *tail: _native().gemm_m256(
            y, x, w_frag, ws, nsk, nf, variant, pipe, 0, *tail
        ),
        x, w_frag.shape[1] * 16, nsk, residual, norm_w, eps,
    )


def _linear_route(
    M: int, N: int, K: int, twin: Optional[str], eligible: bool = True
) -> Tuple[str, dict]:
    """Where linear() sends a call: (route, kwargs) with route one of
    "m256" (gemm_m256 kwargs), "skinny" ({"swizzled": bool}) or "library".
    twin is the layout of the pre-swizzled weight copy: "frag"
    (fragment-major), "kmajor" (legacy) or None. eligible says the tensors
    suit the custom kernels at all: x a contiguous 2-D bf16 GPU tensor, w
    contiguous bf16."""
    if not (
        eligible
        and M > 0
        and N % 64 == 0
        and N <= _SKINNY_MAX_N
        and K % 32 == 0
    ):
        return "library", {}
    if twin == "frag" and 8 < M <= 256 and K % 64 == 0:
        # the measured table decides; a shape it leaves out is the
        # library's, even where M <= 16 would fit the skinny kernel
        cfg = _m256_config(M, N, K)
        return ("m256", cfg) if cfg is not None else ("library", {})
    if twin == "kmajor" and M <= _SKINNY_SWZ_MAX_M:
        return "skinny", {"swizzled": True}
    if M <= _SKINNY_MAX_M:
        return "skinny", {"swizzled": False}
    return "library", {}


def _route_of(
    x: torch.Tensor, w: torch.Tensor, w_swz: Optional[torch.Tensor]
) -> Tuple[str, dict]:
    twin = None if w_swz is None else {4: "frag", 3: "kmajor"}.get(w_swz.dim())
    eligible = (
        x.is_cuda
        and x.dim() == 2
        and x.dtype == torch.bfloat16
        and w.dtype == torch.bfloat16
        and x.is_contiguous()
        and w.is_contiguous()
    )
    return _linear_route(x.shape[0], w.shape[0], w.shape[1], twin, eligible)


def linear_rmsnorm_residual(
    x: torch.Tensor, w: torch.Tensor, w_swz: Optional[torch.Tensor],
    residual: torch.Tensor, norm_w: torch.Tensor, eps: float = 1e-5,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normed, residual) = rmsnorm_residual(linear(x, w, w_swz), residual,
    norm_w, eps). Fused into the split-K reduction exactly when linear()
    would pick gemm_m256 with nsk > 1 and the row width is covered; every
    other case (CPU, library shapes, M <= 8, M > 256, the legacy k-major
    twin, LLMAPI_NO_DECODE_FUSION=1) runs the two ops as before."""
    if not x.is_cuda:
        return reference.linear_rmsnorm_residual(x, w, residual, norm_w, eps)
    if not os.environ.get("LLMAPI_NO_DECODE_FUSION"):
        route, cfg = _route_of(x, w, w_swz)
        if (
            route == "m256"
            and cfg["nsk"] > 1
            and _reduce_norm_covers(w.shape[0])
            and residual.is_contiguous()
        ):
            return gemm_m256_rmsnorm_residual(
                x, w_swz, residual, norm_w, eps, **cfg
            )
    return rmsnorm_residual(linear(x, w, w_swz), residual, norm_w, eps)


def interleave_gate_up(w: torch.Tensor) -> torch.Tensor:
    """Row-permute a [gate; up] stacked weight [2I, K] into block-16
    interleaved order [g0..15, u0..15, g16..31, ...]: after
    swizzle_weight_frag, the gate/up accumulators for the same output
    column land in the SAME lane of adjacent 16-col fragments, which is
    what gemm_m256's fused swiglu epilogue consumes."""
    two_i, K = w.shape
    assert two_i % 32 == 0
    return w.view(2, two_i // 32, 16, K).transpose(0, 1).reshape(two_i, K)


def gemm_m256_swiglu(
    x: torch.Tensor, w_frag: torch.Tensor, nf: int = 8, variant: int = 1,
    pipe: int = 0,
) -> torch.Tensor:
    """silu(x @ gate.T) * (x @ up.T) in ONE kernel: w_frag is
    swizzle_weight_frag(interleave_gate_up(gate_up)) and the swiglu runs
    in the GEMM epilogue on the fp32 accumulators — the [M, 2I]
    intermediate round trip and the separate swiglu kernel disappear
    (~72 MB of HBM traffic per llama-3-8b layer at M=256)."""
    M, K = x.shape
    N = w_frag.shape[1] * 16
    y = torch.empty((M, N // 2), dtype=torch.bfloat16, device=x.device)
    _native().gemm_m256(y, x, w_frag, None, 1, nf, variant, pipe, 1)
    return y


def _m256_swiglu_config(M: int, N: int, K: int) -> Optional[dict]:
    """Measured dispatch for the FUSED gate_up+swiglu decode MLP front
    (profiles/r02_gemm_m256_sweep.md). N is the stacked 2*intermediate.
    Only the 8B shape measured ahead of library+swiglu (77.2 vs 79.4 us
    cold-L3); the 70B shape loses (304.8 vs 226.6) and stays unfused."""
    if os.environ.get("LLMAPI_NO_FUSED_SWIGLU"):
        return None
    if not (8 < M <= 256):
        return None
    if N == 28672 and K == 4096:  # llama-3-8b tp=1
        if M <= 128:  # 55.0 vs 61.8 us at M=128 (glds variant)
            return {"nf": 8, "variant": 0, "pipe": 0}
        return {"nf": 8, "variant": 1, "pipe": 0}
    if N == 7168 and K == 4096:  # tp=4 gate_up shard: 45.9 vs 46.8 us
        return {"nf": 4, "variant": 0, "pipe": 4}
    return None


def swiglu_linear(
    x: torch.Tensor, w: torch.Tensor,
    w_swz: Optional[torch.Tensor] = None,
    w_int: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """MLP front: swiglu(x @ w.T) with w = [gate; up] stacked. Routes to
    the fused gemm_m256 epilogue when the interleaved twin exists and the
    measured table says it wins; otherwise library GEMM + swiglu kernel."""
    if w_int is not None and x.dim() == 2:
        cfg = _m256_swiglu_config(x.shape[0], w_int.shape[1] * 16, x.shape[1])
        if cfg is not None:
            return gemm_m256_swiglu(x, w_int, **cfg)
    return swiglu(linear(x, w, w_swz))


def linear(
    x: torch.Tensor, w: torch.Tensor, w_swz: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """y = x @ w.T. Decode-shaped bf16 GEMMs (M <= 256) go through the
    macro-tile gfx950 kernel (csrc/gemm_m256.hip) when the fragment-major
    weight twin exists (models/llama.py builds them), through the
    streaming skinny kernel (csrc/gemm_skinny.hip) in the latency regime
    otherwise; everything else through the TunableOp-tuned library GEMMs."""
    route, kw = _route_of(x, w, w_swz)
    if route == "m256":
        return gemm_m256(x, w_swz, **kw)
    if route == "skinny":
        return _gemm_skinny(x, w_swz if kw["swizzled"] else w, kw["swizzled"])
    return torch.nn.functional.linear(x, w)


# ---- fp8 (e4m3) weights: W8A16 decode GEMM (csrc/gemm_w8.hip) ----
_W8_MAX_M = 256  # keep in sync with GS_MAX_M in gemm_stream.h


def w8_reserve_dequant(device, numel: int) -> torch.Tensor:
    """Make the per-device buffer the M > 256 route dequantises into hold at
    least numel bf16. Reserved once at model init, so captured graphs never
    see it move."""
    return _w8_dq.get(device, numel)


def dequant_w8(
    q_frag: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """Fragment-major fp8 twin + scale -> row-major bf16 [N, K]; into `out`
    when given, else into the per-device buffer (valid until the next call)."""
    K, N = q_frag.shape[0] * 64, q_frag.shape[1] * 16
    if not q_frag.is_cuda:
        w = reference.fp8_dequantize_weight(
            reference.unswizzle_weight_frag_fp8(q_frag), scale, torch.bfloat16
        )
        if out is not None:
            out.copy_(w)
            return out
        return w
    if out is None:
        out = w8_reserve_dequant(q_frag.device, N * K)[: N * K].view(N, K)
    _native().dequant_w8(out, q_frag, scale)
    return out


def _w8_gpu_check(x: torch.Tensor) -> None:
    if x.dim() != 2 or x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise RuntimeError(
            "linear_w8 / linear_w4 on GPU need a contiguous 2-D bf16 activation "
            f"(got dim={x.dim()}, dtype={x.dtype}, contiguous={x.is_contiguous()})"
        )


def _w8_m256_default(M: int, N: int, K: int) -> dict:
    """nf and nsk of the macro-tile fp8 kernel where nothing was measured:
    nf by gemm_m256's rule (4 when N % 128 != 0), nsk from _m256_nsk."""
    if N % 128 == 0 and M > 64:
        nf = 8
    else:
        nf = 8 if N // 64 >= 448 else 4
    if N % (16 * nf) != 0:
        nf = 4
    return {"nf": nf, "nsk": _m256_nsk(N, K, nf)}


# (N, K) -> {measured M: (nf, nsk) or None}. Cold-cache sweep over nf in
# {4,8} x nsk in {1,2,4,8} (tools/gemm_w8_bench.py --sweep,
# profiles/r06_w8_macro.md); each comment is "macro vs streaming" in us,
# medians of 3 rounds. A cell is None where no macro configuration's
# three-round range lay wholly below the streaming kernel's.
_W8_M256_TABLE = {
    (6144, 4096): {      # llama-3-8b qkv
        64: (4, 8),      # 17.5 vs 22.3
        128: (4, 8),     # 20.6 vs 36.6
        256: (8, 4),     # 29.2 vs 56.8
    },
    (4096, 4096): {      # llama-3-8b o
        64: None,        # best 17.2 vs 13.4
        128: (4, 8),     # 18.4 vs 20.4
        256: (4, 4),     # 22.0 vs 28.1
    },
    (28672, 4096): {     # llama-3-8b gate_up
        64: (4, 2),      # 40.3 vs 50.5
        128: (8, 2),     # 51.6 vs 92.9
        256: (8, 1),     # 70.5 vs 152.0
    },
    (4096, 14336): {     # llama-3-8b down
        64: None,        # best 31.5 vs 28.1
        128: (4, 8),     # 33.4 vs 49.3
        256: (8, 8),     # 47.0 vs 74.1
    },
    (10240, 8192): {     # llama-3-70b qkv
        64: (8, 8),      # 33.3 vs 54.2
        128: (4, 4),     # 45.0 vs 97.5
        256: (8, 2),     # 74.3 vs 156.3
    },
    (8192, 8192): {      # llama-3-70b o
        64: (4, 8),      # 27.5 vs 29.5
        128: (8, 8),     # 34.7 vs 54.1
        256: (8, 4),     # 51.0 vs 82.6
    },
    (57344, 8192): {     # llama-3-70b gate_up
        64: (4, 1),      # 125.7 vs 199.4
        128: (8, 1),     # 158.4 vs 368.7
        256: (8, 1),     # 267.2 vs 600.3
    },
    (8192, 28672): {     # llama-3-70b down
        64: (4, 8),      # 67.1 vs 93.7
        128: (8, 8),     # 89.6 vs 181.7
        256: (8, 4),     # 145.4 vs 285.1
    },
}
_W8_M256_MS = (64, 128, 256)  # the batch sizes the sweep measured


def _w8_m256_config(M: int, N: int, K: int) -> Optional[dict]:
    """Measured dispatch table of the macro-tile fp8 kernel
    (csrc/gemm_w8_m256.hip) against the streaming fp8 kernel. Returns
    {"nf", "nsk"}, or None to keep the streaming kernel. Only the measured
    shapes have entries. A measured M takes its own cell; an M between two
    measured batch sizes takes the upper one's configuration (the kernel
    runs the same wave count there), and only where the macro kernel won at
    BOTH ends; below the smallest measured M nothing is assumed."""
    row = _W8_M256_TABLE.get((N, K))
    if row is None or not (_W8_M256_MS[0] <= M <= _W8_M256_MS[-1]):
        return None
    hi = next(i for i, m in enumerate(_W8_M256_MS) if m >= M)
    cell = row[_W8_M256_MS[hi]]
    if cell is None or (M != _W8_M256_MS[hi] and row[_W8_M256_MS[hi - 1]] is None):
        return None
    return {"nf": cell[0], "nsk": cell[1]}


def _w8_macro_config(M: int, N: int, K: int) -> Optional[dict]:
    """The macro-tile route of linear_w8 for this call, or None. Opt-in:
    LLMAPI_W8_MACRO_MIN_M=m (read at call time) sends m <= M <= 256 to
    gemm_w8_m256 wherever the measured table has an entry."""
    knob = os.environ.get("LLMAPI_W8_MACRO_MIN_M")
    if not knob or not (int(knob) <= M <= _W8_MAX_M):
        return None
    return _w8_m256_config(M, N, K)


def gemm_w8_m256(
    x: torch.Tensor, q_frag: torch.Tensor, scale: torch.Tensor,
    nf: Optional[int] = None, nsk: Optional[int] = None,
) -> torch.Tensor:
    """y = x @ (scale * q).T on the macro-tile W8A16 kernel
    (csrc/gemm_w8_m256.hip): the structure of the register-staged gemm_m256
    with the fp8 twin converted once per workgroup into the LDS tile.
    M <= 256; nf in {4, 8} is the column-tile width in 16-col fragments."""
    M, K = x.shape
    N = q_frag.shape[1] * 16
    cfg = _w8_m256_default(M, N, K)
    if nf is None:
        nf = cfg["nf"]
    if nsk is None:
        nsk = cfg["nsk"] if nf == cfg["nf"] else _m256_nsk(N, K, nf)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_w8_m256(y, x, q_frag, scale, ws, nsk, nf)
    return y


def gemm_w8_m256_rmsnorm_residual(
    x: torch.Tensor, q_frag: torch.Tensor, scale: torch.Tensor,
    residual: torch.Tensor, norm_w: torch.Tensor, eps: float, nf: int,
    nsk: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rmsnorm_residual(gemm_w8_m256(x, q_frag, scale), residual, norm_w)
    with the residual add and the norm fused into the split-K slab
    reduction; residual is updated in place, bit-identical to the unfused
    pair. Needs nsk > 1."""
    if nsk < 2:
        raise ValueError("fused reduce+norm needs split-K slabs (nsk > 1)")
    return _splitk_norm(
        lambda y, ws, *tail: _native().gemm_w8_m256(
            y, x, q_frag, scale, ws, nsk, nf, *tail
        ),
        x, q_frag.shape[1] * 16, nsk, residual, norm_w, eps,
    )


def linear_w8(
    x: torch.Tensor, q_frag: torch.Tensor, scale: torch.Tensor,
    nsk: Optional[int] = None,
) -> torch.Tensor:
    """y = x @ (scale * q).T with q the fragment-major fp8 e4m3 twin
    (swizzle_weight_frag_fp8) and scale one fp32 per output channel.
    GPU: M <= 256 runs the W8A16 streaming kernel (csrc/gemm_w8.hip),
    larger M dequantises into the per-device bf16 buffer and calls the
    library GEMM. With LLMAPI_W8_MACRO_MIN_M=m set and no explicit nsk,
    m <= M <= 256 runs the macro-tile kernel (csrc/gemm_w8_m256.hip) for
    the shapes _w8_m256_config lists. CPU: the reference."""
    if not x.is_cuda:
        return reference.linear_w8(
            x, reference.unswizzle_weight_frag_fp8(q_frag), scale
        )
    _w8_gpu_check(x)
    M, K = x.shape
    N = q_frag.shape[1] * 16
    if M > _W8_MAX_M:
        return torch.nn.functional.linear(x, dequant_w8(q_frag, scale))
    if nsk is None:
        macro = _w8_macro_config(M, N, K)
        if macro is not None:
            return gemm_w8_m256(x, q_frag, scale, **macro)
        nsk = _w8_nsk(N, K)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_w8(y, x, q_frag, scale, ws, nsk)
    return y


def linear_w8_rmsnorm_residual(
    x: torch.Tensor, q_frag: torch.Tensor, scale: torch.Tensor,
    residual: torch.Tensor, norm_w: torch.Tensor, eps: float = 1e-5,
    nsk: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normed, residual) = rmsnorm_residual(linear_w8(x, q_frag, scale),
    residual, norm_w, eps). On the split-K kernel route (nsk > 1) with a
    covered row width the residual add and the norm run inside the slab
    reduction; bit-identical to the unfused pair, which every other case
    runs (LLMAPI_NO_DECODE_FUSION=1 forces it). The same holds on the
    macro-tile route (LLMAPI_W8_MACRO_MIN_M, see linear_w8) with that
    kernel's nsk."""
    if x.is_cuda and not os.environ.get("LLMAPI_NO_DECODE_FUSION"):
        _w8_gpu_check(x)
        M, K = x.shape
        N = q_frag.shape[1] * 16
        macro = _w8_macro_config(M, N, K) if nsk is None else None
        if macro is not None:
            if (
                macro["nsk"] > 1
                and _reduce_norm_covers(N)
                and residual.is_contiguous()
            ):
                return gemm_w8_m256_rmsnorm_residual(
                    x, q_frag, scale, residual, norm_w, eps, **macro
                )
            return rmsnorm_residual(
                gemm_w8_m256(x, q_frag, scale, **macro), residual, norm_w, eps
            )
        k = _w8_nsk(N, K) if nsk is None else nsk
        if (
            M <= _W8_MAX_M
            and k > 1
            and _reduce_norm_covers(N)
            and residual.is_contiguous()
        ):
            return _splitk_norm(
                lambda y, ws, *tail: _native().gemm_w8(
                    y, x, q_frag, scale, ws, k, *tail
                ),
                x, N, k, residual, norm_w, eps,
            )
    return rmsnorm_residual(linear_w8(x, q_frag, scale, nsk), residual, norm_w, eps)


# ---- MXFP4 weights: W4A16 decode GEMM (csrc/gemm_w4.hip) ----

def dequant_w4(
    q_frag: torch.Tensor, s_frag: torch.Tensor, out: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """Fragment-major MXFP4 twin -> row-major bf16 [N, K]; into `out` when
    given, else into the per-device buffer dequant_w8 uses (valid until the
    next call of either)."""
    K, N = q_frag.shape[0] * 64, q_frag.shape[1] * 16
    if not q_frag.is_cuda:
        w = reference.mxfp4_dequantize_weight(
            *reference.unswizzle_weight_frag_mxfp4(q_frag, s_frag), torch.bfloat16
        )
        if out is not None:
            out.copy_(w)
            return out
        return w
    if out is None:
        out = w8_reserve_dequant(q_frag.device, N * K)[: N * K].view(N, K)
    _native().dequant_w4(out, q_frag, s_frag)
    return out


def _w4_m256_default(M: int, N: int, K: int) -> dict:
    """nf and nsk of the macro-tile MXFP4 kernel where nothing was measured:
    the rule of _w8_m256_default (nf by gemm_m256's rule, nsk from
    _m256_nsk)."""
    return _w8_m256_default(M, N, K)


# (N, K) -> {measured M: (nf, nsk) or None}. Cold-cache sweep over nf in
# {4,8} x nsk in {1,2,4,8} (tools/gemm_w4_bench.py --sweep,
# profiles/r08_w4_macro.md); each comment is "macro vs streaming" in us,
# medians of 3 rounds. A cell is None where no macro configuration's
# three-round range lay wholly below the MXFP4 streaming kernel's.
_W4_M256_TABLE = {
    (6144, 4096): {      # llama-3-8b qkv
        64: (4, 8),      # 19.1 vs 22.3
        128: (8, 8),     # 22.8 vs 38.6
        256: (8, 4),     # 28.4 vs 56.8
    },
    (4096, 4096): {      # llama-3-8b o
        64: None,        # best 16.2 vs 12.8
        128: (4, 4),     # 19.3 vs 20.3
        256: (4, 4),     # 22.5 vs 28.9
    },
    (28672, 4096): {     # llama-3-8b gate_up
        64: (4, 2),      # 38.2 vs 49.4
        128: (4, 1),     # 49.9 vs 94.5
        256: (8, 1),     # 67.6 vs 152.5
    },
    (4096, 14336): {     # llama-3-8b down
        64: None,        # best 29.9 vs 26.6
        128: (4, 8),     # 32.2 vs 47.1
        256: (8, 8),     # 44.4 vs 73.2
    },
    (10240, 8192): {     # llama-3-70b qkv
        64: (8, 8),      # 31.4 vs 51.4
        128: (4, 4),     # 43.3 vs 98.6
        256: (4, 4),     # 72.3 vs 156.4
    },
    (8192, 8192): {      # llama-3-70b o
        64: (4, 8),      # 24.9 vs 29.7
        128: (8, 8),     # 33.0 vs 52.2
        256: (8, 4),     # 49.0 vs 82.5
    },
    (57344, 8192): {     # llama-3-70b gate_up
        64: (4, 1),      # 111.8 vs 188.5
        128: (8, 1),     # 151.8 vs 369.5
        256: (8, 1),     # 251.9 vs 595.1
    },
    (8192, 28672): {     # llama-3-70b down
        64: (4, 8),      # 62.0 vs 95.1
        128: (8, 8),     # 84.3 vs 171.7
        256: (8, 4),     # 139.0 vs 269.3
    },
}
_W4_M256_MS = (64, 128, 256)  # the batch sizes the sweep measured


def _w4_m256_config(M: int, N: int, K: int) -> Optional[dict]:
    """Measured dispatch table of the macro-tile MXFP4 kernel
    (csrc/gemm_w4_m256.hip) against the streaming MXFP4 kernel. Returns
    {"nf", "nsk"}, or None to keep the streaming kernel. The lookup is
    _w8_m256_config's: only the measured shapes have entries; a measured M
    takes its own cell; an M between two measured batch sizes takes the
    upper one's configuration, and only where the macro kernel won at BOTH
    ends; below the smallest measured M nothing is assumed."""
    row = _W4_M256_TABLE.get((N, K))
    if row is None or not (_W4_M256_MS[0] <= M <= _W4_M256_MS[-1]):
        return None
    hi = next(i for i, m in enumerate(_W4_M256_MS) if m >= M)
    cell = row[_W4_M256_MS[hi]]
    if cell is None or (M != _W4_M256_MS[hi] and row[_W4_M256_MS[hi - 1]] is None):
        return None
    return {"nf": cell[0], "nsk": cell[1]}


def _w4_macro_config(M: int, N: int, K: int) -> Optional[dict]:
    """The macro-tile route of linear_w4 for this call, or None. Opt-in:
    LLMAPI_W4_MACRO_MIN_M=m (read at call time) sends m <= M <= 256 to
    gemm_w4_m256 wherever the measured table has an entry."""
    knob = os.environ.get("LLMAPI_W4_MACRO_MIN_M")
    if not knob or not (int(knob) <= M <= _W8_MAX_M):
        return None
    return _w4_m256_config(M, N, K)


def gemm_w4_m256(
    x: torch.Tensor, q_frag: torch.Tensor, s_frag: torch.Tensor,
    nf: Optional[int] = None, nsk: Optional[int] = None,
) -> torch.Tensor:
    """y = x @ dequant(q, s).T on the macro-tile W4A16 kernel
    (csrc/gemm_w4_m256.hip): the structure of gemm_w8_m256 with the MXFP4
    twin converted once per workgroup into the LDS tile. M <= 256; nf in
    {4, 8} is the column-tile width in 16-col fragments."""
    M, K = x.shape
    N = q_frag.shape[1] * 16
    cfg = _w4_m256_default(M, N, K)
    if nf is None:
        nf = cfg["nf"]
    if nsk is None:
        nsk = cfg["nsk"] if nf == cfg["nf"] else _m256_nsk(N, K, nf)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_w4_m256(y, x, q_frag, s_frag, ws, nsk, nf)
    return y


def gemm_w4_m256_rmsnorm_residual(
    x: torch.Tensor, q_frag: torch.Tensor, s_frag: torch.Tensor,
    residual: torch.Tensor, norm_w: torch.Tensor, eps: float, nf: int,
    nsk: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rmsnorm_residual(gemm_w4_m256(x, q_frag, s_frag), residual, norm_w)
    with the residual add and the norm fused into the split-K slab
    reduction; residual is updated in place, bit-identical to the unfused
    pair. Needs nsk > 1."""
    if nsk < 2:
        raise ValueError("fused reduce+norm needs split-K slabs (nsk > 1)")
    return _splitk_norm(
        lambda y, ws, *tail: _native().gemm_w4_m256(
            y, x, q_frag, s_frag, ws, nsk, nf, *tail
        ),
        x, q_frag.shape[1] * 16, nsk, residual, norm_w, eps,
    )


def linear_w4(
    x: torch.Tensor, q_frag: torch.Tensor, s_frag: torch.Tensor,
    nsk: Optional[int] = None,
) -> torch.Tensor:
    """y = x @ dequant(q, s).T with (q_frag, s_frag) the fragment-major
    MXFP4 twin (swizzle_weight_frag_mxfp4): e2m1 nibbles and one e8m0 scale
    per 32 k of a row. GPU: M <= 256 runs the W4A16 streaming kernel
    (csrc/gemm_w4.hip), larger M dequantises into the per-device bf16 buffer
    and calls the library GEMM. With LLMAPI_W4_MACRO_MIN_M=m set and no
    explicit nsk, m <= M <= 256 runs the macro-tile kernel
    (csrc/gemm_w4_m256.hip) for the shapes _w4_m256_config lists. CPU: the
    reference."""
    if not x.is_cuda:
        return reference.linear_w4(
            x, *reference.unswizzle_weight_frag_mxfp4(q_frag, s_frag)
        )
    _w8_gpu_check(x)
    M, K = x.shape
    N = q_frag.shape[1] * 16
    if M > _W8_MAX_M:
        return torch.nn.functional.linear(x, dequant_w4(q_frag, s_frag))
    if nsk is None:
        macro = _w4_macro_config(M, N, K)
        if macro is not None:
            return gemm_w4_m256(x, q_frag, s_frag, **macro)
        nsk = _w4_nsk(N, K)
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ws = _slabs.get(x.device, nsk * M * N) if nsk > 1 else None
    _native().gemm_w4(y, x, q_frag, s_frag, ws, nsk)
    return y


def linear_w4_rmsnorm_residual(
    x: torch.Tensor, q_frag: torch.Tensor, s_frag: torch.Tensor,
    residual: torch.Tensor, norm_w: torch.Tensor, eps: float = 1e-5,
    nsk: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normed, residual) = rmsnorm_residual(linear_w4(x, q_frag, s_frag),
    residual, norm_w, eps). On the split-K kernel route (nsk > 1) with a
    covered row width the residual add and the norm run inside the slab
    reduction; bit-identical to the unfused pair, which every other case
    runs (LLMAPI_NO_DECODE_FUSION=1 forces it). The same holds on the
    macro-tile route (LLMAPI_W4_MACRO_MIN_M, see linear_w4) with that
    kernel's nsk."""
    if x.is_cuda and not os.environ.get("LLMAPI_NO_DECODE_FUSION"):
        _w8_gpu_check(x)
        M, K = x.shape
        N = q_frag.shape[1] * 16
        macro = _w4_macro_config(M, N, K) if nsk is None else None
        if macro is not None:
            if (
                macro["nsk"] > 1
                and _reduce_norm_covers(N)
                and residual.is_contiguous()
            ):
                return gemm_w4_m256_rmsnorm_residual(
                    x, q_frag, s_frag, residual, norm_w, eps, **macro
                )
            return rmsnorm_residual(
                gemm_w4_m256(x, q_frag, s_frag, **macro), residual, norm_w, eps
            )
        k = _w4_nsk(N, K) if nsk is None else nsk
        if (
            M <= _W8_MAX_M
            and k > 1
            and _reduce_norm_covers(N)
            and residual.is_contiguous()
        ):
            return _splitk_norm(
                lambda y, ws, *tail: _native().gemm_w4(
                    y, x, q_frag, s_frag, ws, k, *tail
                ),
                x, N, k, residual, norm_w, eps,
            )
    return rmsnorm_residual(linear_w4(x, q_frag, s_frag, nsk), residual, norm_w, eps)


# ---- multi-LoRA: batched-gather adapter kernels (csrc/lora.hip) ----
LORA_MAX_RANK = 64  # keep in sync with LORA_MAX_R in lora.hip


def lora_padded_rank(rank: int) -> int:
    """The stack width R for adapters of up to `rank`: the next multiple
    of 8 (one 16-byte vector of a B row), at most LORA_MAX_RANK."""
    if not (1 <= rank <= LORA_MAX_RANK):
        raise ValueError(f"LoRA rank must be in [1, {LORA_MAX_RANK}], got {rank}")
    return -(-rank // 8) * 8


class LoraStack:
    """The adapter slots of ONE projection: A [S, nseg*R, K] and B [S, N, R]
    in the activation dtype, zero where a slot is empty or its adapter's
    rank is below R. ranks (int32 [S], true rank per slot) and scales (fp32
    [S], alpha / r) are shared by all stacks of a model. seg_bounds are the
    end columns of the nseg output segments (q | k | v, gate | up); the
    last is N. Allocated once: captured graphs hold these addresses."""

    def __init__(self, A, B, ranks, scales, seg_bounds):
        self.A, self.B, self.ranks, self.scales = A, B, ranks, scales
        self.seg_bounds = tuple(int(b) for b in seg_bounds)
        self.nseg = len(self.seg_bounds)
        self.R = B.shape[2]
        if A.shape[1] != self.nseg * self.R or self.seg_bounds[-1] != B.shape[1]:
            raise ValueError("LoraStack: A/B/seg_bounds do not fit together")


_lora_t = _Scratch(torch.float32)  # shrink output t between the two kernels


def _lora_gpu_check(t: torch.Tensor, what: str, dtype: torch.dtype) -> None:
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(
            f"LoRA ops on GPU need {what} as a contiguous {dtype} GPU tensor "
            f"(got device={t.device}, dtype={t.dtype}, "
            f"contiguous={t.is_contiguous()})"
        )


def lora_shrink(
    x: torch.Tensor, A: torch.Tensor, ranks: torch.Tensor,
    adapter_ids: torch.Tensor, nseg: int, out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """t [T, nseg*R] fp32 with t[row, s*R + j] = sum_k x[row, k] *
    A[slot, s*R + j, k], slot = adapter_ids[row]. On the GPU a row of slot
    -1 and the columns j >= ranks[slot] are NOT written (lora_expand reads
    neither); t is `out` when given, else a view of the per-device scratch,
    valid until the next call. CPU: the reference, which zeroes them."""
    if not x.is_cuda:
        t = reference.lora_shrink(x, A, ranks, adapter_ids, nseg)
        if out is not None:
            out.copy_(t)
            return out
        return t
    _lora_gpu_check(x, "x", torch.bfloat16)
    _lora_gpu_check(A, "A", torch.bfloat16)
    _lora_gpu_check(ranks, "ranks", torch.int32)
    _lora_gpu_check(adapter_ids, "adapter_ids", torch.int32)
    T, nR = x.shape[0], A.shape[1]
    if out is None:
        out = _lora_t.get(x.device, T * nR)[: T * nR].view(T, nR)
    _native().lora_shrink(out, x, A, ranks, adapter_ids, int(nseg))
    return out


def lora_expand(
    y: torch.Tensor, t: torch.Tensor, B: torch.Tensor, ranks: torch.Tensor,
    scales: torch.Tensor, adapter_ids: torch.Tensor, seg_bounds,
) -> torch.Tensor:
    """In place on y [T, N]: y[row, n] = bf16(float(y[row, n]) +
    scales[slot] * sum_j t[row, seg(n)*R + j] * B[slot, n, j]); a row of
    slot -1 keeps its bits. seg_bounds: end column of each segment (up to
    three, multiples of 8, the last one N). Returns y."""
    seg_bounds = tuple(int(b) for b in seg_bounds)
    N = y.shape[1]
    if not (1 <= len(seg_bounds) <= 3) or seg_bounds[-1] != N:
        raise ValueError(f"seg_bounds {seg_bounds} must be 1-3 ends, the last {N}")
    if not y.is_cuda:
        return reference.lora_expand(y, t, B, ranks, scales, adapter_ids, seg_bounds)
    _lora_gpu_check(y, "y", torch.bfloat16)
    _lora_gpu_check(B, "B", torch.bfloat16)
    _lora_gpu_check(t, "t", torch.float32)
    _lora_gpu_check(ranks, "ranks", torch.int32)
    _lora_gpu_check(scales, "scales", torch.float32)
    _lora_gpu_check(adapter_ids, "adapter_ids", torch.int32)
    starts = seg_bounds[:-1] + (N, N)  # a segment that is not there starts at N
    _native().lora_expand(
        y, t, B, ranks, scales, adapter_ids, len(seg_bounds), starts[0], starts[1]
    )
    return y


def lora_add(
    y: torch.Tensor, x: torch.Tensor, stack: LoraStack, adapter_ids: torch.Tensor
) -> torch.Tensor:
    """y += scale * B (A x) per row, in place on the projection's output y
    = W x: lora_shrink then lora_expand over one projection's stack."""
    t = lora_shrink(x, stack.A, stack.ranks, adapter_ids, stack.nseg)
    return lora_expand(
        y, t, stack.B, stack.ranks, stack.scales, adapter_ids, stack.seg_bounds
    )


def topk_topp_filter(
    logits: torch.Tensor, topp: torch.Tensor, topk: torch.Tensor
) -> torch.Tensor:
    """Mask logits outside the per-row top-k / top-p set to -inf, in
    place, and return logits. GPU: histogram-threshold kernel
    (csrc/sampling.hip, no sort, no host loop); CPU: batched torch sort
    (reference semantics)."""
    if logits.is_cuda:
        _native().topk_topp_filter(logits, topp, topk)
        return logits
    return reference.topk_topp_filter(logits, topp, topk)


def sample(
    logits: torch.Tensor,
    temperature: torch.Tensor,
    noise: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
        _native().sample(out, logits, temperature, noise)
        return out
    return reference.sample(logits, temperature, noise)


__all__ = [
    "have_native",
    "build_rope_cache",
    "rmsnorm",
    "rmsnorm_residual",
    "rope_inplace",
    "rope_and_kv_write",
    "swiglu",
    "kv_cache_write",
    "linear",
    "gemm_m256",
    "gemm_m256_rmsnorm_residual",
    "linear_rmsnorm_residual",
    "swizzle_weight",
    "swizzle_weight_frag",
    "fp8_quantize_weight",
    "fp8_dequantize_weight",
    "swizzle_weight_frag_fp8",
    "unswizzle_weight_frag_fp8",
    "linear_w8",
    "linear_w8_rmsnorm_residual",
    "gemm_w8_m256",
    "gemm_w8_m256_rmsnorm_residual",
    "dequant_w8",
    "w8_reserve_dequant",
    "mxfp4_quantize_weight",
    "mxfp4_dequantize_weight",
    "swizzle_weight_frag_mxfp4",
    "unswizzle_weight_frag_mxfp4",
    "linear_w4",
    "linear_w4_rmsnorm_residual",
    "gemm_w4_m256",
    "gemm_w4_m256_rmsnorm_residual",
    "dequant_w4",
    "LoraStack",
    "lora_padded_rank",
    "lora_shrink",
    "lora_expand",
    "lora_add",
    "attention_prefill",
    "attention_decode",
    "sample",
    "topk_topp_filter",
    "reference",
]
