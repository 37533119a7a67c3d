"""Pure-PyTorch fp32 reference implementations of every engine op.

These are the *semantic contract* for the HIP kernels in csrc/: GPU numerics
tests compare each gfx950 kernel against these (run in fp32) per-shape, and
the CPU engine path runs on them directly so the whole gateway + engine
stack is testable without a GPU.

Shapes (T = total tokens in a varlen batch, B = sequences, D = head dim):
- rmsnorm:            x [T, H]          -> y [T, H]
- rmsnorm_residual:   x, residual       -> (y, x+residual)
- rope_inplace:       q [T, Hq, D], k [T, Hkv, D], positions [T]
- swiglu:             x [T, 2I]         -> silu(x[:, :I]) * x[:, I:]
- kv_cache_write:     k/v [T, Hkv, D] -> cache [nblocks, Hkv, block, D]
- attention_prefill:  varlen causal flash (q [T,Hq,D], k/v [T,Hkv,D], cu_seqlens)
- attention_decode:   q [B, Hq, D] vs paged cache via block_tables
- sample:             logits [B, V] (+ per-seq temperature, optional noise)
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    dtype = x.dtype
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    y = xf * torch.rsqrt(var + eps) * weight.float()
    return y.to(dtype)


def rmsnorm_residual(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> Tuple[torch.Tensor, torch.Tensor]:
    r = (x.float() + residual.float()).to(x.dtype)
    return rmsnorm(r, weight, eps), r


def linear_rmsnorm_residual(
    x: torch.Tensor, w: torch.Tensor, residual: torch.Tensor,
    norm_w: torch.Tensor, eps: float = 1e-5,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Projection followed by the residual-add norm (what the GPU path
    fuses into the split-K reduction): y = x @ w.T rounded to the input
    dtype, then rmsnorm_residual(y, residual)."""
    y = torch.nn.functional.linear(x, w)
    return rmsnorm_residual(y, residual, norm_w, eps)


def build_rope_cache(
    max_positions: int, head_dim: int, theta: float = 500000.0, device="cpu"
) -> torch.Tensor:
    """Return [max_positions, head_dim] fp32 cache: [cos(half) | sin(half)]."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half, dtype=torch.float32, device=device) / half))
    pos = torch.arange(max_positions, dtype=torch.float32, device=device)
    ang = torch.outer(pos, inv_freq)  # [P, half]
    return torch.cat([ang.cos(), ang.sin()], dim=-1).contiguous()


def rope_inplace(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor
) -> None:
    """Llama-style rotate-half RoPE applied in place to q and k."""
    half = q.shape[-1] // 2
    cs = cos_sin[positions]  # [T, D]
    cos = cs[:, :half].unsqueeze(1)  # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1)
    for t in (q, k):
        tf = t.float()
        x1, x2 = tf[..., :half], tf[..., half:]
        t[..., :half] = (x1 * cos - x2 * sin).to(t.dtype)
        t[..., half:] = (x2 * cos + x1 * sin).to(t.dtype)


def swiglu(x: torch.Tensor) -> torch.Tensor:
    inter = x.shape[-1] // 2
    g = x[..., :inter].float()
    u = x[..., inter:].float()
    return (g * torch.sigmoid(g) * u).to(x.dtype)


# ---- multi-LoRA: y = W x + scale * B (A x), adapter slot per row ----
# A [S, nseg*R, K], B [S, N, R]; ranks int32 [S] (true rank of a slot, the
# rest of R is zero padding), scales fp32 [S] (alpha / r), adapter_ids int32
# [T] (-1 = base model). seg_bounds are the END columns of the nseg output
# segments (the last one is N): segment s of y reads rows [s*R, (s+1)*R) of t.

def lora_shrink(
    x: torch.Tensor, A: torch.Tensor, ranks: torch.Tensor,
    adapter_ids: torch.Tensor, nseg: int,
) -> torch.Tensor:
    """t[row, s*R + j] = sum_k x[row, k] * A[slot, s*R + j, k] in fp32;
    zero for j >= rank[slot] and for rows of slot -1 (the GPU kernel does
    not write those)."""
    T = x.shape[0]
    R = A.shape[1] // nseg
    t = torch.zeros(T, nseg * R, dtype=torch.float32, device=x.device)
    live = (torch.arange(R, device=x.device).unsqueeze(0)
            < ranks.to(torch.long).unsqueeze(1)).repeat(1, nseg)  # [S, nseg*R]
    for slot in torch.unique(adapter_ids).tolist():
        if slot < 0:
            continue
        rows = adapter_ids == slot
        t[rows] = (x[rows].float() @ A[slot].float().T) * live[slot].float()
    return t


def lora_expand(
    y: torch.Tensor, t: torch.Tensor, B: torch.Tensor, ranks: torch.Tensor,
    scales: torch.Tensor, adapter_ids: torch.Tensor, seg_bounds,
) -> torch.Tensor:
    """In place: y[row, n] = (float(y[row, n]) + scale[slot] * sum_j
    t[row, seg(n)*R + j] * B[slot, n, j]) rounded to y's dtype; rows of
    slot -1 are not touched."""
    R = B.shape[2]
    for slot in torch.unique(adapter_ids).tolist():
        if slot < 0:
            continue
        rows = adapter_ids == slot
        r = int(ranks[slot])
        tr = t[rows]
        yr = y[rows].float()
        lo = 0
        for s, hi in enumerate(seg_bounds):
            yr[:, lo:hi] += float(scales[slot]) * (
                tr[:, s * R : s * R + r] @ B[slot, lo:hi, :r].float().T
            )
            lo = hi
        y[rows] = yr.to(y.dtype)
    return y


FP8_MAX = 448.0  # e4m3fn


def fp8_quantize_rows(x: torch.Tensor):
    """Per-row (last-dim) e4m3 quantization: returns (uint8 bits, scales).
    x: [..., D] -> bits [..., D] uint8, scales [...] fp32."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (xf / scale.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def fp8_dequantize_rows(bits: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return bits.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1).float()


def fp8_quantize_weight(w: torch.Tensor):
    """Weight quantisation to e4m3fn, one scale per output channel:
    w [N, K] -> (bits uint8 [N, K], scale fp32 [N]).

    The scale is the smallest power of two s with amax/s <= 448 (an
    all-zero row gets 1). e4m3 is a floating format, so a power-of-two
    scale costs no relative precision, and bits*scale is exactly
    representable in bf16 (3 mantissa bits, exponent shift only)."""
    wf = w.float()
    amax = wf.abs().amax(dim=-1)
    # amax/448 = m * 2^e with m in [0.5, 1): the smallest power of two not
    # below it is 2^(e-1) when m == 0.5 exactly, else 2^e
    m, e = torch.frexp(amax / FP8_MAX)
    e = torch.where(m == 0.5, e - 1, e)
    scale = torch.where(
        amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax)
    )
    # the clamp only guards the rounding of amax/448 itself (torch's e4m3fn
    # cast does not saturate)
    q = (wf / scale.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def fp8_dequantize_weight(
    q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16
) -> torch.Tensor:
    """bits [N, K] * scale [N] -> [N, K]; exact for bf16 (and wider)."""
    return (q.view(torch.float8_e4m3fn).float() * scale.float().unsqueeze(-1)).to(dtype)


def swizzle_weight_frag_fp8(q: torch.Tensor) -> torch.Tensor:
    """bits [N, K] -> fragment-major [K/64, N/16, 64, 16] for gemm_w8.

    [k64][n16][lane][j] = q[n16*16 + (lane&15)][k64*64 + (j>>3)*32 +
    (lane>>4)*8 + (j&7)]: each 1 KiB row is one wave's
    mfma_f32_16x16x32_bf16 B-fragments for two consecutive k-steps, one
    16-byte load per lane (the swizzle_weight_frag fragment convention)."""
    N, K = q.shape
    assert K % 64 == 0 and N % 64 == 0
    # k = k64*64 + h*32 + g*8 + e, n = n16*16 + r; lane = g*16 + r, j = h*8 + e
    return (
        q.view(N // 16, 16, K // 64, 2, 4, 8)
        .permute(2, 0, 4, 1, 3, 5)
        .reshape(K // 64, N // 16, 64, 16)
        .contiguous()
    )


def unswizzle_weight_frag_fp8(q_frag: torch.Tensor) -> torch.Tensor:
    """Inverse of swizzle_weight_frag_fp8: [K/64, N/16, 64, 16] -> [N, K]."""
    k64, n16 = q_frag.shape[0], q_frag.shape[1]
    return (
        q_frag.view(k64, n16, 4, 16, 2, 8)
        .permute(1, 3, 0, 4, 2, 5)
        .reshape(n16 * 16, k64 * 64)
        .contiguous()
    )


def linear_w8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """y = x @ (scale * q).T with q the row-major e4m3 bits [N, K]."""
    w = fp8_dequantize_weight(q, scale, torch.float32)
    return (x.float() @ w.T).to(x.dtype)


# OCP MXFP4: e2m1 elements (sign, 2 exponent bits, 1 mantissa bit), one e8m0
# power-of-two scale per block of 32 consecutive k. The 16 element codes:
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_E2M1_TABLE = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32)
MXFP4_BLOCK = 32


def mxfp4_quantize_weight(w: torch.Tensor):
    """Weight quantisation to MXFP4: w [N, K] -> (packed uint8 [N, K/2],
    scale uint8 [N, K/32]).

    A block is 32 consecutive k of one row. Its scale is the smallest power
    of two s with amax/s <= 6, so nothing clips (the rule of
    fp8_quantize_weight), stored as e8m0: byte = exponent + 127 with the
    exponent clamped to [-126, 127] (bytes 0 and 255 never appear); an
    all-zero block gets byte 127. Elements round to nearest-even onto the
    e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} x sign; even k sits in the low
    nibble of a byte, odd k in the high nibble."""
    N, K = w.shape
    assert K % MXFP4_BLOCK == 0
    b = w.float().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = b.abs().amax(dim=-1)
    # amax = m * 2^e with m in [0.5, 1), and 6 * 2^t = 0.75 * 2^(t+3): the
    # smallest t with amax <= 6 * 2^t is e-3 when m <= 0.75, else e-2
    m, e = torch.frexp(amax)
    t = torch.where(m <= 0.75, e - 3, e - 2).clamp(-126, 127)
    t = torch.where(amax > 0, t, torch.zeros_like(t))
    v = b / torch.ldexp(torch.ones_like(amax), t).unsqueeze(-1)
    # round to nearest, ties to the even code: the grid step is 0.5 below 2,
    # 1 below 4 and 2 above, and torch.round's even multiple of the step is
    # the code with a clear mantissa bit. |v| <= 6 by the choice of t (the
    # exponent clamp can only raise t).
    a = v.abs()
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
    g = torch.round(a / step) * step
    code = torch.where(g < 2, g * 2, torch.where(g <= 4, g + 2, torch.full_like(g, 7)))
    code = code.to(torch.uint8) | (((v < 0) & (g > 0)).to(torch.uint8) << 3)
    code = code.view(N, K)
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    return packed.contiguous(), (t + 127).to(torch.uint8)


def mxfp4_dequantize_weight(
    packed: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16
) -> torch.Tensor:
    """packed [N, K/2], scale [N, K/32] -> [N, K]; exact for bf16 (and
    wider): one mantissa bit, and the scale only shifts the exponent."""
    N, K = packed.shape[0], packed.shape[1] * 2
    codes = torch.stack([packed & 15, packed >> 4], dim=-1).view(N, K)
    vals = _E2M1_TABLE.to(packed.device)[codes.long()]
    s = torch.ldexp(
        torch.ones(scale.shape, dtype=torch.float32, device=scale.device),
        scale.to(torch.int32) - 127,
    )
    blocks = vals.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * s.unsqueeze(-1)
    return blocks.view(N, K).to(dtype)


def swizzle_weight_frag_mxfp4(packed: torch.Tensor, scale: torch.Tensor):
    """packed [N, K/2], scale [N, K/32] -> fragment-major (q_frag
    [K/64, N/16, 64, 8], s_frag [K/64, N/64, 16, 8]) for gemm_w4.

    q_frag[k64][n16][lane][j] = packed[n16*16 + (lane&15)][k64*32 +
    (j>>2)*16 + (lane>>4)*4 + (j&3)]: the fp8 fragment convention in
    nibbles — each 512 B row is one wave's mfma_f32_16x16x32_bf16
    B-fragments for two consecutive k-steps (bytes 0-3 then 4-7), one 8-byte
    load per lane; the nibble order inside a byte is unchanged.
    s_frag[k64][n64][r][f*2 + h] = scale[n64*64 + f*16 + r][k64*2 + h]: the
    8 bytes at [r] are the block scales lane r (and r+16, r+32, r+48) needs
    for its four n-fragments f and two k32 halves h of that step."""
    N, K = packed.shape[0], packed.shape[1] * 2
    assert K % 64 == 0 and N % 64 == 0
    assert scale.shape == (N, K // MXFP4_BLOCK)
    # byte = k64*32 + h*16 + g*4 + e, n = n16*16 + r; lane = g*16 + r, j = h*4 + e
    q_frag = (
        packed.view(N // 16, 16, K // 64, 2, 4, 4)
        .permute(2, 0, 4, 1, 3, 5)
        .reshape(K // 64, N // 16, 64, 8)
        .contiguous()
    )
    s_frag = (
        scale.view(N // 64, 4, 16, K // 64, 2)
        .permute(3, 0, 2, 1, 4)
        .reshape(K // 64, N // 64, 16, 8)
        .contiguous()
    )
    return q_frag, s_frag


def unswizzle_weight_frag_mxfp4(q_frag: torch.Tensor, s_frag: torch.Tensor):
    """Inverse of swizzle_weight_frag_mxfp4: -> (packed [N, K/2], scale
    [N, K/32])."""
    k64, n16 = q_frag.shape[0], q_frag.shape[1]
    packed = (
        q_frag.view(k64, n16, 4, 16, 2, 4)
        .permute(1, 3, 0, 4, 2, 5)
        .reshape(n16 * 16, k64 * 32)
        .contiguous()
    )
    scale = (
        s_frag.view(k64, n16 // 4, 16, 4, 2)
        .permute(1, 3, 2, 0, 4)
        .reshape(n16 * 16, k64 * 2)
        .contiguous()
    )
    return packed, scale


def linear_w4(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """y = x @ dequant(packed, scale).T with the row-major MXFP4 pair."""
    w = mxfp4_dequantize_weight(packed, scale, torch.float32)
    return (x.float() @ w.T).to(x.dtype)


def kv_cache_write(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale: "Optional[torch.Tensor]" = None,
    v_scale: "Optional[torch.Tensor]" = None,
) -> None:
    """Scatter new K/V rows into the paged cache.

    cache layout: [num_blocks, num_kv_heads, block_size, head_dim];
    slot_mapping[t] = block_id * block_size + block_offset.
    """
    block_size = k_cache.shape[2]
    blocks = torch.div(slot_mapping, block_size, rounding_mode="floor")
    offs = slot_mapping % block_size
    if k_scale is not None:  # fp8 e4m3 cache with per-row scales
        kq, ks = fp8_quantize_rows(k)
        vq, vs = fp8_quantize_rows(v)
        k_cache[blocks, :, offs, :] = kq
        v_cache[blocks, :, offs, :] = vq
        k_scale[blocks, :, offs] = ks
        v_scale[blocks, :, offs] = vs
        return
    k_cache[blocks, :, offs, :] = k.to(k_cache.dtype)
    v_cache[blocks, :, offs, :] = v.to(v_cache.dtype)


def attention_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    scale: Optional[float] = None,
    causal: bool = True,
    k_cache: Optional[torch.Tensor] = None,
    v_cache: Optional[torch.Tensor] = None,
    block_tables: Optional[torch.Tensor] = None,
    cached_lens: Optional[torch.Tensor] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = None,
) -> torch.Tensor:
    """Varlen causal attention with GQA over fresh K/V; with cached_lens,
    each sequence also attends (unmasked) to its cached prefix gathered
    from the paged cache (prefix caching / chunked prefill).

    window = W > 0 (sliding-window attention): the row at absolute position
    p (cached_lens + its row index) attends to keys p - W < j <= p only,
    across the cached prefix and the fresh tokens alike; cache blocks that
    lie wholly below the first row's window are not read."""
    W = int(window or 0)
    if W < 0:
        raise ValueError(f"window must be >= 0, got {window}")
    if W and not causal:
        raise ValueError("a sliding window needs causal=True")
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    group = Hq // Hkv
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    out = torch.empty_like(q)
    cu = cu_seqlens.tolist()
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        L = e - s
        qi = q[s:e].float()  # [L, Hq, D]
        ki = k[s:e].float().repeat_interleave(group, dim=1)
        vi = v[s:e].float().repeat_interleave(group, dim=1)
        nc = int(cached_lens[i]) if cached_lens is not None else 0
        # first cached position inside the window of fresh row 0
        lo = max(nc - W + 1, 0) if W else 0
        if nc > lo:
            bs = k_cache.shape[2]
            rows_k, rows_v = [], []
            for pos in range(lo, nc):
                blk = int(block_tables[i, pos // bs])
                kr = k_cache[blk, :, pos % bs, :]
                vr = v_cache[blk, :, pos % bs, :]
                if k_scale is not None:
                    kr = fp8_dequantize_rows(kr, k_scale[blk, :, pos % bs])
                    vr = fp8_dequantize_rows(vr, v_scale[blk, :, pos % bs])
                rows_k.append(kr)
                rows_v.append(vr)
            kc = torch.stack(rows_k).float().repeat_interleave(group, dim=1)
            vc = torch.stack(rows_v).float().repeat_interleave(group, dim=1)
            ki = torch.cat([kc, ki], dim=0)
            vi = torch.cat([vc, vi], dim=0)
        scores = torch.einsum("qhd,khd->hqk", qi, ki) * scale
        if causal:
            mask = torch.triu(
                torch.ones(L, L, dtype=torch.bool, device=q.device), diagonal=1
            )
            if nc > lo:  # cached keys precede every fresh row: never masked
                mask = torch.cat(
                    [torch.zeros(L, nc - lo, dtype=torch.bool, device=q.device), mask],
                    dim=1,
                )
            if W:  # column c is absolute key lo + c, row r absolute nc + r
                row = torch.arange(L, device=q.device)[:, None] + nc
                col = torch.arange(mask.shape[1], device=q.device)[None, :] + lo
                mask = mask | (col <= row - W)
            scores.masked_fill_(mask, float("-inf"))
        p = torch.softmax(scores, dim=-1)
        out[s:e] = torch.einsum("hqk,khd->qhd", p, vi).to(q.dtype)
    return out


def attention_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: Optional[float] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = None,
) -> torch.Tensor:
    """Single-token decode attention over the paged KV cache. window = W > 0
    (sliding-window attention) uses keys [max(0, L - W), L) only and reads
    no block that lies wholly below them."""
    W = int(window or 0)
    if W < 0:
        raise ValueError(f"window must be >= 0, got {window}")
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    block_size = k_cache.shape[2]
    group = Hq // Hkv
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    out = torch.empty_like(q)
    for b in range(B):
        L = int(context_lens[b])
        nblocks = (L + block_size - 1) // block_size
        lo = max(L - W, 0) if W else 0
        b0 = lo // block_size       # first block of the window
        lo, L = lo - b0 * block_size, L - b0 * block_size
        blocks = block_tables[b, b0:nblocks].long()
        # gather [L, Hkv, D], then keep [lo, L)
        if k_scale is not None:
            kd = fp8_dequantize_rows(k_cache[blocks], k_scale[blocks])
            vd = fp8_dequantize_rows(v_cache[blocks], v_scale[blocks])
            kk = kd.permute(0, 2, 1, 3).reshape(-1, Hkv, D)[lo:L].float()
            vv = vd.permute(0, 2, 1, 3).reshape(-1, Hkv, D)[lo:L].float()
        else:
            kk = k_cache[blocks].permute(0, 2, 1, 3).reshape(-1, Hkv, D)[lo:L].float()
            vv = v_cache[blocks].permute(0, 2, 1, 3).reshape(-1, Hkv, D)[lo:L].float()
        kk = kk.repeat_interleave(group, dim=1)  # [L, Hq, D]
        vv = vv.repeat_interleave(group, dim=1)
        qb = q[b].float()  # [Hq, D]
        scores = torch.einsum("hd,khd->hk", qb, kk) * scale
        p = torch.softmax(scores, dim=-1)
        out[b] = torch.einsum("hk,khd->hd", p, vv).to(q.dtype)
    return out


def sample(
    logits: torch.Tensor,
    temperature: torch.Tensor,
    noise: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Greedy when temperature<=0, else Gumbel-max sampling.

    temperature: [B] fp32; noise: [B, V] uniform(0,1) — supplied by the
    caller so GPU and CPU paths can be compared with identical randomness.
    """
    B, V = logits.shape
    lf = logits.float()
    temps = temperature.view(B, 1).float()
    greedy = temps <= 0
    if noise is None or bool(greedy.all()):
        return lf.argmax(dim=-1)
    u = noise.float().clamp_min(1e-20)
    inner = (-torch.log(u)).clamp_min(1e-20)
    gumbel = -torch.log(inner)
    scored = torch.where(greedy, lf, lf / temps.clamp_min(1e-6) + gumbel)
    return scored.argmax(dim=-1)


def topk_topp_filter(
    logits: torch.Tensor, topp: torch.Tensor, topk: torch.Tensor
) -> torch.Tensor:
    """Batched top-k / top-p filtering: mask entries outside the kept set
    to -inf, in place, and return logits. Semantics: top-p keeps the
    smallest prefix of the descending-sorted row whose softmax mass
    reaches p (the crossing token included); top-k keeps rank < k; both
    given -> intersection. Rows with topk==0 and topp>=1 are untouched."""
    B, V = logits.shape
    active = (topk > 0) | (topp < 1.0)
    if not bool(active.any()):
        return logits
    lf = logits.float()
    sorted_logits, sorted_idx = torch.sort(lf, descending=True, dim=-1)
    pos = torch.arange(V, device=logits.device).unsqueeze(0)  # [1, V]
    k = torch.where(topk > 0, topk, torch.full_like(topk, V)).unsqueeze(1)
    mask_sorted = pos >= k  # beyond top-k rank
    probs = torch.softmax(sorted_logits, dim=-1)
    cum = probs.cumsum(dim=-1)
    # keep through the first position where cumulative >= p
    crossed = (cum - probs) >= topp.unsqueeze(1)
    mask_sorted |= crossed
    mask_sorted &= active.unsqueeze(1)
    mask = torch.zeros_like(mask_sorted).scatter_(1, sorted_idx, mask_sorted)
    logits.masked_fill_(mask, float("-inf"))
    return logits
