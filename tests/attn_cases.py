"""Inputs, fp64 references and the acceptance bound for the attention-kernel
edge tests (test_attention_cases_cpu.py, test_attention_edges_gpu.py).

Why not randn alone: with randn Q/K/V the softmax is flat, one key of L
carries ~1/L of the weight, and a kernel that loses a key moves the output
by less than any tolerance that bf16 allows. The "needle" (decode, cached
prefill) and "diagonal"/"poison" (prefill) inputs give ONE chosen key a
score ~14 above the rest, so that key's V row essentially IS the output and
a kernel that omits it -- or admits one it must mask -- is wrong by O(1).

Everything unused in a paged cache is NaN (bf16 caches) or byte 0x7f with a
NaN scale (fp8 caches): free blocks, the tail of each sequence's last block,
and one spare block that every block-table entry past a sequence's last
used block points at. Entries never point out of range, so a kernel that
reads what it must not produces NaN, not a stray access.

The references gather through the block table and compute scores, softmax
and PV in fp64 from the exact bf16 (or exactly dequantised fp8) inputs.

Metric, used everywhere: per (row, head) max_d|got - ref64| / max_d|ref64|,
maximum over rows and heads.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Tuple

import torch

from llmapigateway_amd.ops import reference

D = 128
MARGIN = 14.0        # score lead of a needle / diagonal / poison key
Q_JITTER = 0.3       # per-head noise on the shared query direction
FP8_NAN_BYTE = 0x7F  # e4m3fn NaN

# ---------------------------------------------------------------------------
# Noise floors and acceptance bounds.
#
# F(case) = metric(bf16(reference evaluated in fp32), fp64 reference): what a
# correct kernel with fp32 arithmetic and a bf16 result cannot avoid. For
# fp8 caches the dequantised K/V are rounded to bf16 first, the precision in
# which the kernels consume them. The floors below are max F over every
# decode case (DECODE_CASES) and every prefill case (PREFILL_CASES) of this
# module, measured by test_attention_cases_cpu.py on the CPU, which
# recomputes them on every run and asserts that they still hold. Measured:
# decode 0.005819 (split-fp8-needle-2048; bf16 caches peak at 0.0039, flat
# inputs), prefill 0.004760 (cached-fp8-flat; 0.0039 without a cache). The
# fp8 cases are the worst because bf16(V) and the bf16 result round twice.
# The constants round those figures up.
#
# The bound is 4 x floor. The factor covers what the fp32 reference does
# not model: __expf, the summation order across waves and splits, in
# prefill the bf16 rounding of P before the PV MFMA (~2^-9 sum|p||v|), and
# in the v2 fp8 decode kernel the truncation of K*scale and V*scale to bf16.
# Nothing here is taken from a kernel's output.
# ---------------------------------------------------------------------------
DECODE_FLOOR = 0.0059
PREFILL_FLOOR = 0.0048
ATTN_BOUND_DECODE = 4.0 * DECODE_FLOOR
ATTN_BOUND_PREFILL = 4.0 * PREFILL_FLOOR
# every needle / diagonal / poison case: each mutation listed for the case
# moves the metric by at least this much
SENSITIVITY_MIN = 0.25


def metric(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max over (row, head) of max_d|got-ref| / max_d|ref|. A row whose
    reference is all zero (empty context) scores 0 if got is zero too, inf
    otherwise; NaN in got gives NaN, which fails every `<=`."""
    g = got.detach().double().cpu()
    r = ref64.double()
    num = (g - r).abs().amax(dim=-1)
    den = r.abs().amax(dim=-1)
    inf = torch.full_like(num, float("inf"))
    ratio = torch.where(den > 0, num / den.clamp_min(1e-300),
                        torch.where(num == 0, torch.zeros_like(num), inf))
    ratio = torch.where(torch.isnan(num), num, ratio)
    if torch.isnan(ratio).any():
        return float("nan")
    return float(ratio.max())


def _unit(x: torch.Tensor) -> torch.Tensor:
    return x / x.norm(dim=-1, keepdim=True)


def _randn(g: torch.Generator, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=g, dtype=torch.float32)


# ---------------------------------------------------------------------------
# paged cache with poisoned unused slots
# ---------------------------------------------------------------------------

@dataclass
class Paged:
    k_cache: torch.Tensor            # [NB, Hkv, BS, D] bf16 | uint8
    v_cache: torch.Tensor
    k_scale: Optional[torch.Tensor]  # [NB, Hkv, BS] fp32 (fp8 caches)
    v_scale: Optional[torch.Tensor]
    block_tables: torch.Tensor       # [B, width] int32
    lens: torch.Tensor               # [B] int32
    spare: int


def build_paged(ks: List[torch.Tensor], vs: List[torch.Tensor], BS: int,
                width: int, fp8: bool, g: torch.Generator) -> Paged:
    """ks[b], vs[b]: [L_b, Hkv, D] bf16. Shuffled block ids; 3 free blocks
    and 1 spare block stay poisoned, as does each last block's tail."""
    B = len(ks)
    Hkv = ks[0].shape[1]
    lens = [int(k.shape[0]) for k in ks]
    nblk = [(L + BS - 1) // BS for L in lens]
    width = max(width, max(nblk), 1)
    used = sum(nblk)
    NB = used + 4
    perm = torch.randperm(NB, generator=g).tolist()
    spare = perm[used]
    if fp8:
        k_cache = torch.full((NB, Hkv, BS, D), FP8_NAN_BYTE, dtype=torch.uint8)
        v_cache = torch.full((NB, Hkv, BS, D), FP8_NAN_BYTE, dtype=torch.uint8)
        k_scale = torch.full((NB, Hkv, BS), float("nan"), dtype=torch.float32)
        v_scale = torch.full((NB, Hkv, BS), float("nan"), dtype=torch.float32)
    else:
        k_cache = torch.full((NB, Hkv, BS, D), float("nan"), dtype=torch.bfloat16)
        v_cache = torch.full((NB, Hkv, BS, D), float("nan"), dtype=torch.bfloat16)
        k_scale = v_scale = None
    bt = torch.full((B, width), spare, dtype=torch.int32)
    nxt = 0
    for b in range(B):
        L = lens[b]
        if L == 0:
            continue
        ids = perm[nxt:nxt + nblk[b]]
        nxt += nblk[b]
        bt[b, :nblk[b]] = torch.tensor(ids, dtype=torch.int32)
        pos = torch.arange(L)
        blk = torch.tensor(ids)[pos // BS]
        off = pos % BS
        if fp8:
            kq, ksc = reference.fp8_quantize_rows(ks[b])
            vq, vsc = reference.fp8_quantize_rows(vs[b])
            k_cache[blk, :, off, :] = kq
            v_cache[blk, :, off, :] = vq
            k_scale[blk, :, off] = ksc
            v_scale[blk, :, off] = vsc
        else:
            k_cache[blk, :, off, :] = ks[b]
            v_cache[blk, :, off, :] = vs[b]
    return Paged(k_cache, v_cache, k_scale, v_scale, bt,
                 torch.tensor(lens, dtype=torch.int32), spare)


def gather_paged(p: Paged, b: int, L: int, dtype: torch.dtype,
                 kv_round_bf16: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """K, V [L, Hkv, D] of sequence b through its block-table row."""
    BS = p.k_cache.shape[2]
    nb = (L + BS - 1) // BS
    blocks = p.block_tables[b, :nb].long()
    if p.k_scale is not None:
        k = reference.fp8_dequantize_rows(p.k_cache[blocks], p.k_scale[blocks])
        v = reference.fp8_dequantize_rows(p.v_cache[blocks], p.v_scale[blocks])
        if kv_round_bf16:
            k, v = k.bfloat16(), v.bfloat16()
    else:
        k, v = p.k_cache[blocks], p.v_cache[blocks]
    Hkv = k.shape[1]
    k = k.permute(0, 2, 1, 3).reshape(-1, Hkv, D)[:L].to(dtype)
    v = v.permute(0, 2, 1, 3).reshape(-1, Hkv, D)[:L].to(dtype)
    return k, v


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

class DecodeSpec(NamedTuple):
    id: str
    lens: Tuple[int, ...]
    G: int = 4
    Hkv: int = 2
    BS: int = 16
    kind: str = "flat"           # "flat" | "needle"
    needle: object = None        # "first" | "last" | "blk_end" | "blk_next" | int
    fp8: bool = False
    scale: Optional[float] = None
    width: int = 0               # minimum block-table width (forces the split path)
    seed: int = 0


@dataclass
class DecodeCase:
    spec: DecodeSpec
    q: torch.Tensor              # [B, Hq, D] bf16
    paged: Paged
    scale: float
    needles: List[Optional[int]] = field(default_factory=list)  # per sequence

    @property
    def mutations(self) -> Tuple[str, ...]:
        """Mutations of the reference that this case must expose."""
        if self.spec.kind != "needle":
            return ()
        return ("drop", "short") if self.spec.needle == "last" else ("drop",)


def needle_pos(needle, L: int, BS: int) -> Optional[int]:
    if L <= 0:
        return None
    p = {"first": 0, "last": L - 1, "blk_end": BS - 1, "blk_next": BS}.get(needle, needle)
    return min(int(p), L - 1)


def build_decode(spec: DecodeSpec) -> DecodeCase:
    g = torch.Generator().manual_seed(1000 + spec.seed)
    B, Hkv, G = len(spec.lens), spec.Hkv, spec.G
    scale = spec.scale if spec.scale is not None else D ** -0.5
    q = _randn(g, B, Hkv, G, D)
    ks, vs, needles = [], [], []
    for b, L in enumerate(spec.lens):
        k = _randn(g, L, Hkv, D)
        v = _randn(g, L, Hkv, D)
        pos = needle_pos(spec.needle, L, spec.BS) if spec.kind == "needle" else None
        if spec.kind == "needle":
            # one query direction w per kv group; the needle key is the
            # multiple of w whose score is MARGIN for q = sqrt(D) w
            w = _unit(_randn(g, Hkv, D))
            q[b] = math.sqrt(D) * w[:, None, :] + Q_JITTER * q[b]
            if pos is not None:
                k[pos] = (MARGIN / (scale * math.sqrt(D))) * w
        needles.append(pos)
        ks.append(k.bfloat16())
        vs.append(v.bfloat16())
    paged = build_paged(ks, vs, spec.BS, spec.width, spec.fp8, g)
    return DecodeCase(spec, q.reshape(B, Hkv * G, D).bfloat16(), paged, scale, needles)


def decode_reference(case: DecodeCase, dtype: torch.dtype = torch.float64,
                     mutate: Optional[str] = None,
                     kv_round_bf16: bool = False) -> torch.Tensor:
    """[B, Hq, D] in `dtype`. mutate: "drop" removes each needle key,
    "short" uses L-1 keys -- the mistakes the needle cases must expose."""
    q = case.q.to(dtype)
    B, Hq, _ = q.shape
    G = case.spec.G
    out = torch.zeros(B, Hq, D, dtype=dtype)
    for b in range(B):
        L = int(case.paged.lens[b])
        if L == 0:
            continue
        k, v = gather_paged(case.paged, b, L, dtype, kv_round_bf16)
        keep = torch.ones(L, dtype=torch.bool)
        if mutate == "drop" and case.needles[b] is not None:
            keep[case.needles[b]] = False
        elif mutate == "short":
            keep[L - 1] = False
        k, v = k[keep], v[keep]
        if k.shape[0] == 0:
            continue
        k = k.repeat_interleave(G, dim=1)
        v = v.repeat_interleave(G, dim=1)
        s = torch.einsum("hd,khd->hk", q[b], k) * case.scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hk,khd->hd", p, v)
    return out


_EDGE_LENS = (1, 63, 64, 65, 255, 256, 257)
_NEEDLES = ("first", "last", "blk_end", "blk_next", 63, 64, 255, 256)
_SPLIT_LENS = (2047, 2048, 2049, 4096, 4097)


def _decode_cases() -> List[DecodeSpec]:
    cs: List[DecodeSpec] = []
    seed = 0

    def add(id, lens, **kw):
        nonlocal seed
        seed += 1
        cs.append(DecodeSpec(id=id, lens=tuple(lens), seed=seed, **kw))

    # ragged batch of every chunk/stride edge, both block sizes
    for BS in (16, 64):
        add(f"ragged-bs{BS}-flat", _EDGE_LENS, BS=BS)
        for n in _NEEDLES:
            add(f"ragged-bs{BS}-needle-{n}", _EDGE_LENS, BS=BS, kind="needle", needle=n)
    # each edge length on its own
    for L in _EDGE_LENS:
        add(f"len{L}-needle-last", (L, L), kind="needle", needle="last")
    # every GQA group size (v2 gives wave w heads w, w+4)
    for G in range(1, 9):
        add(f"G{G}-needle-last", (65, 257), G=G, kind="needle", needle="last")
        add(f"G{G}-flat", (65, 257), G=G)
    # fp8 cache, non-split
    add("ragged-fp8-flat", _EDGE_LENS, fp8=True)
    add("ragged-fp8-needle-last", _EDGE_LENS, fp8=True, kind="needle", needle="last")
    # non-default scale
    add("ragged-scale0.05-needle-last", _EDGE_LENS, kind="needle", needle="last", scale=0.05)
    add("ragged-scale0.05-flat", _EDGE_LENS, scale=0.05)
    # split path: block table spans > 2048 positions and B*Hkv < 192
    for fp8 in (False, True):
        t = "fp8" if fp8 else "bf16"
        add(f"split-{t}-flat", _SPLIT_LENS, Hkv=1, fp8=fp8)
        for n in ("first", "last", 2047, 2048):
            add(f"split-{t}-needle-{n}", _SPLIT_LENS, Hkv=1, fp8=fp8,
                kind="needle", needle=n)
        # idle splits of the short row publish empty partials
        add(f"split-{t}-mix-flat", (5, 5000), Hkv=1, fp8=fp8)
        add(f"split-{t}-mix-needle-last", (5, 5000), Hkv=1, fp8=fp8,
            kind="needle", needle="last")
    # 1025 block-table entries: global block-table fallback + split-count cap
    add("long16400-flat", (16400,), Hkv=1)
    for n in (0, 16383, 16384, 16399):
        add(f"long16400-needle-{n}", (16400,), Hkv=1, kind="needle", needle=n)
    # empty rows among live ones, non-split and split
    add("empty-row-nonsplit", (65, 0, 257), kind="needle", needle="last")
    add("empty-row-split", (0, 2049, 5, 0), Hkv=1, kind="needle", needle="last", width=129)
    # direct-binding cases (explicit version / nsplit): L straddles split edges
    for G in (4, 7):
        for fp8 in (False, True):
            t = "fp8" if fp8 else "bf16"
            add(f"binding-G{G}-{t}", (2047, 2049, 4100, 70), G=G, Hkv=1, fp8=fp8,
                kind="needle", needle="last")
    return cs


DECODE_CASES: List[DecodeSpec] = _decode_cases()
DECODE_BY_ID = {c.id: c for c in DECODE_CASES}

# Flat cases exercise accumulation over many comparable keys. They canNOT
# see (the metric moves by less than the bound at L >~ 30): a dropped key,
# a context length off by one, a missed block-table entry, a lost chunk at a
# split edge; in prefill a mask that leaks or excludes one position. Those
# are the needle / diagonal / poison cases' job. No claim beyond this.
FLAT_BLIND_TO = ("drop", "short", "leak1", "boundary", "nodiag")


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------

class PrefillSpec(NamedTuple):
    id: str
    lens: Tuple[int, ...]
    cached: Optional[Tuple[int, ...]] = None
    G: int = 2
    Hkv: int = 2
    BS: int = 16
    kind: str = "flat"           # "flat" | "diag" | "poison" | "needle" (cached)
    needle: object = None        # "first" | "last" (cached position)
    fp8: bool = False
    scale: Optional[float] = None
    seed: int = 0


@dataclass
class PrefillCase:
    spec: PrefillSpec
    q: torch.Tensor              # [T, Hq, D] bf16
    k: torch.Tensor              # [T, Hkv, D] bf16
    v: torch.Tensor
    cu_seqlens: torch.Tensor     # [B+1] int32
    scale: float
    paged: Optional[Paged] = None
    needles: List[Optional[int]] = field(default_factory=list)

    @property
    def mutations(self) -> Tuple[str, ...]:
        return {"diag": ("nodiag",), "poison": ("leak1", "boundary"),
                "needle": ("drop",)}.get(self.spec.kind, ())


def build_prefill(spec: PrefillSpec) -> PrefillCase:
    g = torch.Generator().manual_seed(5000 + spec.seed)
    Hkv, G = spec.Hkv, spec.G
    T = sum(spec.lens)
    scale = spec.scale if spec.scale is not None else D ** -0.5
    b_coef = MARGIN / (scale * math.sqrt(D))
    q = _randn(g, T, Hkv, G, D)
    k = _randn(g, T, Hkv, D)
    v = _randn(g, T, Hkv, D)
    if spec.kind in ("diag", "poison"):
        # u[t + 1] is token t's direction, u[0] stands in for "u_{-1}"
        u = _unit(_randn(g, T + 1, Hkv, D))
        q = math.sqrt(D) * u[1:, :, None, :] + Q_JITTER * q
        k = b_coef * (u[1:] if spec.kind == "diag" else u[:-1])
    cu = [0]
    for L in spec.lens:
        cu.append(cu[-1] + L)
    paged, needles = None, []
    if spec.cached is not None:
        ks, vs = [], []
        for i, nc in enumerate(spec.cached):
            kc = _randn(g, nc, Hkv, D)
            vc = _randn(g, nc, Hkv, D)
            pos = None
            if spec.kind == "needle":
                w = _unit(_randn(g, Hkv, D))
                s, e = cu[i], cu[i + 1]
                q[s:e] = math.sqrt(D) * w[None, :, None, :] + Q_JITTER * q[s:e]
                pos = needle_pos(spec.needle, nc, spec.BS)
                if pos is not None:
                    kc[pos] = b_coef * w
            needles.append(pos)
            ks.append(kc.bfloat16())
            vs.append(vc.bfloat16())
        paged = build_paged(ks, vs, spec.BS, 0, spec.fp8, g)
    return PrefillCase(spec, q.reshape(T, Hkv * G, D).bfloat16(), k.bfloat16(),
                       v.bfloat16(), torch.tensor(cu, dtype=torch.int32), scale,
                       paged, needles)


def prefill_reference(case: PrefillCase, dtype: torch.dtype = torch.float64,
                      mutate: Optional[str] = None,
                      kv_round_bf16: bool = False) -> torch.Tensor:
    """[T, Hq, D] in `dtype`; causal within each sequence's fresh tokens,
    every fresh row sees the whole cached prefix. mutate:
      "nodiag"   key >= qrow masked (row 0 keeps its only key);
      "leak1"    key > qrow + 1 masked instead of key > qrow;
      "boundary" the last row of a sequence also sees the first token of
                 the next sequence;
      "drop"     the needle key of the cached prefix is removed."""
    q, k, v = case.q.to(dtype), case.k.to(dtype), case.v.to(dtype)
    T, Hq, _ = q.shape
    G = case.spec.G
    cu = case.cu_seqlens.tolist()
    out = torch.zeros(T, Hq, D, dtype=dtype)
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        L = e - s
        if L == 0:
            continue
        ext = 1 if (mutate == "boundary" and e < T) else 0
        ki, vi = k[s:e + ext], v[s:e + ext]
        row = torch.arange(L)[:, None]
        col = torch.arange(L + ext)[None, :]
        if mutate == "nodiag":
            allowed = (col < row) | ((row == 0) & (col == 0))
        elif mutate == "leak1":
            allowed = col <= row + 1
        elif mutate == "boundary":
            allowed = (col <= row) | ((row == L - 1) & (col == L))
        else:
            allowed = col <= row
        nc = int(case.paged.lens[i]) if case.paged is not None else 0
        if nc > 0:
            kc, vc = gather_paged(case.paged, i, nc, dtype, kv_round_bf16)
            keep = torch.ones(nc, dtype=torch.bool)
            if mutate == "drop" and case.needles[i] is not None:
                keep[case.needles[i]] = False
            kc, vc = kc[keep], vc[keep]
            ki, vi = torch.cat([kc, ki]), torch.cat([vc, vi])
            allowed = torch.cat(
                [torch.ones(L, kc.shape[0], dtype=torch.bool), allowed], dim=1)
        ki = ki.repeat_interleave(G, dim=1)
        vi = vi.repeat_interleave(G, dim=1)
        sc = torch.einsum("qhd,khd->hqk", q[s:e], ki) * case.scale
        sc = sc.masked_fill(~allowed[None], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[s:e] = torch.einsum("hqk,khd->qhd", p, vi)
    return out


_PF_LENS = (1, 63, 64, 65, 128, 129)


def _prefill_cases() -> List[PrefillSpec]:
    cs: List[PrefillSpec] = []
    seed = 0

    def add(id, lens, **kw):
        nonlocal seed
        seed += 1
        cs.append(PrefillSpec(id=id, lens=tuple(lens), seed=seed, **kw))

    for kind in ("diag", "poison", "flat"):
        add(f"varlen-{kind}", _PF_LENS, kind=kind)
    add("varlen-diag-scale0.05", _PF_LENS, kind="diag", scale=0.05)
    add("varlen-poison-scale0.05", _PF_LENS, kind="poison", scale=0.05)
    # cached context: three sequences, one block-table row each
    for fp8 in (False, True):
        t = "fp8" if fp8 else "bf16"
        for n in ("first", "last"):
            add(f"cached-{t}-needle-{n}", (65, 33, 1), cached=(0, 17, 64),
                kind="needle", needle=n, fp8=fp8)
        add(f"cached-{t}-flat", (65, 33, 1), cached=(0, 17, 64), fp8=fp8)
    return cs


PREFILL_CASES: List[PrefillSpec] = _prefill_cases()
PREFILL_BY_ID = {c.id: c for c in PREFILL_CASES}


# ---------------------------------------------------------------------------
# built cases and fp64 references, computed once per process and shared
# ---------------------------------------------------------------------------

_built: dict = {}


def decode_case(id: str) -> Tuple[DecodeCase, torch.Tensor]:
    key = ("d", id)
    if key not in _built:
        case = build_decode(DECODE_BY_ID[id])
        _built[key] = (case, decode_reference(case))
    return _built[key]


def prefill_case(id: str) -> Tuple[PrefillCase, torch.Tensor]:
    key = ("p", id)
    if key not in _built:
        case = build_prefill(PREFILL_BY_ID[id])
        _built[key] = (case, prefill_reference(case))
    return _built[key]
