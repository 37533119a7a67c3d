"""Inputs and fp64 references for the sliding-window attention tests
(test_attention_window_cases_cpu.py, test_attention_window_gpu.py), built on
the helpers of attn_cases.py: the same needle construction (one key with a
score lead of MARGIN), the same poisoned paged cache, the same metric, floors
and bounds.

Window W: the query at absolute position p attends to keys p - W < j <= p.
A window goes wrong at its edge, so the chosen key sits there:

  needle-edge  the leading key is the OLDEST key inside the window
               (decode: L - W; prefill: row - W + 1). A window one key too
               short ("win_short", W - 1) loses it.
  poison-out   the leading key is the NEWEST key outside the window
               (decode: L - W - 1; prefill: row - W). A window one key too
               long ("win_leak", W + 1) admits it.

A released block: every block-table entry of a block that lies wholly below
the window (decode: below L - W; cached prefill: below the first fresh row's
window) points at the NaN spare block, the way the engine leaves a block it
has given back. A kernel that reads such an entry produces NaN. The
references gather through the table as it was before the release.

Noise floors: see WIN_DECODE_FLOOR / WIN_PREFILL_FLOOR below.
"""

from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Tuple

import torch

from tests import attn_cases as ac
from tests.attn_cases import D, MARGIN, Q_JITTER, Paged, build_paged, gather_paged

MUTATIONS = {"win_leak": +1, "win_short": -1}

# ---------------------------------------------------------------------------
# Noise floors of the windowed cases: F(case) = metric(bf16(reference in
# fp32), fp64 reference), as attn_cases.py defines it, measured on the CPU by
# test_attention_window_cases_cpu.py, which recomputes them on every run. A
# window only removes keys, so the floors of attn_cases.py were expected to
# hold; they do for bf16 caches (worst 0.003854) but not for fp8 caches,
# where a short window leaves few keys to average the double rounding
# (bf16(V), then the bf16 result) away. Measured: decode 0.007015
# (ragged-fp8-bs64-w63-poison-out), prefill 0.006337
# (cached300-fp8-w32-poison-out). The constants round those up; the bounds
# are 4 x floor as in attn_cases.py. Nothing here is taken from a kernel.
# ---------------------------------------------------------------------------
WIN_DECODE_FLOOR = 0.0071
WIN_PREFILL_FLOOR = 0.0064
WIN_BOUND_DECODE = 4.0 * WIN_DECODE_FLOOR
WIN_BOUND_PREFILL = 4.0 * WIN_PREFILL_FLOOR


def _release(paged: Paged, first_needed: List[int]) -> Tuple[Paged, torch.Tensor]:
    """Point the entries of blocks wholly below first_needed[b] at the spare
    block. Returns (paged, the table before the release)."""
    BS = paged.k_cache.shape[2]
    full = paged.block_tables.clone()
    for b, lo in enumerate(first_needed):
        paged.block_tables[b, : max(lo, 0) // BS] = paged.spare
    return paged, full


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

class WinDecodeSpec(NamedTuple):
    id: str
    lens: Tuple[int, ...]
    W: int
    kind: str = "flat"   # "flat" | "needle-edge" | "poison-out" | "needle-last"
    G: int = 4
    Hkv: int = 2
    BS: int = 16
    fp8: bool = False
    seed: int = 0


@dataclass
class WinDecodeCase:
    spec: WinDecodeSpec
    q: torch.Tensor               # [B, Hq, D] bf16
    paged: Paged                  # block tables with the released entries
    full_tables: torch.Tensor     # ... and before the release
    scale: float
    needles: List[Optional[int]] = field(default_factory=list)

    @property
    def mutation(self) -> Optional[str]:
        return {"needle-edge": "win_short", "poison-out": "win_leak"}.get(self.spec.kind)


def _decode_needle(kind: str, L: int, W: int) -> Optional[int]:
    if kind == "needle-edge":
        return max(L - W, 0)
    if kind == "poison-out":
        return L - W - 1 if L - W - 1 >= 0 else None
    if kind == "needle-last":
        return L - 1
    return None


def build_win_decode(spec: WinDecodeSpec) -> WinDecodeCase:
    g = torch.Generator().manual_seed(21000 + spec.seed)
    B, Hkv, G = len(spec.lens), spec.Hkv, spec.G
    scale = D ** -0.5
    q = ac._randn(g, B, Hkv, G, D)
    ks, vs, needles = [], [], []
    for b, L in enumerate(spec.lens):
        k = ac._randn(g, L, Hkv, D)
        v = ac._randn(g, L, Hkv, D)
        pos = _decode_needle(spec.kind, L, spec.W)
        if spec.kind != "flat":
            w = ac._unit(ac._randn(g, Hkv, D))
            q[b] = math.sqrt(D) * w[:, None, :] + Q_JITTER * q[b]
            if pos is not None:
                k[pos] = (MARGIN / (scale * math.sqrt(D))) * w
        needles.append(pos)
        ks.append(k.bfloat16())
        vs.append(v.bfloat16())
    paged = build_paged(ks, vs, spec.BS, 0, spec.fp8, g)
    paged, full = _release(paged, [L - spec.W for L in spec.lens])
    return WinDecodeCase(spec, q.reshape(B, Hkv * G, D).bfloat16(), paged, full,
                         scale, needles)


def win_decode_reference(case: WinDecodeCase, dtype: torch.dtype = torch.float64,
                         mutate: Optional[str] = None,
                         kv_round_bf16: bool = False,
                         window: Optional[int] = None) -> torch.Tensor:
    """[B, Hq, D] in `dtype` over the keys [max(0, L - W), L). mutate:
    "win_leak" uses W + 1, "win_short" W - 1 (no key at all for W = 1: the
    row is zeros). window overrides the case's W."""
    W = (case.spec.W if window is None else window) + MUTATIONS.get(mutate, 0)
    q = case.q.to(dtype)
    B, Hq, _ = q.shape
    G = case.spec.G
    full = dataclasses.replace(case.paged, block_tables=case.full_tables)
    out = torch.zeros(B, Hq, D, dtype=dtype)
    for b in range(B):
        L = int(case.paged.lens[b])
        lo = max(L - W, 0)
        if L == 0 or lo >= L:
            continue
        k, v = gather_paged(full, b, L, dtype, kv_round_bf16)
        k = k[lo:].repeat_interleave(G, dim=1)
        v = v[lo:].repeat_interleave(G, dim=1)
        s = torch.einsum("hd,khd->hk", q[b], k) * case.scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hk,khd->hd", p, v)
    return out


_WINDOWS = (1, 16, 63, 64, 65, 100)
_KINDS = ("needle-edge", "poison-out", "needle-last", "flat")
_SPLIT_LENS = (2049, 4097, 5000)


def _ragged_lens(W: int) -> Tuple[int, ...]:
    lens = []
    for L in (1, W - 1, W, W + 1, 63, 64, 65, 255, 256, 257):
        if L > 0 and L not in lens:
            lens.append(L)
    return tuple(lens)


def _decode_cases() -> List[WinDecodeSpec]:
    cs: List[WinDecodeSpec] = []

    def add(id, lens, W, **kw):
        cs.append(WinDecodeSpec(id=id, lens=tuple(lens), W=W, seed=len(cs) + 1, **kw))

    # every window against every chunk / stride / window edge, both block
    # sizes, both cache types
    for fp8 in (False, True):
        t = "fp8" if fp8 else "bf16"
        for BS in (16, 64):
            for W in _WINDOWS:
                for kind in _KINDS:
                    add(f"ragged-{t}-bs{BS}-w{W}-{kind}", _ragged_lens(W), W,
                        kind=kind, BS=BS, fp8=fp8)
    # G = 7: v2 gives wave w heads w and w + 4 (G = 4 is the default above)
    for kind in _KINDS:
        add(f"G7-w65-{kind}", _ragged_lens(65), 65, kind=kind, G=7)
    # split path (block table spans > 2048 positions, B * Hkv < 192): W = 64
    # leaves every split but the window's below it, 2048 puts the window edge
    # inside a split of the windowless geometry, 2100 straddles a split edge
    for fp8 in (False, True):
        t = "fp8" if fp8 else "bf16"
        for W in (64, 2048, 2100):
            for kind in ("needle-edge", "poison-out", "flat"):
                add(f"split-{t}-w{W}-{kind}", _SPLIT_LENS, W, kind=kind, Hkv=1, fp8=fp8)
        for kind in ("needle-edge", "poison-out"):
            add(f"split-{t}-mix-w64-{kind}", (5, 5000), 64, kind=kind, Hkv=1, fp8=fp8)
    # 1025 block-table entries: the window's first entry is 1018 and its
    # last 1024, either side of the 1024-entry LDS table of a windowless call
    for kind in ("needle-edge", "poison-out"):
        add(f"long16400-w100-{kind}", (16400,), 100, kind=kind, Hkv=1)
    # ... and a window of 1025 entries itself: the global fallback
    add("long16400-w16390-needle-edge", (16400,), 16390, kind="needle-edge", Hkv=1)
    add("long16400-w16390-needle-last", (16400,), 16390, kind="needle-last", Hkv=1)
    return cs


WIN_DECODE_CASES: List[WinDecodeSpec] = _decode_cases()
WIN_DECODE_BY_ID = {c.id: c for c in WIN_DECODE_CASES}


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------

class WinPrefillSpec(NamedTuple):
    id: str
    lens: Tuple[int, ...]
    W: int
    kind: str = "flat"   # "flat" | "diag" | "needle-edge" | "poison-out"
    cached: Optional[Tuple[int, ...]] = None
    G: int = 2
    Hkv: int = 2
    BS: int = 16
    fp8: bool = False
    seed: int = 0


@dataclass
class WinPrefillCase:
    spec: WinPrefillSpec
    q: torch.Tensor               # [T, Hq, D] bf16
    k: torch.Tensor               # [T, Hkv, D] bf16
    v: torch.Tensor
    cu_seqlens: torch.Tensor      # [B+1] int32
    scale: float
    paged: Optional[Paged] = None
    full_tables: Optional[torch.Tensor] = None

    @property
    def mutation(self) -> Optional[str]:
        return {"needle-edge": "win_short", "poison-out": "win_leak"}.get(self.spec.kind)


def build_win_prefill(spec: WinPrefillSpec) -> WinPrefillCase:
    """Positions are absolute per sequence: nc cached keys, then L fresh
    tokens. Fresh row r (absolute nc + r) has its own query direction u_r;
    the key at absolute position nc + r - shift is b * u_r, where shift is 0
    (diag), W - 1 (needle-edge) or W (poison-out), wherever that position
    exists -- in the cached prefix, across the seam or among the fresh keys."""
    g = torch.Generator().manual_seed(25000 + spec.seed)
    Hkv, G, W = spec.Hkv, spec.G, spec.W
    scale = D ** -0.5
    b_coef = MARGIN / (scale * math.sqrt(D))
    shift = {"diag": 0, "needle-edge": W - 1, "poison-out": W}.get(spec.kind)
    cached = spec.cached or (0,) * len(spec.lens)
    qs, kf, vf, kc, vc = [], [], [], [], []
    for L, nc in zip(spec.lens, cached):
        q = ac._randn(g, L, Hkv, G, D)
        k = ac._randn(g, nc + L, Hkv, D)
        v = ac._randn(g, nc + L, Hkv, D)
        if shift is not None:
            u = ac._unit(ac._randn(g, L, Hkv, D))
            q = math.sqrt(D) * u[:, :, None, :] + Q_JITTER * q
            for r in range(L):
                a = nc + r - shift
                if a >= 0:
                    k[a] = b_coef * u[r]
        qs.append(q)
        kc.append(k[:nc].bfloat16())
        vc.append(v[:nc].bfloat16())
        kf.append(k[nc:])
        vf.append(v[nc:])
    cu = [0]
    for L in spec.lens:
        cu.append(cu[-1] + L)
    T = cu[-1]
    paged = full = None
    if spec.cached is not None:
        paged = build_paged(kc, vc, spec.BS, 0, spec.fp8, g)
        paged, full = _release(paged, [nc - W + 1 for nc in cached])
    return WinPrefillCase(
        spec, torch.cat(qs).reshape(T, Hkv * G, D).bfloat16(),
        torch.cat(kf).bfloat16(), torch.cat(vf).bfloat16(),
        torch.tensor(cu, dtype=torch.int32), scale, paged, full)


def win_prefill_reference(case: WinPrefillCase, dtype: torch.dtype = torch.float64,
                          mutate: Optional[str] = None,
                          kv_round_bf16: bool = False,
                          window: Optional[int] = None) -> torch.Tensor:
    """[T, Hq, D] in `dtype`: the row at absolute position p attends to the
    keys p - W < j <= p of its own sequence, cached prefix and fresh tokens
    alike. mutate / window as in win_decode_reference."""
    W = (case.spec.W if window is None else window) + MUTATIONS.get(mutate, 0)
    q, k, v = case.q.to(dtype), case.k.to(dtype), case.v.to(dtype)
    T, Hq, _ = q.shape
    G = case.spec.G
    cu = case.cu_seqlens.tolist()
    full = None
    if case.paged is not None:
        full = dataclasses.replace(case.paged, block_tables=case.full_tables)
    out = torch.zeros(T, Hq, D, dtype=dtype)
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        L = e - s
        nc = int(case.paged.lens[i]) if case.paged is not None else 0
        ki, vi = k[s:e], v[s:e]
        if nc > 0:
            kc, vc = gather_paged(full, i, nc, dtype, kv_round_bf16)
            ki, vi = torch.cat([kc, ki]), torch.cat([vc, vi])
        row = torch.arange(L)[:, None] + nc
        col = torch.arange(nc + L)[None, :]
        allowed = (col <= row) & (col > row - W)
        ki = ki.repeat_interleave(G, dim=1)
        vi = vi.repeat_interleave(G, dim=1)
        sc = torch.einsum("qhd,khd->hqk", q[s:e], ki) * case.scale
        sc = sc.masked_fill(~allowed[None], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        p = torch.where(allowed.any(dim=1)[None, :, None], p, torch.zeros_like(p))
        out[s:e] = torch.einsum("hqk,khd->qhd", p, vi)
    return out


_PF_LENS = (1, 63, 64, 65, 128, 129, 200)


def _prefill_cases() -> List[WinPrefillSpec]:
    cs: List[WinPrefillSpec] = []

    def add(id, lens, W, **kw):
        cs.append(WinPrefillSpec(id=id, lens=tuple(lens), W=W, seed=len(cs) + 1, **kw))

    # W = 1: the output is the token's own V row
    add("varlen-w1-diag", _PF_LENS, 1, kind="diag")
    for W in (1, 16, 64, 65, 100):
        for kind in ("needle-edge", "poison-out", "flat"):
            add(f"varlen-w{W}-{kind}", _PF_LENS, W, kind=kind)
    # cached context: the chosen keys lie in the cached prefix and across the
    # cached / fresh seam; (300, 300) releases 16 blocks per sequence
    for fp8 in (False, True):
        t = "fp8" if fp8 else "bf16"
        for kind in ("needle-edge", "poison-out", "flat"):
            add(f"cached-{t}-w32-{kind}", (65, 33, 1), 32, kind=kind,
                cached=(0, 17, 64), fp8=fp8)
            add(f"cached300-{t}-w32-{kind}", (5, 40), 32, kind=kind,
                cached=(300, 300), fp8=fp8)
    return cs


WIN_PREFILL_CASES: List[WinPrefillSpec] = _prefill_cases()
WIN_PREFILL_BY_ID = {c.id: c for c in WIN_PREFILL_CASES}


# ---------------------------------------------------------------------------
# built cases and fp64 references, computed once per process and shared
# ---------------------------------------------------------------------------

_built: dict = {}


def win_decode_case(id: str) -> Tuple[WinDecodeCase, torch.Tensor]:
    key = ("d", id)
    if key not in _built:
        case = build_win_decode(WIN_DECODE_BY_ID[id])
        _built[key] = (case, win_decode_reference(case))
    return _built[key]


def win_prefill_case(id: str) -> Tuple[WinPrefillCase, torch.Tensor]:
    key = ("p", id)
    if key not in _built:
        case = build_win_prefill(WIN_PREFILL_BY_ID[id])
        _built[key] = (case, win_prefill_reference(case))
    return _built[key]
