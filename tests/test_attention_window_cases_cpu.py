"""CPU validation of the sliding-window attention inputs
(attn_window_cases.py) and of the windowed CPU reference of ops: every
needle-edge case moves under a window one key too short, every poison-out
case under a window one key too long, every case stays within the noise
floors of attn_window_cases.py (recomputed here on every run), and ops.reference
with a window is a dense masked softmax over the window's keys that reads no
released block.

Run with -s to see the per-case figures."""

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.ops import reference
from tests import attn_cases as ac
from tests import attn_window_cases as wc


# ---------- sensitivity ----------

@pytest.mark.parametrize(
    "id", [c.id for c in wc.WIN_DECODE_CASES if c.kind in ("needle-edge", "poison-out")])
def test_decode_window_sensitivity(id):
    case, ref64 = wc.win_decode_case(id)
    moved = ac.metric(wc.win_decode_reference(case, mutate=case.mutation), ref64)
    print(f"sensitivity {id} {case.mutation}: {moved:.3f}")
    assert moved >= ac.SENSITIVITY_MIN, (id, case.mutation, moved)


@pytest.mark.parametrize(
    "id", [c.id for c in wc.WIN_PREFILL_CASES if c.kind in ("needle-edge", "poison-out")])
def test_prefill_window_sensitivity(id):
    case, ref64 = wc.win_prefill_case(id)
    moved = ac.metric(wc.win_prefill_reference(case, mutate=case.mutation), ref64)
    print(f"sensitivity {id} {case.mutation}: {moved:.3f}")
    assert moved >= ac.SENSITIVITY_MIN, (id, case.mutation, moved)


def test_diag_w1_is_the_own_v_row():
    case, ref64 = wc.win_prefill_case("varlen-w1-diag")
    G = case.spec.G
    own = case.v.double().repeat_interleave(G, dim=1)
    assert torch.equal(ref64, own)


# ---------- noise floors ----------

def test_decode_window_floor():
    """F(case) = metric(bf16(fp32 reference), fp64 reference) of every
    windowed case is within WIN_DECODE_FLOOR, and the constant is not
    inflated past the measurement."""
    worst, worst_id = 0.0, None
    for c in wc.WIN_DECODE_CASES:
        case, ref64 = wc.win_decode_case(c.id)
        lo = wc.win_decode_reference(case, torch.float32, kv_round_bf16=True).bfloat16()
        f = ac.metric(lo, ref64)
        print(f"floor decode {c.id}: {f:.6f}")
        if f > worst:
            worst, worst_id = f, c.id
        assert f <= wc.WIN_DECODE_FLOOR, (c.id, f)
    print(f"max F(window decode) = {worst:.6f} at {worst_id}")
    assert wc.WIN_DECODE_FLOOR <= 1.25 * worst
    assert wc.WIN_BOUND_DECODE == 4.0 * wc.WIN_DECODE_FLOOR


def test_prefill_window_floor():
    worst, worst_id = 0.0, None
    for c in wc.WIN_PREFILL_CASES:
        case, ref64 = wc.win_prefill_case(c.id)
        lo = wc.win_prefill_reference(case, torch.float32, kv_round_bf16=True).bfloat16()
        f = ac.metric(lo, ref64)
        print(f"floor prefill {c.id}: {f:.6f}")
        if f > worst:
            worst, worst_id = f, c.id
        assert f <= wc.WIN_PREFILL_FLOOR, (c.id, f)
    print(f"max F(window prefill) = {worst:.6f} at {worst_id}")
    assert wc.WIN_PREFILL_FLOOR <= 1.25 * worst
    assert wc.WIN_BOUND_PREFILL == 4.0 * wc.WIN_PREFILL_FLOOR


# ---------- the windowed CPU reference of ops ----------

def _ops_decode(case, window):
    p = case.paged
    return ops.attention_decode(
        case.q, p.k_cache, p.v_cache, p.block_tables, p.lens, case.scale,
        k_scale=p.k_scale, v_scale=p.v_scale, window=window)


def _ops_prefill(case, window, tables=None):
    p = case.paged
    kw = {}
    if p is not None:
        kw = dict(k_cache=p.k_cache, v_cache=p.v_cache,
                  block_tables=p.block_tables if tables is None else tables,
                  cached_lens=p.lens, k_scale=p.k_scale, v_scale=p.v_scale)
    return ops.attention_prefill(
        case.q, case.k, case.v, case.cu_seqlens, max(case.spec.lens), case.scale,
        window=window, **kw)


@pytest.mark.parametrize("id", [c.id for c in wc.WIN_DECODE_CASES
                                if not c.id.startswith("long")])
def test_ops_cpu_decode_window(id):
    """Reads through the released table: NaN would show a read below the
    window."""
    case, ref64 = wc.win_decode_case(id)
    got = _ops_decode(case, case.spec.W)
    assert not torch.isnan(got).any()
    assert ac.metric(got, ref64) <= wc.WIN_DECODE_FLOOR


@pytest.mark.parametrize("id", [c.id for c in wc.WIN_PREFILL_CASES])
def test_ops_cpu_prefill_window(id):
    case, ref64 = wc.win_prefill_case(id)
    got = _ops_prefill(case, case.spec.W)
    assert not torch.isnan(got).any()
    assert ac.metric(got, ref64) <= wc.WIN_PREFILL_FLOOR


@pytest.mark.parametrize("id", ["ragged-bs16-needle-last", "ragged-fp8-flat",
                                "G7-needle-last"])
def test_ops_cpu_decode_wide_window_is_exact(id):
    """window >= L: bit-equal to the call without a window."""
    case, _ = ac.decode_case(id)
    p = case.paged
    args = (case.q, p.k_cache, p.v_cache, p.block_tables, p.lens, case.scale)
    kw = dict(k_scale=p.k_scale, v_scale=p.v_scale)
    base = ops.attention_decode(*args, **kw)
    for W in (max(case.spec.lens), max(case.spec.lens) + 1, 1 << 20):
        assert torch.equal(ops.attention_decode(*args, window=W, **kw), base)
    for W in (0, None):
        assert torch.equal(ops.attention_decode(*args, window=W, **kw), base)
    assert torch.equal(reference.attention_decode(*args, **kw), base)


@pytest.mark.parametrize("id", ["varlen-poison", "cached-bf16-needle-first",
                                "cached-fp8-flat"])
def test_ops_cpu_prefill_wide_window_is_exact(id):
    case, _ = ac.prefill_case(id)
    p = case.paged
    kw = {}
    total = max(case.spec.lens)
    if p is not None:
        kw = dict(k_cache=p.k_cache, v_cache=p.v_cache, block_tables=p.block_tables,
                  cached_lens=p.lens, k_scale=p.k_scale, v_scale=p.v_scale)
        total += int(p.lens.max())
    args = (case.q, case.k, case.v, case.cu_seqlens, max(case.spec.lens), case.scale)
    base = ops.attention_prefill(*args, **kw)
    for W in (total, total + 1, 1 << 20, 0, None):
        assert torch.equal(ops.attention_prefill(*args, window=W, **kw), base)


def test_ops_cpu_window_rejects_bad_arguments():
    case, _ = ac.decode_case("ragged-bs16-flat")
    with pytest.raises(ValueError):
        _ops_decode(case, -1)
    pf, _ = ac.prefill_case("varlen-flat")
    with pytest.raises(ValueError):
        ops.attention_prefill(pf.q, pf.k, pf.v, pf.cu_seqlens, 129, pf.scale,
                              causal=False, window=4)


def test_reference_decode_is_a_dense_masked_softmax():
    """Written out: scores over ALL keys, -inf outside (L - W, L]."""
    g = torch.Generator().manual_seed(5)
    B, Hkv, G, BS, L, W = 1, 2, 2, 16, 70, 23
    q = torch.randn(B, Hkv * G, ac.D, generator=g)
    k = torch.randn(L, Hkv, ac.D, generator=g)
    v = torch.randn(L, Hkv, ac.D, generator=g)
    nb = -(-L // BS)
    kc = torch.zeros(nb, Hkv, BS, ac.D)
    vc = torch.zeros(nb, Hkv, BS, ac.D)
    pos = torch.arange(L)
    kc[pos // BS, :, pos % BS] = k
    vc[pos // BS, :, pos % BS] = v
    bt = torch.arange(nb, dtype=torch.int32)[None]
    got = reference.attention_decode(
        q, kc, vc, bt, torch.tensor([L], dtype=torch.int32), window=W)
    s = torch.einsum("hd,khd->hk", q[0], k.repeat_interleave(G, dim=1)) * ac.D ** -0.5
    j = torch.arange(L)
    s = s.masked_fill(~((j > L - 1 - W) & (j <= L - 1))[None], float("-inf"))
    want = torch.einsum("hk,khd->hd", torch.softmax(s, -1), v.repeat_interleave(G, dim=1))
    assert torch.allclose(got[0], want, atol=1e-5, rtol=1e-5)


def test_reference_prefill_is_a_dense_masked_softmax():
    g = torch.Generator().manual_seed(6)
    Hkv, G, L, W = 2, 2, 50, 9
    q = torch.randn(L, Hkv * G, ac.D, generator=g)
    k = torch.randn(L, Hkv, ac.D, generator=g)
    v = torch.randn(L, Hkv, ac.D, generator=g)
    cu = torch.tensor([0, L], dtype=torch.int32)
    got = reference.attention_prefill(q, k, v, cu, window=W)
    s = torch.einsum("qhd,khd->hqk", q, k.repeat_interleave(G, dim=1)) * ac.D ** -0.5
    r, c = torch.arange(L)[:, None], torch.arange(L)[None, :]
    s = s.masked_fill(~((c <= r) & (c > r - W))[None], float("-inf"))
    want = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v.repeat_interleave(G, dim=1))
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)


# ---------- the inputs themselves ----------

def test_released_blocks_point_at_the_spare():
    for id in ("ragged-bf16-bs16-w16-needle-edge", "split-fp8-w64-poison-out",
               "long16400-w100-needle-edge"):
        case, _ = wc.win_decode_case(id)
        p = case.paged
        BS = p.k_cache.shape[2]
        some = False
        for b, L in enumerate(p.lens.tolist()):
            n = max(L - case.spec.W, 0) // BS
            some = some or n > 0
            assert (p.block_tables[b, :n] == p.spare).all()
            nb = -(-L // BS)
            assert torch.equal(p.block_tables[b, n:nb], case.full_tables[b, n:nb])
            assert (p.block_tables[b, n:nb] != p.spare).all()
        assert some, id
    case, _ = wc.win_prefill_case("cached300-bf16-w32-needle-edge")
    assert (case.paged.block_tables[:, :16] == case.paged.spare).all()
    assert (case.paged.block_tables[:, 16:19] != case.paged.spare).all()


def test_window_case_list_covers_the_paths():
    ids = set(wc.WIN_DECODE_BY_ID)
    for W in (1, 16, 63, 64, 65, 100):
        for BS in (16, 64):
            for t in ("bf16", "fp8"):
                for kind in ("needle-edge", "poison-out", "needle-last", "flat"):
                    c = wc.WIN_DECODE_BY_ID[f"ragged-{t}-bs{BS}-w{W}-{kind}"]
                    assert {1, W, W + 1, 63, 64, 65, 255, 256, 257} <= set(c.lens)
                    assert W == 1 or W - 1 in c.lens
    for W in (64, 2048, 2100):
        c = wc.WIN_DECODE_BY_ID[f"split-bf16-w{W}-needle-edge"]
        assert c.lens == (2049, 4097, 5000) and c.Hkv == 1
        # ops takes the split path once the window's span exceeds 2048 keys
        width = max(-(-L // c.BS) for L in c.lens) * c.BS
        assert (min(width, W + 64) > 2048) == (W >= 2048)
    assert "split-bf16-mix-w64-needle-edge" in ids
    long = wc.WIN_DECODE_BY_ID["long16400-w100-needle-edge"]
    assert (long.lens[0] - long.W) // long.BS < 1024 <= (long.lens[0] - 1) // long.BS
    assert {c.G for c in wc.WIN_DECODE_CASES} == {4, 7}
