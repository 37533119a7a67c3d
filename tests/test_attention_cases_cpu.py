"""CPU validation of the attention edge-test inputs (attn_cases.py): the
fp64 references agree with ops.reference, the measured noise floors match
the committed constants, and every needle / diagonal / poison case moves
the metric by >= SENSITIVITY_MIN under each mistake it is meant to expose,
so test_attention_edges_gpu.py cannot pass on a kernel that makes one.

Run with -s to see the per-case floors and margins."""

import pytest
import torch

from tests import attn_cases as ac
from llmapigateway_amd.ops import reference


def _decode_floor(id):
    case, ref64 = ac.decode_case(id)
    lo = ac.decode_reference(case, torch.float32, kv_round_bf16=True).bfloat16()
    return ac.metric(lo, ref64)


def _prefill_floor(id):
    case, ref64 = ac.prefill_case(id)
    lo = ac.prefill_reference(case, torch.float32, kv_round_bf16=True).bfloat16()
    return ac.metric(lo, ref64)


@pytest.fixture(scope="module")
def decode_floors():
    return {c.id: _decode_floor(c.id) for c in ac.DECODE_CASES}


@pytest.fixture(scope="module")
def prefill_floors():
    return {c.id: _prefill_floor(c.id) for c in ac.PREFILL_CASES}


def _check_floor(name, floors, const):
    worst = max(floors, key=floors.get)
    for id, f in floors.items():
        print(f"floor {name} {id}: {f:.6f}")
    print(f"max F({name}) = {floors[worst]:.6f} at {worst}; constant {const}; "
          f"bound {4 * const:.4f}")
    # the constant covers every case and is not inflated past the measurement
    assert floors[worst] <= const
    assert const <= 1.25 * floors[worst]


def test_decode_floor_matches_constant(decode_floors):
    _check_floor("decode", decode_floors, ac.DECODE_FLOOR)
    assert ac.ATTN_BOUND_DECODE == 4.0 * ac.DECODE_FLOOR


def test_prefill_floor_matches_constant(prefill_floors):
    _check_floor("prefill", prefill_floors, ac.PREFILL_FLOOR)
    assert ac.ATTN_BOUND_PREFILL == 4.0 * ac.PREFILL_FLOOR


@pytest.mark.parametrize("id", [c.id for c in ac.DECODE_CASES])
def test_decode_reference_agrees_with_ops_reference(id):
    """Both on the CPU; the difference is fp32 rounding plus the bf16 result."""
    case, ref64 = ac.decode_case(id)
    p = case.paged
    got = reference.attention_decode(
        case.q, p.k_cache, p.v_cache, p.block_tables, p.lens, case.scale,
        k_scale=p.k_scale, v_scale=p.v_scale)
    assert not torch.isnan(got).any()
    assert ac.metric(got, ref64) <= ac.DECODE_FLOOR


@pytest.mark.parametrize("id", [c.id for c in ac.PREFILL_CASES])
def test_prefill_reference_agrees_with_ops_reference(id):
    case, ref64 = ac.prefill_case(id)
    p = case.paged
    kw = {}
    if p is not None:
        kw = dict(k_cache=p.k_cache, v_cache=p.v_cache, block_tables=p.block_tables,
                  cached_lens=p.lens, k_scale=p.k_scale, v_scale=p.v_scale)
    got = reference.attention_prefill(
        case.q, case.k, case.v, case.cu_seqlens, case.scale, True, **kw)
    assert not torch.isnan(got).any()
    assert ac.metric(got, ref64) <= ac.PREFILL_FLOOR


@pytest.mark.parametrize(
    "id", [c.id for c in ac.DECODE_CASES if c.kind == "needle"])
def test_decode_needle_sensitivity(id):
    case, ref64 = ac.decode_case(id)
    assert case.mutations
    for mut in case.mutations:
        moved = ac.metric(ac.decode_reference(case, mutate=mut), ref64)
        print(f"sensitivity {id} {mut}: {moved:.3f}")
        assert moved >= ac.SENSITIVITY_MIN, (id, mut, moved)


@pytest.mark.parametrize(
    "id", [c.id for c in ac.PREFILL_CASES if c.kind != "flat"])
def test_prefill_sensitivity(id):
    case, ref64 = ac.prefill_case(id)
    assert case.mutations
    for mut in case.mutations:
        moved = ac.metric(ac.prefill_reference(case, mutate=mut), ref64)
        print(f"sensitivity {id} {mut}: {moved:.3f}")
        assert moved >= ac.SENSITIVITY_MIN, (id, mut, moved)


def test_flat_cases_are_blind_to_single_key_mistakes():
    """What the flat family (the only family of the older tests) cannot
    see, stated so nobody relies on it: with the last key dropped, the
    largest absolute output change stays inside the 0.05 that the older
    tests accept, at their lengths and at the split-path lengths. The same
    holds for every mutation in FLAT_BLIND_TO; no claim beyond that."""
    assert {"drop", "short"} <= set(ac.FLAT_BLIND_TO)
    for id, lens in (("flat200", (200, 300)), ("flat-split", (2049, 5000))):
        case = ac.build_decode(ac.DecodeSpec(id=id, lens=lens, Hkv=1, seed=77))
        moved = (ac.decode_reference(case, mutate="short")
                 - ac.decode_reference(case)).abs().max().item()
        print(f"flat decode {lens}, last key dropped: max abs change {moved:.4f}")
        assert moved < 0.05  # the older tests' tolerance


def test_poisoned_slots_are_everything_unused():
    """Every cache slot is either addressed by some (seq, pos < L) or NaN
    (0x7f with a NaN scale for fp8), and table entries past a sequence's
    last used block point at the in-range spare block."""
    for id in ("ragged-bs16-needle-last", "ragged-fp8-needle-last", "empty-row-split"):
        case, _ = ac.decode_case(id)
        p = case.paged
        NB, Hkv, BS, _ = p.k_cache.shape
        live = torch.zeros(NB, BS, dtype=torch.bool)
        for b, L in enumerate(p.lens.tolist()):
            nb = (L + BS - 1) // BS
            assert (p.block_tables[b, nb:] == p.spare).all()
            assert ((p.block_tables[b] >= 0) & (p.block_tables[b] < NB)).all()
            for pos in range(L):
                live[int(p.block_tables[b, pos // BS]), pos % BS] = True
        assert not live[p.spare].any()
        assert live.sum() == int(p.lens.sum())
        for cache, sc in ((p.k_cache, p.k_scale), (p.v_cache, p.v_scale)):
            rows = cache.permute(0, 2, 1, 3).reshape(NB, BS, -1)
            if sc is None:
                assert torch.isnan(rows[~live]).all()
                assert not torch.isnan(rows[live]).any()
            else:
                assert (rows[~live] == ac.FP8_NAN_BYTE).all()
                srows = sc.permute(0, 2, 1).reshape(NB, BS, -1)
                assert torch.isnan(srows[~live]).all()
                assert not torch.isnan(srows[live]).any()


def test_case_list_covers_the_paths():
    """The shapes that select each kernel path are present."""
    ids = set(ac.DECODE_BY_ID)
    assert {f"G{g}-needle-last" for g in range(1, 9)} <= ids
    long = ac.DECODE_BY_ID["long16400-needle-16384"]
    assert -(-long.lens[0] // long.BS) == 1025  # > 1024 block-table entries
    for c in ac.DECODE_CASES:
        assert c.Hkv <= 2 and len(c.lens) * c.Hkv < 192
        if c.id.startswith(("split-", "long", "empty-row-split")):
            width = max(c.width, max(-(-L // c.BS) for L in c.lens))
            assert width * c.BS > 2048, c.id  # ops takes the split path
