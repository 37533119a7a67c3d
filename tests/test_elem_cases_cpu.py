"""CPU validation of the elementwise / sampling edge-test inputs
(elem_cases.py): the fp64 oracles agree with ops.reference within the
floors, the committed floors match what is measured, the input conditions
that make the sampling and filter answers unambiguous hold, and every
mutation a case lists moves its metric past MUTATION_MARGIN x the GPU bound
(or changes the sampled index / the kept set), so the GPU edge tests cannot
pass on a kernel that makes that mistake.

Run with -s to see the floors, the gaps and each mutation's margin."""

import pytest
import torch

from tests import elem_cases as ec
from llmapigateway_amd.ops import reference

RMS_IDS = [c.id for c in ec.RMS_CASES]
ROPE_IDS = [c.id for c in ec.ROPE_CASES]
SWIGLU_IDS = [c.id for c in ec.SWIGLU_CASES]
SAMPLE_IDS = [c.id for c in ec.SAMPLE_CASES]
FILTER_IDS = [c.id for c in ec.FILTER_CASES]


# ---------- ops.reference on each case (computed once, shared) ----------

def _rms_ref(id, fused):
    c = ec.rms_case(id)
    if fused:
        out, res = reference.rmsnorm_residual(c.x, c.residual.clone(), c.weight, c.spec.eps)
        return out, res
    return reference.rmsnorm(c.x, c.weight, c.spec.eps), None


def _rope_ref(id):
    c = ec.rope_case(id)
    buf = c.qkv.buf.clone()
    q, k, _ = c.qkv.views(buf)
    reference.rope_inplace(q, k, c.positions, c.cos_sin)
    return buf


@pytest.fixture(scope="module")
def floors():
    f = {"rmsnorm": {}, "rmsnorm_residual": {}, "rope": {}, "swiglu": {}}
    for id in RMS_IDS:
        c = ec.rms_case(id)
        f["rmsnorm"][id] = ec.rel_metric(_rms_ref(id, False)[0], ec.rmsnorm_oracle(c)[0])
        f["rmsnorm_residual"][id] = ec.rel_metric(
            _rms_ref(id, True)[0], ec.rmsnorm_oracle(c, fused=True)[0])
    for id in ROPE_IDS:
        c = ec.rope_case(id)
        ref, den = ec.rope_oracle(c.qkv, c.positions, c.cos_sin)
        f["rope"][id] = ec.rope_metric(_rope_ref(id)[:, :ref.shape[1]], ref, den)
    for id in SWIGLU_IDS:
        x = ec.swiglu_case(id)
        f["swiglu"][id] = ec.swiglu_metric(reference.swiglu(x), ec.swiglu_oracle(x))
    return f


@pytest.mark.parametrize("op,const,bound", [
    ("rmsnorm", ec.RMSNORM_FLOOR, ec.RMSNORM_BOUND),
    ("rmsnorm_residual", ec.RMSNORM_RESIDUAL_FLOOR, ec.RMSNORM_RESIDUAL_BOUND),
    ("rope", ec.ROPE_FLOOR, ec.ROPE_BOUND),
    ("swiglu", ec.SWIGLU_FLOOR, ec.SWIGLU_BOUND),
])
def test_floor_matches_constant(floors, op, const, bound):
    """Also the agreement of every oracle with ops.reference: the floor IS
    the metric of the reference against the oracle."""
    fl = floors[op]
    worst = max(fl, key=fl.get)
    for id, v in fl.items():
        print(f"floor {op} {id}: {v:.6f}")
    print(f"max F({op}) = {fl[worst]:.6f} at {worst}; constant {const}; bound {bound:.5f}")
    assert fl[worst] <= const
    assert const <= 1.25 * fl[worst]
    assert bound == ec.BOUND_FACTOR * const and ec.BOUND_FACTOR <= 4.0


# ---------- rmsnorm ----------

@pytest.mark.parametrize("id", RMS_IDS)
def test_rmsnorm_residual_oracle_is_bitwise_the_reference(id):
    c = ec.rms_case(id)
    _, res = _rms_ref(id, True)
    _, new_res = ec.rmsnorm_oracle(c, fused=True)
    assert torch.equal(ec.bits(res), ec.bits(new_res))
    assert not torch.isnan(ec.rmsnorm_oracle(c, fused=True)[0]).any()
    assert not torch.isnan(ec.rmsnorm_oracle(c)[0]).any()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("id", RMS_IDS)
def test_rmsnorm_mutations(id, fused):
    c = ec.rms_case(id)
    ref, _ = ec.rmsnorm_oracle(c, fused=fused)
    bound = ec.RMSNORM_RESIDUAL_BOUND if fused else ec.RMSNORM_BOUND
    assert c.spec.mutations
    for mut in c.spec.mutations:
        moved = ec.rel_metric(ec.rmsnorm_oracle(c, fused=fused, mutate=mut)[0], ref)
        print(f"mutation rmsnorm{'_residual' if fused else ''} {id} {mut}: "
              f"{moved:.4g} ({moved / bound:.1f} x bound)")
        assert not ec.passes(moved, ec.MUTATION_MARGIN * bound), (id, mut, moved)


def test_rmsnorm_metric_is_blind_to_the_unrounded_norm():
    """Stated so nobody relies on it (RMS_BLIND_TO): the effect of taking
    the norm on the unrounded residual sum stays inside one bf16 rounding."""
    assert "norm_unrounded" in ec.RMS_BLIND_TO
    for id in ("wave-v4-T7", "block-H8448-T8"):
        c = ec.rms_case(id)
        ref, _ = ec.rmsnorm_oracle(c, fused=True)
        moved = ec.rel_metric(ec.rmsnorm_oracle(c, fused=True, mutate="norm_unrounded")[0], ref)
        print(f"unrounded norm {id}: {moved:.5f}")
        assert moved < ec.RMSNORM_RESIDUAL_BOUND


def test_rmsnorm_cases_cover_the_dispatch():
    shapes = {(c.T, c.H) for c in ec.RMS_CASES}
    wave = {H // 512 for T, H in shapes if T <= 1024 and H <= 4096 and H % 512 == 0}
    assert wave == set(range(1, 9))
    assert {T % 4 for T, H in shapes if T <= 1024 and H % 512 == 0 and H <= 4096} >= {0, 1, 3}
    assert {8, 256, 4608, 5120, 8192, 8448, 16384} <= {H for _, H in shapes}
    assert {(1025, 512), (1025, 4096), (1024, 512)} <= shapes
    assert {c.eps for c in ec.RMS_CASES} == {1e-5, 1e-6}
    c = ec.rms_case("wave-v4-T7")
    assert (c.x[1] == 0).all() and float(c.x[2].float().abs().max()) < 2.0 ** -7
    assert ec.rms_is_wave(1024, 512) and not ec.rms_is_wave(1025, 512)
    assert not ec.rms_is_wave(8, 4608) and ec.rms_is_wave(7, 4096)


def _row_metric(got, ref):
    num = (got - ref).abs()
    return torch.where(ref != 0, num / ref.abs().clamp_min(1e-300),
                       torch.zeros_like(num)).amax(dim=-1)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("id", RMS_IDS)
def test_rmsnorm_spikes_cover_every_trip_and_each_one_is_sharp(id, fused):
    """Per case, not per module: the spike rows sit at the last chunk of
    the row, at the first chunk of the last trip of the kernel's row loop
    (wave form: the last VPL step; block form: the uneven or overflow
    trip), at the first chunk past the block form's register cache, and at
    chunks 63 / 64 / 0 as far as the case has spike rows; and dropping ANY
    ONE of these chunks from the sum of squares fails that row on its own,
    by MUTATION_MARGIN x the bound."""
    c = ec.rms_case(id)
    T, H = c.spec.T, c.spec.H
    nvec = H // 8
    placed = [p for p in c.spike_chunk if p >= 0]
    if nvec == 1:
        assert not placed
        return
    want = ec.spike_positions(T, H)
    n_rows = T - 2 if T >= 3 else T
    assert len(placed) == n_rows
    assert placed[:len(want)] == want[:n_rows]
    assert want[0] == nvec - 1
    if nvec > ec.rms_trip(T, H):
        assert want[1] == ((nvec - 1) // ec.rms_trip(T, H)) * ec.rms_trip(T, H)
    if not ec.rms_is_wave(T, H) and nvec > 1024:
        assert 1024 in want[:3]  # the first re-read chunk
    if T != 1:  # every multi-row case has room for the first entries
        assert n_rows >= min(len(want), 3), (id, n_rows, want)
    if T >= 7:
        assert set(placed) == set(want)  # 63, 64 and 0 too
    ref, _ = ec.rmsnorm_oracle(c, fused=fused)
    bad, _ = ec.rmsnorm_oracle(c, fused=fused, mutate="chunk_missing")
    moved = _row_metric(bad, ref)
    bound = ec.RMSNORM_RESIDUAL_BOUND if fused else ec.RMSNORM_BOUND
    rows = [r for r, p in enumerate(c.spike_chunk) if p >= 0]
    worst = min(float(moved[r]) for r in rows)
    print(f"spikes {id} fused={fused}: chunks {sorted(set(placed))}, weakest row moves "
          f"{worst:.3f} ({worst / bound:.0f} x bound)")
    for r in rows:
        assert float(moved[r]) > ec.MUTATION_MARGIN * bound, (id, r, c.spike_chunk[r])


# ---------- rope ----------

@pytest.mark.parametrize("id", ROPE_IDS)
def test_rope_mutations(id):
    c = ec.rope_case(id)
    ref, den = ec.rope_oracle(c.qkv, c.positions, c.cos_sin)
    for mut in c.spec.mutations:
        bad, _ = ec.rope_oracle(c.qkv, c.positions, c.cos_sin, mutate=mut)
        moved = ec.rope_metric(bad, ref, den)
        print(f"mutation rope {id} {mut}: {moved:.4g} ({moved / ec.ROPE_BOUND:.1f} x bound)")
        assert not ec.passes(moved, ec.MUTATION_MARGIN * ec.ROPE_BOUND), (id, mut, moved)


def test_rope_cases_cover_the_shapes():
    assert {c.D for c in ec.ROPE_CASES} == {32, 64, 128}
    assert {(c.Hq, c.Hkv) for c in ec.ROPE_CASES} == {(7, 1), (3, 3), (8, 2), (28, 4)}
    pairs = {(c.Hq + c.Hkv) * c.D // 2 for c in ec.ROPE_CASES}
    assert min(pairs) < 256 and 256 in pairs and any(p % 256 for p in pairs if p > 256)
    for D in (32, 64, 128):
        assert {c.T for c in ec.ROPE_CASES if c.D == D} == {1, 19}
        assert {c.theta for c in ec.ROPE_CASES if c.D == D} == {1e4, 5e5}
    pos = ec.rope_positions(19).tolist()
    assert 0 in pos and ec.MAX_POS - 1 in pos and len(set(pos)) < len(pos)
    assert pos != sorted(pos)


# ---------- swiglu ----------

@pytest.mark.parametrize("id", SWIGLU_IDS)
def test_swiglu_inputs_and_mutations(id):
    x = ec.swiglu_case(id)
    s = ec.SWIGLU_BY_ID[id]
    gate = x[:, :s.I].float()
    for edge in (88.0, -88.0, 89.0, -89.0, 100.0, -100.0):
        assert bool((gate == edge).any(dim=-1).all()), edge
    zero = gate == 0
    assert bool((zero & torch.signbit(gate)).any()) and bool((zero & ~torch.signbit(gate)).any())
    up = x[:, s.I:].float()
    assert bool((up > 0).any()) and bool((up < 0).any())
    ref = ec.swiglu_oracle(x)
    assert not torch.isnan(ref).any()
    for mut in s.mutations:
        moved = ec.swiglu_metric(ec.swiglu_oracle(x, mutate=mut), ref)
        print(f"mutation swiglu {id} {mut}: {moved:.4g}")
        assert not ec.passes(moved, ec.MUTATION_MARGIN * ec.SWIGLU_BOUND), (id, mut, moved)


# ---------- KV write ----------

@pytest.mark.parametrize("id", [c.id for c in ec.KV_CASES + ec.KV_FP8_CASES])
def test_kv_write_oracle_is_bitwise_the_reference(id):
    c = ec.kv_case(id)
    _, k, v = c.qkv.views()
    want = ec.kv_write_oracle(c.spec, k, v, c.slots)
    got = ec.empty_cache(c.spec)
    live = c.slots >= 0
    reference.kv_cache_write(k[live], v[live], got[0], got[1], c.slots[live],
                             got[2], got[3])
    for name, a, b in zip(("k_cache", "v_cache", "k_scale", "v_scale"), got, want):
        if a is not None:
            assert torch.equal(ec.bits(a), ec.bits(b)), (id, name)
    # the sentinels survive wherever no token was written
    slots = set(c.slots[live].tolist())
    assert {0, ec.NB * c.spec.BS - 1, c.spec.BS - 1, c.spec.BS} <= slots and -1 in c.slots.tolist()
    flat = want[0].permute(0, 2, 1, 3).reshape(ec.NB * c.spec.BS, -1)
    untouched = [s for s in range(ec.NB * c.spec.BS) if s not in slots]
    sent = ec.SENTINEL_BYTE if c.spec.fp8 else ec.SENTINEL_BF16_BITS
    assert bool((ec.bits(flat[untouched]) == sent).all())


def test_e4m3_oracle_on_the_special_rows():
    rows = ec._fp8_special_rows(64).to(ec.BF16)
    assert torch.equal(rows.float(), ec._fp8_special_rows(64))  # exact in bf16
    code, scale = ec.e4m3_quantize_oracle(rows)
    rc, rs = reference.fp8_quantize_rows(rows)
    assert torch.equal(code, rc) and torch.equal(ec.bits(scale), ec.bits(rs))
    assert scale.tolist()[0] == 1.0 and int(code[0].max()) == 0
    assert scale.tolist()[2] == 1.0
    # 17 -> 16, 19 -> 20, 2^-10 -> 0, 3 * 2^-10 -> 2^-8, -0.0 -> 0x80
    val = code[2].view(torch.float8_e4m3fn).float().tolist()
    assert val[1:4] == [16.0, 20.0, -20.0] and val[4] == 0.0 and val[5] == 2.0 ** -8
    assert int(code[2, 8]) == 0x80 and int(code[2, 6]) == 0x80
    tiny = code[1].view(torch.float8_e4m3fn).float().abs()
    assert bool((tiny == 0).any()) and bool(((tiny > 0) & (tiny < 2.0 ** -6)).any())


# ---------- sample ----------

@pytest.mark.parametrize("id", SAMPLE_IDS)
def test_sample_oracle_conditions_and_mutations(id):
    c = ec.sample_case(id)
    B, V = c.logits.shape
    scores = ec.sample_scores(c.logits, c.temperature, c.noise)
    want = ec.sample_oracle(scores)
    assert bool(((want >= 0) & (want < V)).all())
    # the structured oracle is the lowest-index argmax; reference.sample
    # (fp32, torch.argmax) picks the same token
    for b in range(B):
        row = scores[b]
        m = row.max()
        first = int((row == m).nonzero()[0]) if m > ec.NEG_INF else 0
        assert int(want[b]) == first, (id, b)
    ref = reference.sample(c.logits, c.temperature, c.noise)
    assert torch.equal(c.logits[torch.arange(B), ref].double().nan_to_num(neginf=-1e300),
                       c.logits[torch.arange(B), want].double().nan_to_num(neginf=-1e300))
    if c.spec.kind == "temp":
        assert torch.equal(ref, want)
        assert set(ec.TEMPS) >= {1e-7, 1e-3, 0.5, 1.0, 2.0, 100.0}
        assert bool((c.noise == 0).any()) and bool((c.noise == ec.NOISE_MAX).any())
        assert not torch.isinf(c.logits[torch.arange(B), want]).any()
        if V > 4:
            assert bool((torch.isinf(c.logits) & (c.noise == ec.NOISE_MAX)).any())
        for b, (lead, need) in enumerate(ec.sample_gaps(c)):
            print(f"gap {id} row {b} T={float(c.temperature[b]):g}: lead {lead:.4g} "
                  f"required {need:.4g}")
            assert lead >= need, (id, b, lead, need)
    for mut in c.spec.mutations:
        if mut in ("times_T", "neighbour_noise"):
            bad = ec.sample_oracle(ec.sample_scores(c.logits, c.temperature, c.noise, mut))
        else:
            bad = ec.sample_oracle(scores, mutate=mut)
        changed = int((bad != want).sum())
        print(f"mutation sample {id} {mut}: {changed} of {B} rows change")
        assert changed > 0, (id, mut)


def test_sample_cases_cover_the_sizes():
    assert {c.V for c in ec.SAMPLE_CASES if c.kind == "greedy"} == {
        1, 5, 15, 17, 512, 4097, 32000, 152064}
    forms = set()
    for id in SAMPLE_IDS:
        c = ec.sample_case(id)
        if c.spec.kind == "greedy":
            forms.add((c.noise is not None, bool((c.temperature < 0).all())))
            inf_rows = torch.isinf(c.logits).all(dim=-1)
            assert bool(inf_rows.any())
    assert forms == {(False, False), (True, False), (True, True)}


# ---------- topk_topp_filter ----------

@pytest.mark.parametrize("id", FILTER_IDS)
def test_filter_conditions_and_mutations(id):
    c = ec.filter_case(id)
    V = c.spec.V
    oracle = ec.filter_oracle(c)
    tails = 0
    for b, (fr, o) in enumerate(zip(c.rows, oracle)):
        p, k = float(c.topp[b]), int(c.topk[b])
        print(f"filter {id} row {b} {fr.kind} p={p:g} k={k}: keep {int(o.keep.sum())} "
              f"cut {o.cut:.5f} band {o.band} mass {o.mass_before:.6f}/{o.mass_at:.6f} "
              f"tail={o.tail}")
        span = c.logits[b][torch.isfinite(c.logits[b])]
        assert float(span.max() - span.min()) <= ec.FILTER_SPAN
        if fr.superset:
            continue
        assert o.band == 0, (id, b, "a logit lies in [c - G, c)")
        if p < 1.0:
            # either top-p decides and both sides clear p by the margin, or
            # top-k cuts strictly earlier and top-p's prefix is longer by
            # the same margin
            # (nothing precedes a crossing at the row maximum: mass 0)
            assert o.mass_before == 0 or o.mass_before < p - ec.MASS_MARGIN, (id, b)
            if o.p_decides:
                assert o.mass_at >= p + ec.MASS_MARGIN, (id, b)
        tails += o.tail
        # the exact semantics against reference.topk_topp_filter wherever no
        # tie straddles the cut (the reference breaks ties arbitrarily) and
        # the cut is near the top (its fp32 cumsum can pass 1.0 deep in the
        # tail, where it then masks under top-p = 1). The peaked and deep
        # rows with a tail cut therefore have NO second opinion: they are
        # checked against this module's fp64 oracle alone.
        if o.active and int(o.keep.sum()) == o.n_keep <= 64 and not o.tail:
            got = reference.topk_topp_filter(
                c.logits[b:b + 1].clone(), c.topp[b:b + 1], c.topk[b:b + 1])[0]
            assert torch.equal(got != ec.NEG_INF, o.keep & torch.isfinite(c.logits[b])), (id, b)
    if V > 50:
        assert tails >= 3  # peaked and deep rows cross below the first window
    pairs = {(fr.kind, fr.p, fr.k) for fr in c.rows}
    assert {("randn", 1.0, 0), ("randn", 1.0, 1), ("randn", 1.0, -1), ("randn", 1.0, -2)} <= pairs
    assert {1e-6, 0.5, 0.999} <= {fr.p for fr in c.rows}
    for mut in c.spec.mutations:
        bad = ec.filter_oracle(c, mutate=mut)
        changed = sum(int(not torch.equal(a.keep, b.keep))
                      for a, b, fr in zip(oracle, bad, c.rows) if not fr.superset)
        print(f"mutation filter {id} {mut}: {changed} of {len(oracle)} kept sets change")
        if mut == "tail_ignored" and V <= 50:
            continue  # k = 50 exceeds a 17-entry row: no tail case there
        assert changed > 0, (id, mut)
