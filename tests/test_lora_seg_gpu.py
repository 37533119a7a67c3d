"""Segmented multi-LoRA on the GPU (csrc/lora_seg.hip): lora_align's plan,
the MFMA shrink / expand pair called with an explicit plan, lora_add's
dispatch, the model prefill and the engine's captured graphs.

Oracles: ops.reference on exact integer data, a float64 evaluation of the
same bf16 inputs on random data (the vector pair of csrc/lora.hip gives the
error to stay within)."""

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel
from test_lora_gpu import (
    DEV, TINY, _bounds, _cpu_twin, _delta_err, _engine, _exact_case, _guarded,
    _random_stack, _run_batch, _run_gpu, _run_ref,
)

pytestmark = pytest.mark.gpu
HUGE = 1 << 30


def _run_seg(x, A, B, ranks, scales, ids, bounds, y0, mf=None, nsk=None):
    """align + shrink_seg + expand_seg with guards around the partials and y
    -> (y on the CPU, plan)."""
    d = lambda v: v.to(DEV)
    ids_d, rk = d(ids), d(ranks)
    plan = ops.lora_align(ids_d, rk, mf)
    if nsk is None:
        nsk = ops._native().lora_pick_nsk(x.shape[0], plan.mf, len(bounds), x.shape[1])
    tp, tcheck = _guarded((nsk, plan.cap, A.shape[1]), torch.float32)
    y, ycheck = _guarded(tuple(y0.shape), torch.bfloat16, fill=y0.to(DEV))
    ops.lora_shrink_seg(d(x), d(A), rk, ids_d, len(bounds), plan, out=tp)
    out = ops.lora_expand_seg(y, tp, d(B), rk, d(scales), ids_d, bounds, plan)
    assert out.data_ptr() == y.data_ptr()
    tcheck("lora_shrink_seg partials")
    ycheck("lora_expand_seg y")
    return y.cpu(), plan


def _check_exact(case, mf, nsk=None):
    x, A, B, ranks, scales, ids, bounds, y0 = case
    _, y_ref = _run_ref(*case)
    y, plan = _run_seg(*case, mf=mf, nsk=nsk)
    assert torch.equal(y, y_ref)
    base = ids < 0
    assert torch.equal(y[base].view(torch.int16), y0[base].view(torch.int16))
    # the plan: every row of a slot once, slots and rows ascending (stable)
    bm, rows = 16 * mf, plan.sorted_rows.cpu()
    want = [r for s in range(len(ranks)) for r in range(len(ids)) if ids[r] == s]
    assert rows[rows >= 0].tolist() == want
    tiles = rows.view(-1, bm)
    slot_of = torch.where(tiles[:, 0] >= 0, ids[tiles[:, 0].clamp(min=0).long()], -1)
    assert torch.equal(plan.tile_slot.cpu(), slot_of.int())
    return y


@pytest.mark.parametrize("mf", [1, 2, 4])
@pytest.mark.parametrize("rank", [1, 8, 24, 64])
@pytest.mark.parametrize("N,nseg", [(64, 1), (192, 3)])
@pytest.mark.parametrize("T", [1, 17, 256])
def test_exact_integer_data(T, N, nseg, rank, mf):
    _check_exact(_exact_case(T, N, rank, nseg), mf)


def test_split_k_gives_the_same_bits():
    """K = 448: 14 k-steps of 32, divisible neither by 3 slices nor by the
    four waves. Integer data: every partial sum is exact in fp32."""
    T, N, K, R, S = 40, 64, 448, 16, 3
    g = torch.Generator(device="cpu").manual_seed(11)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    x = ri(-1, 2, (T, K)).bfloat16()
    A = ri(-1, 2, (S, R, K)).bfloat16()
    B = torch.zeros(S, N, R)
    for s in range(S):
        B[s, torch.arange(N), ri(0, R, (N,))] = (ri(0, 2, (N,)) * 2 - 1).float()
    case = (
        x, A, B.bfloat16(), torch.full((S,), R, dtype=torch.int32),
        torch.tensor([0.5, 1.0, 2.0]), ri(-1, S, (T,)).int(), (N,),
        ri(-64, 65, (T, N)).bfloat16(),
    )
    y1 = _check_exact(case, 1, nsk=1)
    y3 = _check_exact(case, 1, nsk=3)
    assert torch.equal(y1.view(torch.int16), y3.view(torch.int16))


@pytest.mark.parametrize("pattern", ["one_slot", "one_unused", "bm_and_bm1", "all_base"])
@pytest.mark.parametrize("mf", [1, 2, 4])
def test_segment_edge_patterns(mf, pattern):
    bm = 16 * mf
    T = 2 * bm + 1
    x, A, B, ranks, scales, _, bounds, y0 = _exact_case(T, 192, 24, 3)
    ids = {
        "one_slot": torch.full((T,), 1),
        "one_unused": torch.arange(T) % 2 * 2,
        "bm_and_bm1": (torch.arange(T) >= bm).long(),
        "all_base": torch.full((T,), -1),
    }[pattern].int()
    y = _check_exact((x, A, B, ranks, scales, ids, bounds, y0), mf)
    if pattern == "all_base":  # a plan with no used tile
        assert torch.equal(y.view(torch.int16), y0.view(torch.int16))


def _ref64(x, A, B, ranks, scales, ids, bounds):
    """The adapter delta of every row in float64, from the bf16 inputs."""
    R, out = B.shape[2], torch.zeros(x.shape[0], B.shape[1], dtype=torch.float64)
    for slot in range(A.shape[0]):
        rows, lo = ids == slot, 0
        for s, hi in enumerate(bounds):
            t = x[rows].double() @ A[slot, s * R : (s + 1) * R].double().T
            out[rows, lo:hi] = float(scales[slot]) * (t @ B[slot, lo:hi].double().T)
            lo = hi
    return out


@pytest.mark.parametrize("T", [7, 200])
@pytest.mark.parametrize("rank", [5, 64])
@pytest.mark.parametrize("N", [64, 6144])
@pytest.mark.parametrize("K", [64, 4096])
def test_numerics_random_against_fp64(K, N, rank, T):
    """Both pairs end in the same single bf16 rounding of y; the hi/lo split
    of t leaves the MFMA pair one fp32 accumulation order away from the
    vector pair, so it may err at most twice as much."""
    nseg = 3 if N % 48 == 0 else 1
    A, B, ranks, scales = _random_stack(N, K, rank, nseg)
    g = torch.Generator(device="cpu").manual_seed(T + N + K)
    x = (torch.randn(T, K, generator=g) * 0.5).bfloat16()
    ids = (torch.arange(T) % 4).int()
    case = (x, A, B, ranks, scales, ids, _bounds(N, nseg), torch.zeros(T, N).bfloat16())
    ref = _ref64(*case[:-1])
    err_vec = _delta_err(_run_gpu(*case)[1].double(), ref)
    err_seg = _delta_err(_run_seg(*case)[0].double(), ref)
    print(f"T={T} N={N} K={K} rank={rank}: err vector {err_vec:.3e} segmented {err_seg:.3e}")
    assert err_vec > 0
    assert err_seg <= 2 * err_vec


def _add(monkeypatch, min_t, stack, x, ids):
    monkeypatch.setattr(ops, "LORA_SEG_MIN_T", min_t)
    y = torch.zeros(x.shape[0], stack.B.shape[1], dtype=torch.bfloat16, device=DEV)
    return ops.lora_add(y, x.to(DEV), stack, ids.to(DEV)).cpu()


def test_lora_add_dispatch(monkeypatch):
    T, N, K, rank = 32, 192, 448, 16
    g = torch.Generator(device="cpu").manual_seed(9)
    ids = (torch.arange(T) % 5 - 1).int()
    for bounds in (_bounds(N, 3), (8, 64)):
        N, nseg = bounds[-1], len(bounds)
        A, B, ranks, scales = _random_stack(N, K, rank, nseg)
        x = (torch.randn(T, K, generator=g) * 0.5).bfloat16()
        stack = ops.LoraStack(*(v.to(DEV) for v in (A, B, ranks, scales)), bounds)
        y_seg = _add(monkeypatch, 1, stack, x, ids)
        y_vec = _add(monkeypatch, HUGE, stack, x, ids)
        if bounds[0] % 16:  # not served: threshold 1 still takes the vector pair
            assert torch.equal(y_seg.view(torch.int16), y_vec.view(torch.int16))
            continue
        ref = _ref64(x, A, B, ranks, scales, ids, bounds)
        err_vec, err_seg = _delta_err(y_vec.double(), ref), _delta_err(y_seg.double(), ref)
        print(f"lora_add T={T}: err vector {err_vec:.3e} segmented {err_seg:.3e}")
        assert err_vec > 0
        assert err_seg <= 2 * err_vec


def _prefill_logits(model, ids, n_seq=4, seq_len=10):
    """n_seq prompts of seq_len tokens in one prefill forward -> logits of
    every row; ids: adapter slot per prompt, or None."""
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    dev, T = model.device, n_seq * seq_len
    kv = PagedKVCache(model.config, n_seq, 16, dev, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(5)
    toks = torch.randint(0, model.config.vocab_size, (T,), generator=g)
    seq = torch.arange(T) // seq_len
    batch = ForwardBatch(
        kind="prefill",
        token_ids=toks.to(dev),
        positions=(torch.arange(T) % seq_len).to(dev),
        slot_mapping=(seq * 16 + torch.arange(T) % seq_len).to(dev),
        cu_seqlens=(torch.arange(n_seq + 1, dtype=torch.int32) * seq_len).to(dev),
        max_seqlen=seq_len,
        logits_indices=torch.arange(T).to(dev),
        adapter_ids=None if ids is None else ids[seq].to(dev),
    )
    return model.forward(batch, kv.k_caches, kv.v_caches).float().cpu()


def test_model_prefill_mixed_batch(monkeypatch):
    """40-token prefill of tiny-llama, prompts on [a, base, b, a]: the
    segmented route may differ from the CPU reference path by at most twice
    what the vector route differs by on the same forward."""
    model = LlamaModel(TINY, device=DEV, seed=0, max_loras=2, max_lora_rank=16)
    model.set_adapter(0, model.random_adapter(16, seed=1), alpha=32.0)
    model.set_adapter(1, model.random_adapter(5, seed=2), alpha=10.0)
    ids = torch.tensor([0, -1, 1, 0], dtype=torch.int32)
    ref = _prefill_logits(_cpu_twin(model), ids)
    monkeypatch.setattr(ops, "LORA_SEG_MIN_T", HUGE)
    err_vec = (_prefill_logits(model, ids) - ref).abs().max().item()
    monkeypatch.setattr(ops, "LORA_SEG_MIN_T", 1)
    got = _prefill_logits(model, ids)
    err_seg = (got - ref).abs().max().item()
    print(f"prefill logits gpu-vs-cpu: vector {err_vec:.5f} segmented {err_seg:.5f}")
    assert err_vec > 0
    assert err_seg <= 2 * err_vec
    # the base prompt's rows equal those of a batch without adapters
    all_base = _prefill_logits(model, torch.full((4,), -1, dtype=torch.int32))
    assert torch.equal(got[10:20], all_base[10:20])
    assert not torch.equal(got[:10], all_base[:10])


def test_engine_graph_equals_eager_on_the_segmented_route(monkeypatch):
    monkeypatch.setattr(ops, "LORA_SEG_MIN_T", 1)
    mix, outs = ["a", None, "b", "a"], {}
    for graph in (True, False):
        eng = _engine(graph)
        eng.load_adapter("a", rank=16, alpha=64.0, seed=1)
        eng.load_adapter("b", rank=4, alpha=16.0, seed=2)
        outs[graph] = _run_batch(eng, mix)
        if graph:
            assert eng.stats["graph_steps"] >= 16
            assert _run_batch(eng, mix) == outs[True]  # the graphs, replayed
            base = _run_batch(eng, [None] * 4)
    assert outs[True] == outs[False]
    assert outs[True][0] != base[0] and outs[True][1] == base[1]
