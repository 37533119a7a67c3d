"""The 128-row prefill tile with MXFP4 expert weights (csrc/moe_w4_prefill.hip,
mf = 8): bit for bit the bf16 128-row tile on the dequantised weights, exact
against the fp32 reference, and the moe_mlp / model route."""

import functools

import pytest
import torch
from test_moe_prefill_gpu import CANARY, DEV, MF, PATTERNS, TINY_MOE, _guarded, _ids

from llmapigateway_amd import ops
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel
from llmapigateway_amd.ops import reference

pytestmark = pytest.mark.gpu

E, TOPK = 4, 2


def _quantize(w):
    """[E, N, K] -> (packed, scale, dequantised bf16), expert by expert."""
    qs = [ops.mxfp4_quantize_weight(w[e]) for e in range(w.shape[0])]
    q, s = torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs])
    return q, s, reference.moe_dequantize_experts_mxfp4(q, s)


@functools.lru_cache(maxsize=None)
def _panels(N, K, gate_up):
    g = torch.Generator().manual_seed(N * 7 + K)
    q, s, wd = _quantize((torch.randn(E, N, K, generator=g) * 0.05).bfloat16())
    return (*ops.moe_pack_weights_mxfp4(q.to(DEV), s.to(DEV), gate_up),
            ops.moe_pack_weights(wd.to(DEV), gate_up))


@pytest.mark.parametrize("T", [1, 65, 200])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", [128, 256, 384, 640])
@pytest.mark.parametrize("nb", [1, 3])
def test_bit_identical_to_bf16_tile(nb, K, pattern, T):
    """The convert is exact and the MFMA inputs and order are moe_gemm_big's,
    so both epilogues equal that kernel on the dequantised weights bit for
    bit under the same plan. K in k64 tiles: fewer than the ring, the ring,
    one and a half rings, more than two; N: 1 and 3 column blocks of 128."""
    g = torch.Generator().manual_seed(T + K)
    ids = _ids(pattern, T, TOPK, E).to(DEV)
    wts = (torch.rand(T, TOPK, generator=g) + 0.1).to(DEV)
    plan = ops.moe_align(ids, E, MF)
    real = plan.sorted_pairs >= 0
    q4, s4, wbf = _panels(nb * 128, K, True)
    x = torch.randn(T, K, generator=g).bfloat16().to(DEV)
    act, chk = _guarded((plan.cap, nb * 64), torch.bfloat16)
    ops.moe_gate_up_swiglu(x, ids, q4, plan, out=act, s_gate_up=s4)
    chk("act")
    assert torch.equal(act[real], ops.moe_gate_up_swiglu(x, ids, wbf, plan)[real])
    assert bool((act[~real].view(torch.uint8) == CANARY).all())  # padding rows

    q4, s4, wbf = _panels(nb * 128, K, False)
    a = torch.randn(plan.cap, K, generator=g).bfloat16().to(DEV)
    y, chk = _guarded((T * TOPK, nb * 128), torch.bfloat16)
    ops.moe_down(a, ids, wts, q4, plan, out=y, s_down=s4)
    chk("y_pair")
    assert torch.equal(y, ops.moe_down(a, ids, wts, wbf, plan))


@pytest.mark.parametrize("T", [1, 65, 200])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", [128, 640])
def test_down_exact(K, pattern, T):
    """Ternary act, ternary weights times 2^-3..2^3 per (column, block) (so
    MXFP4 holds them exactly), routing weights in {0.5, 1, 2}: every sum is
    below 2^24 in units of 2^-3, fp32 is exact and there is one rounding, so
    y_pair is bit-equal to the fp32 reference. Rows without a pair hold NaN."""
    H = 128
    g = torch.Generator().manual_seed(T + K)
    tri = lambda *shape: (torch.randint(0, 3, shape, generator=g) - 1).float()
    ids, act = _ids(pattern, T, TOPK, E), tri(T * TOPK, K).bfloat16()
    exps = torch.randint(-3, 4, (E, H, K // 32, 1), generator=g).float()
    w = (tri(E, H, K // 32, 32) * torch.exp2(exps)).view(E, H, K).bfloat16()
    q, s, wd = _quantize(w)
    assert torch.equal(wd, w)
    wts = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T, TOPK), generator=g)]
    plan = ops.moe_align(ids.to(DEV), E, MF)
    sp = plan.sorted_pairs.cpu().long()
    act_sorted = torch.full((plan.cap, K), float("nan")).bfloat16()
    act_sorted[sp >= 0] = act[sp[sp >= 0]]
    y, chk = _guarded((T * TOPK, H), torch.bfloat16)
    q4, s4 = ops.moe_pack_weights_mxfp4(q.to(DEV), s.to(DEV), False)
    ops.moe_down(act_sorted.to(DEV), ids.to(DEV), wts.to(DEV), q4, plan, out=y, s_down=s4)
    chk("y_pair")
    assert torch.equal(y.cpu(), reference.moe_down(act, ids, wts, wd))


def _spy_align(monkeypatch):
    seen, align = [], ops.moe_align
    monkeypatch.setattr(ops, "moe_align", lambda i, e, mf=None: seen.append(mf) or align(i, e, mf))
    return seen


def test_moe_mlp_route(monkeypatch):
    """150 pairs per expert: the 128-row tile at the knob's threshold, the
    64-row kernels above it, and the same bits either way. (H = 192, which
    the tile does not serve, cannot be packed as MXFP4 either: that half of
    the route is in test_moe_w4_prefill_cpu.py.)"""
    T, H, inter = 300, 256, 256
    g = torch.Generator().manual_seed(H)
    x, res = (torch.randn(T, H, generator=g).bfloat16().to(DEV) for _ in range(2))
    ids = torch.stack([torch.randperm(E, generator=g)[:TOPK] for _ in range(T)])
    ids, wts = ids.to(torch.int32).to(DEV), (torch.rand(T, TOPK, generator=g) + 0.1).to(DEV)
    (gq, gs, _), (dq, ds, _) = _panels(2 * inter, H, True), _panels(H, inter, False)
    norm_w = torch.ones(H, dtype=torch.bfloat16, device=DEV)
    seen = _spy_align(monkeypatch)
    got = []
    for min_rows in (128, 10**9):
        monkeypatch.setenv("LLMAPI_MOE_W4_BIG_MIN_ROWS", str(min_rows))
        got.append(ops.moe_mlp(x, None, gq, dq, TOPK, res.clone(), norm_w, 1e-5,
                               ids=ids, weights=wts, s_gate_up=gs, s_down=ds))
    assert seen == [MF, None]
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_model_prefill(monkeypatch):
    """512 tokens, 256 pairs per expert: logits do not depend on the row tile."""
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    T = 512
    model = LlamaModel(TINY_MOE, device=DEV, seed=0, weight_dtype="mxfp4")
    toks = torch.randint(0, TINY_MOE.vocab_size, (T,), generator=torch.Generator().manual_seed(5))
    seen = _spy_align(monkeypatch)
    logits = []
    for min_rows in (128, 10**9):
        monkeypatch.setenv("LLMAPI_MOE_W4_BIG_MIN_ROWS", str(min_rows))
        kv = PagedKVCache(TINY_MOE, T // 16, 16, DEV, torch.bfloat16)
        batch = ForwardBatch(
            kind="prefill", token_ids=toks.to(DEV), positions=torch.arange(T, device=DEV),
            slot_mapping=torch.arange(T, device=DEV),
            cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device=DEV), max_seqlen=T,
            logits_indices=torch.arange(T, device=DEV),
        )
        logits.append(model.forward(batch, kv.k_caches, kv.v_caches).cpu())
    assert seen == [MF, MF, None, None]  # two layers per forward
    assert torch.equal(logits[0], logits[1])
