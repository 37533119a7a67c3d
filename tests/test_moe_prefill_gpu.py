"""The 128-row prefill tile of the grouped expert GEMM (csrc/moe_prefill.hip,
mf = 8) against the fp32 reference and, bit for bit, the 64-row kernels."""

import math

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.models.configs import ModelConfig
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel
from llmapigateway_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 1024  # guard elements on each side
CANARY = 0x5A
MF, BM = 8, 128
PATTERNS = ["random", "one_expert", "one_unused", "bm_and_bm_plus_1"]
TINY_MOE = ModelConfig(  # as in test_moe_gpu.py
    name="tiny-mixtral-hd128", hidden_size=256, intermediate_size=512,
    num_layers=2, num_heads=2, num_kv_heads=1, vocab_size=512, head_dim=128,
    rope_theta=10000.0, max_positions=512, num_experts=4, experts_per_token=2,
)


def _guarded(shape, dtype):
    numel = math.prod(shape)
    buf = torch.empty(numel + 2 * PAD, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(CANARY)

    def check(name):
        torch.cuda.synchronize()
        for part in (buf[:PAD], buf[PAD + numel :]):
            assert bool((part.view(torch.uint8) == CANARY).all()), f"{name}: guard clobbered"

    return buf[PAD : PAD + numel].view(shape), check


def _ids(pattern, T, k, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = T * k
    if pattern == "one_expert":
        flat = torch.full((P,), E - 1)
    elif pattern == "one_unused":
        flat = torch.randint(0, E - 1, (P,), generator=g) + 1  # expert 0 idle
    elif pattern == "bm_and_bm_plus_1":  # expert 0: BM pairs, expert 1: BM + 1
        flat = torch.randint(2, E, (P,), generator=g)
        flat[:BM], flat[BM : 2 * BM + 1] = 0, 1
    else:
        flat = torch.randint(0, E, (P,), generator=g)
    return flat.to(torch.int32).view(T, k)


def _tri(shape, g):
    return (torch.randint(0, 3, shape, generator=g) - 1).bfloat16()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_align(pattern):
    T, k, E = 200, 2, 8
    ids = _ids(pattern, T, k, E)
    cap = ops.moe_cap(T * k, E, MF)
    sp, chk_s = _guarded((cap,), torch.int32)
    te, chk_t = _guarded((cap // BM,), torch.int32)
    ops._native().moe_align(sp, te, ids.to(DEV), E, MF)
    chk_s("sorted_pairs")
    chk_t("tile_expert")
    sp, te, flat = sp.cpu(), te.cpu(), ids.view(-1)
    assert torch.equal(sp[sp >= 0].sort().values, torch.arange(T * k, dtype=torch.int32))
    assert bool((sp[sp < 0] == -1).all())
    for t, e in enumerate(te.tolist()):
        rows = sp[t * BM : (t + 1) * BM]
        if e < 0:
            assert bool((rows == -1).all())
        else:
            assert rows[0] >= 0 and bool((flat[rows[rows >= 0].long()] == e).all())
    if pattern == "bm_and_bm_plus_1":
        assert te.tolist()[:3] == [0, 1, 1] and sp[3 * BM - 1] == -1 and sp[2 * BM] >= 0


@pytest.mark.parametrize("T", [1, 65, 200])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("H,inter", [(128, 64), (384, 192), (128, 448)])
def test_down_exact(H, inter, pattern, T):
    """Integer data, weights in {0.5, 1, 2}: exact sums and one rounding, so
    y_pair is bit-equal. 1, 3 and 7 k-tiles; act rows without a pair hold NaN."""
    k, E = 2, 4
    g = torch.Generator().manual_seed(T)
    ids = _ids(pattern, T, k, E)
    act, w_down = _tri((T * k, inter), g), _tri((E, H, inter), g)
    wts = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T, k), generator=g)]
    ref = reference.moe_down(act, ids, wts, w_down)

    plan = ops.moe_align(ids.to(DEV), E, MF)
    sp = plan.sorted_pairs.cpu().long()
    act_sorted = torch.full((plan.cap, inter), float("nan")).bfloat16()
    act_sorted[sp >= 0] = act[sp[sp >= 0]]
    y, chk = _guarded((T * k, H), torch.bfloat16)
    ops.moe_down(act_sorted.to(DEV), ids.to(DEV), wts.to(DEV),
                 ops.moe_pack_weights(w_down.to(DEV), False), plan, out=y)
    chk("y_pair")
    assert torch.equal(y.cpu(), ref)


def _mlp_case(T, H, inter, E, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).bfloat16()
    res = torch.randn(T, H, generator=g).bfloat16()
    w_gu = (torch.randn(E, 2 * inter, H, generator=g) * 0.05).bfloat16()
    w_dn = (torch.randn(E, H, inter, generator=g) * 0.05).bfloat16()
    norm_w = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16()
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    wts = torch.rand(T, k, generator=g) + 0.1
    return x, res, w_gu, w_dn, norm_w, ids, wts / wts.sum(-1, keepdim=True)


def _err(got, ref):
    return ((got.float() - ref.float()).abs().max() / (ref.float().abs().max() + 1e-3)).item()


@pytest.mark.parametrize("T", [1, 65, 200])
@pytest.mark.parametrize("H,inter", [(64, 64), (448, 192)])
def test_gate_up_swiglu(H, inter, T):
    E, k = 4, 2
    x, _, w_gu, _, _, ids, _ = _mlp_case(T, H, inter, E, k, T + H)
    w = ops.moe_pack_weights(w_gu.to(DEV), True)
    by_pair = []
    for mf in (MF, 4):
        plan = ops.moe_align(ids.to(DEV), E, mf)
        act, chk = _guarded((plan.cap, inter), torch.bfloat16)
        ops.moe_gate_up_swiglu(x.to(DEV), ids.to(DEV), w, plan, out=act)
        chk("act")
        sp, act = plan.sorted_pairs.cpu().long(), act.cpu()
        assert bool((act[sp < 0].view(torch.uint8) == CANARY).all())
        rows = torch.empty(T * k, inter, dtype=torch.bfloat16)
        rows[sp[sp >= 0]] = act[sp >= 0]
        by_pair.append(rows)
    err = _err(by_pair[0], reference.moe_gate_up_swiglu(x, ids, w_gu))
    print(f"T={T} H={H} I={inter}: act err {err:.5f}")
    assert err < 0.02
    assert torch.equal(by_pair[0], by_pair[1])


@pytest.mark.parametrize("H", [256, 192])
def test_moe_mlp_route(H, monkeypatch):
    """150 pairs per expert: the 128-row tile where it serves H, else the
    64-row kernels, and the same bits either way."""
    T, E, k, inter = 300, 4, 2, 192
    x, res, w_gu, w_dn, norm_w, ids, wts = _mlp_case(T, H, inter, E, k, H)
    ref = ops.moe_mlp(x, None, w_gu, w_dn, k, res.clone(), norm_w, 1e-5, ids=ids, weights=wts)
    d = lambda t: t.to(DEV)
    args = (d(x), None, ops.moe_pack_weights(d(w_gu), True), ops.moe_pack_weights(d(w_dn), False), k)
    seen, align = [], ops.moe_align
    monkeypatch.setattr(ops, "moe_align", lambda i, e, mf=None: seen.append(mf) or align(i, e, mf))
    got = []
    for min_rows in (128, 10**9):
        monkeypatch.setenv("LLMAPI_MOE_BIG_MIN_ROWS", str(min_rows))
        got.append(ops.moe_mlp(*args, d(res).clone(), d(norm_w), 1e-5, ids=d(ids), weights=d(wts)))
    assert seen == [MF if H % 128 == 0 else None, None]
    for a, b, r in zip(got[0], got[1], ref):
        assert torch.equal(a, b)
        assert _err(a.cpu(), r) < 0.02


def test_model_prefill(monkeypatch):
    """512 tokens, 256 pairs per expert: logits do not depend on the row tile."""
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    T = 512
    model = LlamaModel(TINY_MOE, device=DEV, seed=0)
    toks = torch.randint(0, TINY_MOE.vocab_size, (T,), generator=torch.Generator().manual_seed(5))
    seen, align = [], ops.moe_align
    monkeypatch.setattr(ops, "moe_align", lambda i, e, mf=None: seen.append(mf) or align(i, e, mf))
    logits = []
    for min_rows in (128, 10**9):
        monkeypatch.setenv("LLMAPI_MOE_BIG_MIN_ROWS", str(min_rows))
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
