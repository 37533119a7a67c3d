"""Mixture of experts on the GPU: routing, the counting sort, the grouped
expert GEMMs and the combine + norm (csrc/moe.hip), the model forward and the
engine through captured decode graphs.

Oracle: the plain-loop fp32 reference in ops.reference, run on the CPU."""

import copy
import dataclasses

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
PATTERNS = ["random", "one_expert", "one_unused", "bm_and_bm_plus_1"]
# the GPU attention kernels cover head_dim 128 only
TINY_MOE = ModelConfig(
    name="tiny-mixtral-hd128", hidden_size=256, intermediate_size=512,
    num_layers=2, num_heads=2, num_kv_heads=1, vocab_size=512, head_dim=128,
    rope_theta=10000.0, max_positions=512, num_experts=4, experts_per_token=2,
)


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), "the HIP extension must be loaded on a GPU box"


def _guarded(shape, dtype, fill=None):
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.empty(numel + 2 * PAD, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(CANARY)
    view = buf[PAD : PAD + numel].view(shape)
    if fill is not None:
        view.copy_(fill)

    def check(name):
        torch.cuda.synchronize()
        for part in (buf[:PAD], buf[PAD + numel :]):
            assert bool((part.view(torch.uint8) == CANARY).all()), f"{name}: guard clobbered"

    return view, check


def _ids(pattern, T, k, E, bm, seed=0):
    """ids [T, k] int32 (CPU) of an assignment pattern; rows need not hold
    distinct experts for the sort and the GEMMs."""
    g = torch.Generator().manual_seed(seed)
    P = T * k
    if pattern == "one_expert":
        flat = torch.full((P,), E - 1)
    elif pattern == "one_unused":
        flat = torch.randint(0, E - 1, (P,), generator=g) + 1  # expert 0 idle
    elif pattern == "bm_and_bm_plus_1":  # expert 0: BM pairs, expert 1: BM + 1
        flat = torch.randint(2, E, (P,), generator=g)
        flat[:bm], flat[bm : 2 * bm + 1] = 0, 1
    else:
        flat = torch.randint(0, E, (P,), generator=g)
    return flat.to(torch.int32).view(T, k)


def _tri(shape, g):
    return (torch.randint(0, 3, shape, generator=g) - 1).bfloat16()


@pytest.mark.parametrize("T", [1, 17, 200])
@pytest.mark.parametrize("E,k", [(2, 1), (2, 2), (8, 1), (8, 2), (8, 8), (64, 1), (64, 2), (64, 8)])
@pytest.mark.parametrize("H", [64, 448])
def test_route_exact(H, E, k, T):
    """Integer data: every logit is an exact fp32 integer in any summation
    order, with many ties, so ids pin the lower-index rule exactly."""
    g = torch.Generator().manual_seed(H + E + k + T)
    x, w = _tri((T, H), g), _tri((E, H), g)
    ref_ids, ref_w = reference.moe_route(x, w, k)
    ids, wts = ops.moe_route(x.to(DEV), w.to(DEV), k)
    assert torch.equal(ids.cpu(), ref_ids)
    assert (wts.cpu() - ref_w).abs().max().item() <= 1e-5
    assert (wts.cpu().sum(-1) - 1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("mf", [1, 2, 4])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_align(pattern, mf):
    T, k, E, bm = 200, 2, 8, 16 * mf
    ids = _ids(pattern, T, k, E, bm)
    cap = ops.moe_cap(T * k, E, mf)
    sp, chk_s = _guarded((cap,), torch.int32)
    te, chk_t = _guarded((cap // bm,), torch.int32)
    ops._native().moe_align(sp, te, ids.to(DEV), E, mf)
    chk_s("sorted_pairs")
    chk_t("tile_expert")
    sp, te, flat = sp.cpu(), te.cpu(), ids.view(-1)
    real = sp[sp >= 0]
    assert torch.equal(real.sort().values, torch.arange(T * k, dtype=torch.int32))
    assert bool((sp[sp < 0] == -1).all())
    for t, e in enumerate(te.tolist()):
        rows = sp[t * bm : (t + 1) * bm]
        if e < 0:
            assert bool((rows == -1).all())
        else:
            assert rows[0] >= 0 and bool((flat[rows[rows >= 0].long()] == e).all())
    if pattern == "bm_and_bm_plus_1":
        assert te.tolist()[:3] == [0, 1, 1] and sp[3 * bm - 1] == -1 and sp[2 * bm] >= 0


@pytest.mark.parametrize("T", [1, 17, 200])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_down_exact(pattern, T):
    """Integer act / w_down and routing weights in {0.5, 1, 2}, I = 64: all
    products, sums and the one rounding are exact, so y_pair is bit-equal.
    Rows of act that hold no pair carry a NaN canary."""
    k, E, H, inter = 2, 4, 128, 64
    mf = ops._native().moe_pick_mf(T, k, E)
    g = torch.Generator().manual_seed(T)
    ids = _ids(pattern, T, k, E, 16 * mf)
    act, w_down = _tri((T * k, inter), g), _tri((E, H, inter), g)
    wts = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T, k), generator=g)]
    ref = reference.moe_down(act, ids, wts, w_down)

    plan = ops.moe_align(ids.to(DEV), E, mf)
    sp = plan.sorted_pairs.cpu().long()
    act_sorted = torch.full((plan.cap, inter), float("nan")).bfloat16()
    act_sorted[sp >= 0] = act[sp[sp >= 0]]
    y, chk = _guarded((T * k, H), torch.bfloat16)  # the kernel scatters into it
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


def _mlp_gpu(x, res, w_gu, w_dn, norm_w, ids, wts, k):
    d = lambda t: t.to(DEV)
    normed, r = ops.moe_mlp(
        d(x), None, ops.moe_pack_weights(d(w_gu), True),
        ops.moe_pack_weights(d(w_dn), False), k, d(res).clone(), d(norm_w), 1e-5,
        ids=d(ids), weights=d(wts),
    )
    return normed.cpu(), r.cpu()


@pytest.mark.parametrize("T", [1, 17, 200])
@pytest.mark.parametrize("H,inter", [(256, 192), (4096, 448)])
@pytest.mark.parametrize("E", [4, 8])
def test_mlp_numerics(E, H, inter, T):
    """Random data, ids and weights given (no router, so no near-tie can
    flip a case): normalised max error against the fp32 reference < 0.02."""
    k = 2
    x, res, w_gu, w_dn, norm_w, ids, wts = _mlp_case(T, H, inter, E, k, T + E)
    ref_n, ref_r = ops.moe_mlp(x, None, w_gu, w_dn, k, res.clone(), norm_w, 1e-5,
                               ids=ids, weights=wts)
    got_n, got_r = _mlp_gpu(x, res, w_gu, w_dn, norm_w, ids, wts, k)
    errs = [
        ((g.float() - r.float()).abs().max() / (r.float().abs().max() + 1e-3)).item()
        for g, r in ((got_n, ref_n), (got_r, ref_r))
    ]
    # the swiglu epilogue on its own, written into a guarded act [cap, I]:
    # real rows against the reference, padding rows left as they were
    plan = ops.moe_align(ids.to(DEV), E)
    act, chk = _guarded((plan.cap, inter), torch.bfloat16)
    ops.moe_gate_up_swiglu(x.to(DEV), ids.to(DEV),
                           ops.moe_pack_weights(w_gu.to(DEV), True), plan, out=act)
    chk("act")
    sp, act = plan.sorted_pairs.cpu().long(), act.cpu()
    ref_a = reference.moe_gate_up_swiglu(x, ids, w_gu).float()
    errs.append(((act[sp >= 0].float() - ref_a[sp[sp >= 0]]).abs().max()
                 / (ref_a.abs().max() + 1e-3)).item())
    assert bool((act[sp < 0].view(torch.uint8) == CANARY).all())
    print(f"T={T} H={H} I={inter} E={E}: normed err {errs[0]:.5f} residual err "
          f"{errs[1]:.5f} act err {errs[2]:.5f}")
    assert max(errs) < 0.02


def test_mlp_sensitivity():
    T, H, inter, E, k = 17, 256, 192, 4, 2
    x, res, w_gu, w_dn, norm_w, ids, wts = _mlp_case(T, H, inter, E, k, 3)
    base = _mlp_gpu(x, res, w_gu, w_dn, norm_w, ids, wts, k)[1]
    # another expert for one pair: row 5 changes and no other row
    ids2 = ids.clone()
    ids2[5, 1] = next(e for e in range(E) if e not in ids[5].tolist())
    got = _mlp_gpu(x, res, w_gu, w_dn, norm_w, ids2, wts, k)[1]
    changed = (got != base).any(dim=1)
    assert changed.tolist() == [t == 5 for t in range(T)]
    # one element of w_down[2]: exactly the rows routed to expert 2 change
    w2 = w_dn.clone()
    w2[2, 7, 11] += 4.0
    got = _mlp_gpu(x, res, w_gu, w2, norm_w, ids, wts, k)[1]
    assert torch.equal((got != base).any(dim=1), (ids == 2).any(dim=1))
    assert bool((got != base)[:, [c for c in range(H) if c != 7]].sum() == 0)


def _decode_logits(model, rows=17):
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    dev = model.device
    kv = PagedKVCache(model.config, rows, 16, dev, torch.bfloat16)
    toks = torch.randint(0, model.config.vocab_size, (rows,),
                         generator=torch.Generator().manual_seed(5))
    batch = ForwardBatch(
        kind="decode", token_ids=toks.to(dev),
        positions=torch.zeros(rows, dtype=torch.long, device=dev),
        slot_mapping=(torch.arange(rows) * 16).to(dev),
        block_tables=torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1),
        context_lens=torch.ones(rows, dtype=torch.int32, device=dev),
    )
    return model.forward(batch, kv.k_caches, kv.v_caches).float().cpu()


def test_model_forward_all_experts():
    """k = E = 4: no selection, so no routing flip. GPU-vs-CPU max logit
    error of the MoE model within 2x that of the dense model of the same
    shapes (one more bf16 rounding per pair output, and the k-term sum)."""
    errs = {}
    for name, cfg in (
        ("dense", dataclasses.replace(TINY_MOE, num_experts=0, experts_per_token=0)),
        ("moe", dataclasses.replace(TINY_MOE, experts_per_token=4)),
    ):
        model = LlamaModel(cfg, device=DEV, seed=0)
        twin = copy.copy(model)
        twin.device = torch.device("cpu")
        for attr in ("embed", "lm_head", "final_norm", "cos_sin"):
            setattr(twin, attr, getattr(model, attr).cpu())
        twin.layers = [
            {
                key: (ops.moe_unpack_weights(v, key == "experts_gate_up")
                      if key.startswith("experts_") else v).cpu()
                for key, v in layer.items() if not key.endswith(("_swz", "_int"))
            }
            for layer in model.layers
        ]
        errs[name] = (_decode_logits(model) - _decode_logits(twin)).abs().max().item()
    print(f"gpu-vs-cpu max logit error: dense {errs['dense']:.5f}, moe {errs['moe']:.5f} "
          f"(ratio {errs['moe'] / errs['dense']:.3f})")
    assert errs["dense"] > 0
    assert errs["moe"] <= 2 * errs["dense"]


def _engine(use_hipgraph, **kw):
    from llmapigateway_amd.engine import LLMEngine

    kw = {"model": TINY_MOE, "tp_size": 1, **kw}
    return LLMEngine(
        device=DEV, dtype=torch.bfloat16, block_size=16, num_blocks=64,
        max_model_len=256, max_batch_size=4, seed=0, use_hipgraph=use_hipgraph,
        admit_min_batch=1, **kw,
    )


def test_engine_graph_equals_eager_and_repeats():
    from llmapigateway_amd.engine import EngineRequest, SamplingParams

    outs = []
    for graph in (True, False):
        eng = _engine(graph)
        for _ in range(2):  # the second, identical run replays the graphs
            reqs = [
                eng.add_request(EngineRequest(
                    list(range(3 + i, 35 + i)),
                    SamplingParams(max_tokens=17, ignore_eos=True)))
                for i in range(4)
            ]
            while eng.has_work():
                eng.step()
            eng.step()  # deliver the deferred last tokens
            assert all(r.state == "finished" and len(r.out_ids) == 17 for r in reqs)
            outs.append([r.out_ids for r in reqs])
        if graph:
            assert eng.stats["graph_steps"] >= 32
    assert outs[0] == outs[1] == outs[2] == outs[3]


@pytest.mark.parametrize("kw", [{"weight_dtype": "fp8"}, {"max_loras": 1}, {"tp_size": 2}])
def test_engine_rejects_unsupported(kw):
    with pytest.raises(NotImplementedError):
        _engine(False, **kw)
