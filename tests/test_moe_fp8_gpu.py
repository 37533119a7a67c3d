"""fp8 expert weights on the GPU (csrc/moe_w8.hip): the W8A16 grouped GEMM
against the bf16 grouped GEMM on the dequantised weights (bit identity) and
the fp32 reference, the model forward, the engine through captured graphs."""

import dataclasses
import functools

import pytest
import torch
from test_moe_mxfp4_cpu import TINY as TINY_MOE  # H 256 / I 512, head_dim 128
from test_moe_mxfp4_cpu import decode_logits
from test_moe_mxfp4_gpu import PATTERNS, _guarded, _ids

from llmapigateway_amd import ops
from llmapigateway_amd.models.llama import LlamaModel
from llmapigateway_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV, CANARY = "cuda:0", 0x5A
E, TOPK = 4, 2


def _quantize(w):
    """[E, N, K] -> (bits, scale, dequantised bf16), expert by expert."""
    qs = [ops.fp8_quantize_weight(w[e]) for e in range(w.shape[0])]
    q, s = torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs])
    return q, s, reference.moe_dequantize_experts_fp8(q, s)


def _pack(q, s, gate_up):
    return ops.moe_pack_weights_fp8(q.to(DEV), s.to(DEV), gate_up)


@functools.lru_cache(maxsize=None)
def _panels(N, K, gate_up):
    """Rows of magnitude 2^j, j in -6..3, times N(0, 0.05): many channel scales."""
    g = torch.Generator().manual_seed(N * 7 + K)
    mag = torch.exp2(torch.randint(-6, 4, (E, N, 1), generator=g).float())
    q, s, wd = _quantize((mag * torch.randn(E, N, K, generator=g) * 0.05).bfloat16())
    assert s.unique().numel() >= 8
    return (*_pack(q, s, gate_up), ops.moe_pack_weights(wd.to(DEV), gate_up))


# mf None: from moe_pick_mf (1, 1 and 4 for these T); (17, 2) adds BM = 32
@pytest.mark.parametrize("T,mf", [(1, None), (17, None), (200, None), (17, 2)])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("gi", range(4))
@pytest.mark.parametrize("nb", [1, 3])
def test_bit_identical_to_bf16_kernel(nb, gi, pattern, T, mf):
    """Exact conversion, moe_gemm_kernel's MFMA inputs and order, power-of-two
    channel scales: both epilogues equal that kernel on the dequantised
    weights bit for bit. K: 1, D - 1, D + 1 and 2D + 1 groups of 64 (D = the
    ring depth); N: one and three column blocks (128 gate_up, 64 down)."""
    mf = mf or ops._native().moe_pick_mf(T, TOPK, E)
    depth = ops.MOE_W8_RING_DEPTH
    K = [1, depth - 1, depth + 1, 2 * depth + 1][gi] * 64
    g = torch.Generator().manual_seed(T + K)
    ids = _ids(pattern, T, 16 * mf).to(DEV)
    wts = (torch.rand(T, TOPK, generator=g) + 0.1).to(DEV)
    plan = ops.moe_align(ids, E, mf)
    real = plan.sorted_pairs >= 0
    q8, s8, wbf = _panels(nb * 128, K, True)
    x = torch.randn(T, K, generator=g).bfloat16().to(DEV)
    act, chk = _guarded(plan.cap, nb * 64)
    ops.moe_gate_up_swiglu(x, ids, q8, plan, out=act, s_gate_up=s8)
    chk("act")
    assert torch.equal(act[real], ops.moe_gate_up_swiglu(x, ids, wbf, plan)[real])
    assert bool((act[~real].view(torch.uint8) == CANARY).all())  # padding rows

    q8, s8, wbf = _panels(nb * 64, K, False)
    a = torch.randn(plan.cap, K, generator=g).bfloat16().to(DEV)
    y, chk = _guarded(T * TOPK, nb * 64)
    ops.moe_down(a, ids, wts, q8, plan, out=y, s_down=s8)
    chk("y_pair")
    assert torch.equal(y, ops.moe_down(a, ids, wts, wbf, plan))


@pytest.mark.parametrize("T", [1, 17, 200])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_down_exact(pattern, T):
    """Ternary act, ternary weights times a power of two 2^-3..2^3 per row,
    routing weights in {0.5, 1, 2}, K = one group: everything is exact, so
    y_pair is bit-equal to the fp32 reference. Unused act rows carry NaN."""
    H, K = 128, 64
    mf = ops._native().moe_pick_mf(T, TOPK, E)
    g = torch.Generator().manual_seed(T)
    tri = lambda *shape: (torch.randint(0, 3, shape, generator=g) - 1).float()
    ids, act = _ids(pattern, T, 16 * mf), tri(T * TOPK, K).bfloat16()
    exps = torch.randint(-3, 4, (E, H, 1), generator=g).float()
    w = (tri(E, H, K) * torch.exp2(exps)).bfloat16()
    q, s, wd = _quantize(w)
    assert torch.equal(wd, w) and s.unique().numel() >= 7
    wts = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T, TOPK), generator=g)]
    plan = ops.moe_align(ids.to(DEV), E, mf)
    sp = plan.sorted_pairs.cpu().long()
    act_sorted = torch.full((plan.cap, K), float("nan")).bfloat16()
    act_sorted[sp >= 0] = act[sp[sp >= 0]]
    y, chk = _guarded(T * TOPK, H)
    q8, s8 = _pack(q, s, False)
    ops.moe_down(act_sorted.to(DEV), ids.to(DEV), wts.to(DEV), q8, plan, out=y, s_down=s8)
    chk("y_pair")
    assert torch.equal(y.cpu(), reference.moe_down(act, ids, wts, wd))


def test_mlp_sensitivity():
    """One byte of expert 2's down panel, one scale of expert 1's gate_up
    panel: exactly the rows routed to that expert change."""
    T, H, inter = 17, 256, 384
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, H, generator=g).bfloat16()
    w_gu = (torch.randn(E, 2 * inter, H, generator=g) * 0.05).bfloat16()
    w_dn = (torch.randn(E, H, inter, generator=g) * 0.05).bfloat16()
    ids = torch.stack([torch.randperm(E, generator=g)[:TOPK] for _ in range(T)]).to(torch.int32)
    gq, gs, gd = _quantize(w_gu)
    # row 7 of expert 2's down is one weight, at the k where the smallest
    # |act| of the rows routed there is largest: far above a bf16 ulp
    act = reference.moe_gate_up_swiglu(x, ids, gd).float()[(ids == 2).view(-1)]
    kcol = int(act.abs().min(dim=0).values.argmax())
    w_dn[2, 7] = 0
    w_dn[2, 7, kcol] = 16.0
    dq, ds, _ = _quantize(w_dn)

    def run(gq, gs, dq, ds):
        (g8, gs8), (d8, ds8) = _pack(gq, gs, True), _pack(dq, ds, False)
        return ops.moe_mlp(
            x.to(DEV), None, g8, d8, TOPK, torch.zeros(T, H, dtype=torch.bfloat16, device=DEV),
            torch.ones(H, dtype=torch.bfloat16, device=DEV), 1e-5, ids=ids.to(DEV),
            weights=torch.full((T, TOPK), 0.5, device=DEV), s_gate_up=gs8, s_down=ds8,
        )[1].cpu()

    base = run(gq, gs, dq, ds)
    q2, s2 = ops.moe_unpack_weights_fp8(*ops.moe_pack_weights_fp8(dq, ds, False), False)
    assert q2[2, 7, kcol] == 0x78  # 256 = 16 / scale
    q2[2, 7, kcol] ^= 0x40  # exponent bit: 256 -> 1
    diff = run(gq, gs, q2, s2) != base
    assert torch.equal(diff.any(dim=1), (ids == 2).any(dim=1))
    assert not bool(diff[:, [c for c in range(H) if c != 7]].any())
    gs2 = gs.clone()
    gs2[1, 40] *= 2
    assert torch.equal((run(gq, gs2, dq, ds) != base).any(dim=1), (ids == 1).any(dim=1))


def test_model_forward_all_experts():
    """k = E = 4, so no routing flip: GPU-vs-CPU max logit error with fp8
    experts within 2x that of the dense bf16 model of the same shapes."""
    errs = {}
    for name, cfg, kw in (
        ("dense", dataclasses.replace(TINY_MOE, num_experts=0, experts_per_token=0), {}),
        ("moe", dataclasses.replace(TINY_MOE, experts_per_token=4), {"expert_dtype": "fp8"}),
    ):
        gpu, cpu = (LlamaModel(cfg, device=d, seed=0, **kw) for d in (DEV, "cpu"))
        errs[name] = (decode_logits(gpu, 17).cpu() - decode_logits(cpu, 17)).abs().max().item()
    print(f"gpu-vs-cpu max logit error: dense bf16 {errs['dense']:.5f}, moe with fp8 "
          f"experts {errs['moe']:.5f} (ratio {errs['moe'] / errs['dense']:.3f})")
    assert errs["dense"] > 0
    assert errs["moe"] <= 2 * errs["dense"]


def test_engine_graph_equals_eager_and_repeats():
    from llmapigateway_amd.engine import EngineRequest, LLMEngine, SamplingParams

    outs = []
    for graph in (True, False):
        eng = LLMEngine(
            model=TINY_MOE, tp_size=1, expert_dtype="fp8", device=DEV,
            dtype=torch.bfloat16, block_size=16, num_blocks=64, max_model_len=256,
            max_batch_size=4, seed=0, use_hipgraph=graph, admit_min_batch=1,
        )
        assert "experts_down_q8" in eng.model.layers[0]
        for _ in range(2):  # the second, identical run replays the graphs
            sp = SamplingParams(max_tokens=17, ignore_eos=True)
            reqs = [eng.add_request(EngineRequest(list(range(3 + i, 35 + i)), sp)) for i in range(4)]
            while eng.has_work():
                eng.step()
            eng.step()  # deliver the deferred last tokens
            assert all(r.state == "finished" and len(r.out_ids) == 17 for r in reqs)
            outs.append([r.out_ids for r in reqs])
        assert not graph or eng.stats["graph_steps"] >= 32
    assert outs[0] == outs[1] == outs[2] == outs[3]
