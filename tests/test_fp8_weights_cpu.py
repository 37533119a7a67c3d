"""fp8 (e4m3) weight quantisation: the scheme (ops.reference), its fragment
layout, TP sharding, the fp8 model / engine on the CPU reference path and
the config knob."""

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.engine import LLMEngine, SamplingParams
from llmapigateway_amd.models.configs import get_model_config
from llmapigateway_amd.models.llama import LlamaModel
from llmapigateway_amd.parallel.tp import shard_gate_up, shard_qkv, shard_row

PROJ = ("qkv", "o", "gate_up", "down")


def _weight(N=192, K=448, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g) * 0.02


# ---------- quantiser ----------

def test_scales_are_powers_of_two_and_minimal():
    w = _weight()
    q, s = ops.fp8_quantize_weight(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape
    assert s.dtype == torch.float32 and s.shape == (w.shape[0],)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all()), "scales must be powers of two"
    amax = w.abs().amax(dim=-1)
    assert bool((amax / s <= 448).all())
    assert bool((amax / (s / 2) > 448).all()), "not the smallest such power"


def test_quantised_range_and_no_nan():
    w = _weight()
    w[5, 7] = 3.0  # an outlier row
    q, _ = ops.fp8_quantize_weight(w)
    assert not bool(((q & 0x7F) == 0x7F).any()), "e4m3fn NaN encoding produced"
    assert bool((q.view(torch.float8_e4m3fn).float().abs() <= 448).all())


def test_exact_power_of_two_amax():
    # amax/448 exactly a power of two: scale is that power, q hits 448
    w = torch.zeros(64, 64)
    w[:, 0] = 448.0 * 2.0 ** -9
    w[1, 0] = -448.0 * 2.0 ** 3
    q, s = ops.fp8_quantize_weight(w)
    assert s[0].item() == 2.0 ** -9 and s[1].item() == 2.0 ** 3
    assert q.view(torch.float8_e4m3fn).float()[0, 0].item() == 448.0
    assert q.view(torch.float8_e4m3fn).float()[1, 0].item() == -448.0


def test_zero_row_scale_is_one():
    w = _weight()
    w[3] = 0
    q, s = ops.fp8_quantize_weight(w)
    assert s[3].item() == 1.0
    assert bool((q[3] == 0).all())


def test_dequant_exact_in_bf16():
    q, s = ops.fp8_quantize_weight(_weight())
    d = ops.fp8_dequantize_weight(q, s, torch.float32)
    assert torch.equal(d.bfloat16().float(), d)
    assert torch.equal(ops.fp8_dequantize_weight(q, s, torch.bfloat16).float(), d)


def test_round_trip_error_half_ulp():
    w = _weight(256, 512, seed=1)
    q, s = ops.fp8_quantize_weight(w)
    d = ops.fp8_dequantize_weight(q, s, torch.float32)
    normal = q.view(torch.float8_e4m3fn).float().abs() >= 2.0 ** -6
    assert normal.float().mean() > 0.9
    rel = ((d - w).abs() / w.abs())[normal]
    print(f"max round-trip relative error on normals: {rel.max().item():.5f}")
    assert rel.max().item() <= 2.0 ** -4


def test_bf16_input_quantises_like_its_float_value():
    w = _weight().bfloat16()
    q1, s1 = ops.fp8_quantize_weight(w)
    q2, s2 = ops.fp8_quantize_weight(w.float())
    assert torch.equal(q1, q2) and torch.equal(s1, s2)


# ---------- swizzle ----------

@pytest.mark.parametrize("N,K", [(64, 64), (192, 448)])
def test_swizzle_inverse_identity(N, K):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    f = ops.swizzle_weight_frag_fp8(q)
    assert f.shape == (K // 64, N // 16, 64, 16) and f.is_contiguous()
    assert torch.equal(ops.unswizzle_weight_frag_fp8(f), q)
    # the documented layout, spot-checked element by element
    for _ in range(500):
        k64, n16, lane, j = (
            int(torch.randint(0, hi, (1,), generator=g))
            for hi in (K // 64, N // 16, 64, 16)
        )
        n = n16 * 16 + (lane & 15)
        k = k64 * 64 + (j >> 3) * 32 + (lane >> 4) * 8 + (j & 7)
        assert f[k64, n16, lane, j] == q[n, k]


def test_swizzle_rejects_odd_shapes():
    with pytest.raises(AssertionError):
        ops.swizzle_weight_frag_fp8(torch.zeros(48, 64, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        ops.swizzle_weight_frag_fp8(torch.zeros(64, 96, dtype=torch.uint8))


def test_linear_w8_reference_and_op():
    w = _weight()
    q, s = ops.fp8_quantize_weight(w)
    x = torch.randn(5, w.shape[1], generator=torch.Generator().manual_seed(2))
    ref = x @ ops.fp8_dequantize_weight(q, s, torch.float32).T
    assert torch.equal(ops.reference.linear_w8(x, q, s), ref)
    assert torch.equal(ops.linear_w8(x, ops.swizzle_weight_frag_fp8(q), s), ref)
    xb = x.bfloat16()
    assert ops.linear_w8(xb, ops.swizzle_weight_frag_fp8(q), s).dtype == torch.bfloat16


# ---------- sharding: quantise the full matrix, then shard bits and scales ----------

def test_sharded_dequant_equals_shard_of_dequant():
    tp = 2
    q_size, kv_size, inter, hidden = 256, 128, 512, 256
    cases = {
        "qkv": (
            _weight(q_size + 2 * kv_size, hidden, 3),
            lambda t, r: shard_qkv(t, r, tp, q_size, kv_size),
            True,
        ),
        "gate_up": (
            _weight(2 * inter, hidden, 4),
            lambda t, r: shard_gate_up(t, r, tp, inter),
            True,
        ),
        "row": (_weight(hidden, inter, 5), lambda t, r: shard_row(t, r, tp), False),
    }
    for name, (w, shard, column) in cases.items():
        q, s = ops.fp8_quantize_weight(w)
        full = ops.fp8_dequantize_weight(q, s, torch.float32)
        for rank in range(tp):
            qs = shard(q, rank)
            ss = shard(s, rank) if column else s
            got = ops.fp8_dequantize_weight(qs, ss, torch.float32)
            assert torch.equal(got, shard(full, rank)), (name, rank)


def test_tp_model_is_a_sharding_of_the_tp1_model():
    cfg = get_model_config("tiny-llama")
    full = LlamaModel(cfg, dtype=torch.float32, seed=3, weight_dtype="fp8")
    part = LlamaModel(
        cfg.scaled_for_tp(2), dtype=torch.float32, seed=3, weight_dtype="fp8",
        tp_rank=1, tp_size=2, full_config=cfg,
    )

    def deq(layer, name):
        return ops.fp8_dequantize_weight(
            ops.unswizzle_weight_frag_fp8(layer[name + "_q8"]),
            layer[name + "_s8"], torch.float32,
        )

    lf, lp = full.layers[0], part.layers[0]
    assert torch.equal(deq(lp, "o"), shard_row(deq(lf, "o"), 1, 2))
    assert torch.equal(deq(lp, "down"), shard_row(deq(lf, "down"), 1, 2))
    assert torch.equal(
        deq(lp, "qkv"), shard_qkv(deq(lf, "qkv"), 1, 2, cfg.q_size, cfg.kv_size)
    )
    assert torch.equal(
        deq(lp, "gate_up"),
        shard_gate_up(deq(lf, "gate_up"), 1, 2, cfg.intermediate_size),
    )


# ---------- model / engine ----------

def _engine(**kw):
    return LLMEngine(
        model="tiny-llama", device="cpu", dtype=torch.float32, block_size=16,
        num_blocks=64, seed=7, **kw,
    )


def _greedy(eng):
    req = eng.generate(
        list(range(3, 20)), SamplingParams(max_tokens=16, ignore_eos=True)
    )
    assert req.state == "finished" and len(req.out_ids) == 16
    return req.out_ids


def test_engine_fp8_matches_fake_quant_and_is_deterministic():
    fp8 = _greedy(_engine(weight_dtype="fp8"))
    sim_eng = _engine()
    sim_eng.model.quantize_weights_(simulate=True)
    assert fp8 == _greedy(sim_eng)
    assert fp8 == _greedy(_engine(weight_dtype="fp8"))


def test_fp8_model_layout_and_bytes():
    cfg = get_model_config("tiny-llama")
    bf16 = LlamaModel(cfg, dtype=torch.bfloat16, seed=0)
    fp8 = LlamaModel(cfg, dtype=torch.bfloat16, seed=0, weight_dtype="fp8")
    proj_bf16 = proj_fp8 = scales = 0
    for lb, lq in zip(bf16.layers, fp8.layers):
        for name in PROJ:
            assert name not in lq and name + "_swz" not in lq
            q8, s8 = lq[name + "_q8"], lq[name + "_s8"]
            assert q8.dtype == torch.uint8 and s8.dtype == torch.float32
            assert q8.numel() == lb[name].numel() and s8.numel() == lb[name].shape[0]
            proj_bf16 += lb[name].numel() * lb[name].element_size()
            proj_fp8 += q8.numel() * q8.element_size()
            scales += s8.numel() * s8.element_size()
    assert proj_fp8 * 2 == proj_bf16
    # per-tensor accounting: everything else is unchanged
    assert fp8.param_bytes() == bf16.param_bytes() - proj_bf16 + proj_fp8 + scales
    # embeddings, lm_head and norms stay in the model dtype
    assert fp8.embed.dtype == fp8.lm_head.dtype == torch.bfloat16
    assert fp8.layers[0]["input_norm"].dtype == torch.bfloat16


def test_quantize_weights_in_place_equals_constructor():
    cfg = get_model_config("tiny-llama")
    a = LlamaModel(cfg, dtype=torch.float32, seed=1, weight_dtype="fp8")
    b = LlamaModel(cfg, dtype=torch.float32, seed=1).quantize_weights_("fp8")
    assert b.weight_dtype == "fp8"
    for la, lb in zip(a.layers, b.layers):
        assert la.keys() == lb.keys()
        for k in la:
            assert torch.equal(la[k], lb[k]), k
    with pytest.raises(RuntimeError):
        b.quantize_weights_("fp8")
    with pytest.raises(ValueError):
        LlamaModel(cfg, dtype=torch.float32, seed=1).quantize_weights_("int4")
    with pytest.raises(ValueError):
        LlamaModel(cfg, dtype=torch.float32, weight_dtype="fp4")


def test_simulate_keeps_auto_layout():
    cfg = get_model_config("tiny-llama")
    m = LlamaModel(cfg, dtype=torch.float32, seed=1).quantize_weights_(simulate=True)
    assert m.weight_dtype == "auto"
    ref = LlamaModel(cfg, dtype=torch.float32, seed=1, weight_dtype="fp8")
    for lm, lr in zip(m.layers, ref.layers):
        for name in PROJ:
            want = ops.fp8_dequantize_weight(
                ops.unswizzle_weight_frag_fp8(lr[name + "_q8"]),
                lr[name + "_s8"], torch.float32,
            )
            assert torch.equal(lm[name], want)


def test_env_fallback(monkeypatch):
    monkeypatch.setenv("LLMAPI_WEIGHT_DTYPE", "fp8")
    eng = _engine()
    assert eng.weight_dtype == "fp8" and eng.model.weight_dtype == "fp8"
    monkeypatch.delenv("LLMAPI_WEIGHT_DTYPE")
    assert _engine().weight_dtype == "auto"


# ---------- config ----------

def test_local_url_weight_dtype_and_engine_key():
    from llmapigateway_amd.config.loader import EngineSpec, ProviderDetails
    from llmapigateway_amd.engine.registry import EngineRegistry

    spec = ProviderDetails(baseUrl="local://llama-3-8b?weight_dtype=fp8").engine_spec()
    assert spec.model == "llama-3-8b" and spec.weight_dtype == "fp8"
    default = ProviderDetails(baseUrl="local://llama-3-8b").engine_spec()
    assert default.weight_dtype == "auto" and EngineSpec().weight_dtype == "auto"
    reg = EngineRegistry()
    assert reg._engine_key(spec) != reg._engine_key(default)
    explicit = ProviderDetails(
        baseUrl="local://", engine={"model": "llama-3-8b", "weight_dtype": "fp8"}
    ).engine_spec()
    assert reg._engine_key(explicit) == reg._engine_key(spec)


def test_engine_stats_report_weight_dtype():
    from llmapigateway_amd.config.loader import EngineSpec
    from llmapigateway_amd.engine.registry import EngineRegistry

    reg = EngineRegistry()
    try:
        reg.get_engine(EngineSpec(model="tiny-llama", weight_dtype="fp8"))
        rows = reg.stats()
        assert rows and rows[0]["weight_dtype"] == "fp8"
    finally:
        import asyncio

        asyncio.run(reg.aclose())
