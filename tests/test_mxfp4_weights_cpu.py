"""MXFP4 (e2m1 elements, e8m0 block-32 scales) weight quantisation: the
scheme (ops.reference), its fragment layout, TP sharding, the mxfp4 model /
engine on the CPU reference path and the config knob."""

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.engine import LLMEngine, SamplingParams
from llmapigateway_amd.models.configs import get_model_config
from llmapigateway_amd.models.llama import LlamaModel
from llmapigateway_amd.parallel.tp import shard_gate_up, shard_qkv, shard_row

PROJ = ("qkv", "o", "gate_up", "down")
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _weight(N=192, K=448, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g) * 0.02


def _scale_f32(s):
    return torch.ldexp(torch.ones(s.shape), s.to(torch.int32) - 127)


# ---------- quantiser ----------

def test_shapes_and_scale_bytes_minimal():
    w = _weight()
    w[0, :32] *= 2.0 ** -140  # a block far below the e8m0 range
    w[1, :32] *= 2.0 ** 100
    q, s = ops.mxfp4_quantize_weight(w)
    N, K = w.shape
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2)
    assert s.dtype == torch.uint8 and s.shape == (N, K // 32)
    assert int(s.min()) >= 1 and int(s.max()) <= 254
    assert int(s[0, 0]) == 1, "exponent clamps at -126"
    amax = w.view(N, K // 32, 32).abs().amax(dim=-1)
    sf = _scale_f32(s)
    assert bool((amax / sf <= 6).all()), "a block clips"
    free = s > 1  # the lower clamp is the one case where s is not minimal
    assert bool((amax / (sf / 2) > 6)[free].all()), "not the smallest such power"


def test_exact_power_of_two_boundary():
    # amax exactly 6 * 2^t: the scale is 2^t and the element code is 6
    w = torch.zeros(64, 64)
    w[0, 0] = 6.0 * 2.0 ** -9
    w[0, 33] = -6.0 * 2.0 ** 3
    w[1, 0] = 6.0 * 2.0 ** -9 * (1 + 2.0 ** -20)  # just above: next power
    q, s = ops.mxfp4_quantize_weight(w)
    assert s[0].tolist() == [127 - 9, 127 + 3] and int(s[1, 0]) == 127 - 8
    assert int(q[0, 0]) == 0x07 and int(q[0, 16]) == 0xF0


def test_zero_block_scale_byte_is_127():
    w = _weight()
    w[3, 64:96] = 0
    q, s = ops.mxfp4_quantize_weight(w)
    assert int(s[3, 2]) == 127
    assert bool((q[3, 32:48] == 0).all())


def test_packing_even_k_in_low_nibble():
    w = torch.zeros(64, 64)
    w[0, 0], w[0, 1], w[0, 2], w[0, 3] = 6.0, -1.0, 0.5, 3.0
    q, s = ops.mxfp4_quantize_weight(w)
    assert int(s[0, 0]) == 127
    assert int(q[0, 0]) == (0x7 | (0xA << 4))
    assert int(q[0, 1]) == (0x1 | (0x5 << 4))


def test_rounds_to_nearest_even_code():
    # one block with amax 6 (scale 1): ties go to the code with mantissa 0
    vals = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.26, 0.74, 2.49, 4.99, 5.01]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.5, 0.5, 2.0, 4.0, 6.0]
    w = torch.zeros(64, 64)
    w[0, : len(vals)] = torch.tensor(vals)
    w[1, : len(vals)] = -torch.tensor(vals)
    d = ops.mxfp4_dequantize_weight(*ops.mxfp4_quantize_weight(w), torch.float32)
    assert d[0, : len(vals)].tolist() == want
    assert d[1, : len(vals)].tolist() == [-v for v in want]


def test_dequant_exact_in_bf16():
    w = _weight()
    w[0, :32] *= 2.0 ** -140
    q, s = ops.mxfp4_quantize_weight(w)
    d = ops.mxfp4_dequantize_weight(q, s, torch.float32)
    assert torch.equal(d.bfloat16().float(), d)
    assert torch.equal(ops.mxfp4_dequantize_weight(q, s, torch.bfloat16).float(), d)
    assert ops.mxfp4_dequantize_weight(q, s).dtype == torch.bfloat16


def test_round_trip_error_half_grid_step():
    w = _weight(256, 512, seed=1)
    q, s = ops.mxfp4_quantize_weight(w)
    d = ops.mxfp4_dequantize_weight(q, s, torch.float32)
    sf = _scale_f32(s).repeat_interleave(32, dim=1)
    a = (w / sf).abs()  # in units of the block scale: the e2m1 grid
    assert float(a.max()) <= 6
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
    err = (d - w).abs() / sf
    print(f"max round-trip error in grid steps: {(err / step).max().item():.4f}")
    assert bool((err <= step / 2).all())
    # and every dequantised magnitude is a grid point
    assert bool(torch.isin((d / sf).abs(), GRID).all())


def test_outlier_touches_only_its_block():
    w = _weight()
    _, s0 = ops.mxfp4_quantize_weight(w)
    w2 = w.clone()
    w2[5, 40] = 3.0  # block 1 of row 5
    q2, s2 = ops.mxfp4_quantize_weight(w2)
    assert int(s2[5, 1]) > int(s0[5, 1])
    s2[5, 1] = s0[5, 1]
    assert torch.equal(s2, s0)


def test_bf16_input_quantises_like_its_float_value():
    w = _weight().bfloat16()
    q1, s1 = ops.mxfp4_quantize_weight(w)
    q2, s2 = ops.mxfp4_quantize_weight(w.float())
    assert torch.equal(q1, q2) and torch.equal(s1, s2)


# ---------- swizzle ----------

@pytest.mark.parametrize("N,K", [(64, 64), (192, 448), (512, 256)])
def test_swizzle_inverse_identity(N, K):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    s = torch.randint(0, 256, (N, K // 32), generator=g, dtype=torch.uint8)
    qf, sf = ops.swizzle_weight_frag_mxfp4(q, s)
    assert qf.shape == (K // 64, N // 16, 64, 8) and qf.is_contiguous()
    assert sf.shape == (K // 64, N // 64, 16, 8) and sf.is_contiguous()
    q2, s2 = ops.unswizzle_weight_frag_mxfp4(qf, sf)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # the other composition, on random fragment bytes
    qf_r = torch.randint(0, 256, qf.shape, generator=g, dtype=torch.uint8)
    sf_r = torch.randint(0, 256, sf.shape, generator=g, dtype=torch.uint8)
    qf2, sf2 = ops.swizzle_weight_frag_mxfp4(*ops.unswizzle_weight_frag_mxfp4(qf_r, sf_r))
    assert torch.equal(qf2, qf_r) and torch.equal(sf2, sf_r)
    # the documented layout, spot-checked element by element
    for _ in range(500):
        k64, n16, lane, j = (
            int(torch.randint(0, hi, (1,), generator=g))
            for hi in (K // 64, N // 16, 64, 8)
        )
        n = n16 * 16 + (lane & 15)
        byte = k64 * 32 + (j >> 2) * 16 + (lane >> 4) * 4 + (j & 3)
        assert qf[k64, n16, lane, j] == q[n, byte]
        # that byte holds k = 2*byte, 2*byte+1: MFMA k-group lane>>4, half j>>2
        f, h = n16 & 3, j >> 2
        assert sf[k64, n16 // 4, lane & 15, f * 2 + h] == s[n, (2 * byte) // 32]


def test_swizzle_rejects_odd_shapes():
    def z(N, K):
        return (
            torch.zeros(N, K // 2, dtype=torch.uint8),
            torch.zeros(N, K // 32, dtype=torch.uint8),
        )

    with pytest.raises(AssertionError):
        ops.swizzle_weight_frag_mxfp4(*z(48, 64))
    with pytest.raises(AssertionError):
        ops.swizzle_weight_frag_mxfp4(*z(64, 96))
    with pytest.raises(AssertionError):  # scales of another K
        ops.swizzle_weight_frag_mxfp4(z(64, 64)[0], z(64, 128)[1])


def test_linear_w4_reference_and_op():
    w = _weight()
    q, s = ops.mxfp4_quantize_weight(w)
    x = torch.randn(5, w.shape[1], generator=torch.Generator().manual_seed(2))
    ref = x @ ops.mxfp4_dequantize_weight(q, s, torch.float32).T
    assert torch.equal(ops.reference.linear_w4(x, q, s), ref)
    qf, sf = ops.swizzle_weight_frag_mxfp4(q, s)
    assert torch.equal(ops.linear_w4(x, qf, sf), ref)
    assert ops.linear_w4(x.bfloat16(), qf, sf).dtype == torch.bfloat16
    assert torch.equal(
        ops.dequant_w4(qf, sf), ops.mxfp4_dequantize_weight(q, s, torch.bfloat16)
    )
    assert ops._w4_nsk(64, 4096) == 8 and ops._w4_nsk(64, 512) == 1


# ---------- sharding: quantise the full matrix, then shard bits and scales ----------

def test_sharded_dequant_equals_shard_of_dequant():
    tp = 2
    q_size, kv_size, inter, hidden = 256, 128, 512, 256
    cases = {
        "qkv": (
            _weight(q_size + 2 * kv_size, hidden, 3),
            lambda t, r: shard_qkv(t, r, tp, q_size, kv_size),
        ),
        "gate_up": (
            _weight(2 * inter, hidden, 4),
            lambda t, r: shard_gate_up(t, r, tp, inter),
        ),
        "row": (_weight(hidden, inter, 5), lambda t, r: shard_row(t, r, tp)),
    }
    for name, (w, shard) in cases.items():
        q, s = ops.mxfp4_quantize_weight(w)
        full = ops.mxfp4_dequantize_weight(q, s, torch.float32)
        for rank in range(tp):
            got = ops.mxfp4_dequantize_weight(shard(q, rank), shard(s, rank), torch.float32)
            assert torch.equal(got, shard(full, rank)), (name, rank)


def test_tp_model_is_a_sharding_of_the_tp1_model():
    cfg = get_model_config("tiny-llama")
    full = LlamaModel(cfg, dtype=torch.float32, seed=3, weight_dtype="mxfp4")
    part = LlamaModel(
        cfg.scaled_for_tp(2), dtype=torch.float32, seed=3, weight_dtype="mxfp4",
        tp_rank=1, tp_size=2, full_config=cfg,
    )

    def deq(layer, name):
        return ops.mxfp4_dequantize_weight(
            *ops.unswizzle_weight_frag_mxfp4(layer[name + "_q4"], layer[name + "_s4"]),
            torch.float32,
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


def test_engine_mxfp4_matches_fake_quant_and_is_deterministic():
    mx = _greedy(_engine(weight_dtype="mxfp4"))
    sim_eng = _engine()
    sim_eng.model.quantize_weights_("mxfp4", simulate=True)
    assert sim_eng.model.weight_dtype == "auto"
    assert mx == _greedy(sim_eng)
    assert mx == _greedy(_engine(weight_dtype="mxfp4"))


def test_mxfp4_model_layout_and_bytes():
    cfg = get_model_config("tiny-llama")
    bf16 = LlamaModel(cfg, dtype=torch.bfloat16, seed=0)
    fp8 = LlamaModel(cfg, dtype=torch.bfloat16, seed=0, weight_dtype="fp8")
    mx = LlamaModel(cfg, dtype=torch.bfloat16, seed=0, weight_dtype="mxfp4")
    proj_bf16 = proj_mx = 0
    for lb, lq in zip(bf16.layers, mx.layers):
        for name in PROJ:
            assert name not in lq and name + "_swz" not in lq and name + "_q8" not in lq
            q4, s4 = lq[name + "_q4"], lq[name + "_s4"]
            assert q4.dtype == torch.uint8 and s4.dtype == torch.uint8
            assert q4.numel() * 2 == lb[name].numel()
            assert s4.numel() * 32 == lb[name].numel()
            proj_bf16 += lb[name].numel() * lb[name].element_size()
            proj_mx += q4.numel() + s4.numel()
    assert proj_mx * 64 == proj_bf16 * 17  # 4.25 of 16 bits per weight
    # per-tensor accounting: everything else is unchanged
    assert mx.param_bytes() == bf16.param_bytes() - proj_bf16 + proj_mx
    assert mx.param_bytes() < fp8.param_bytes() < bf16.param_bytes()
    # embeddings, lm_head and norms stay in the model dtype
    assert mx.embed.dtype == mx.lm_head.dtype == torch.bfloat16
    assert mx.layers[0]["input_norm"].dtype == torch.bfloat16


def test_quantize_weights_in_place_equals_constructor():
    cfg = get_model_config("tiny-llama")
    a = LlamaModel(cfg, dtype=torch.float32, seed=1, weight_dtype="mxfp4")
    b = LlamaModel(cfg, dtype=torch.float32, seed=1).quantize_weights_("mxfp4")
    assert b.weight_dtype == "mxfp4"
    for la, lb in zip(a.layers, b.layers):
        assert la.keys() == lb.keys()
        for k in la:
            assert torch.equal(la[k], lb[k]), k
    with pytest.raises(RuntimeError):
        b.quantize_weights_("mxfp4")
    with pytest.raises(RuntimeError):
        b.quantize_weights_("fp8")


def test_simulate_keeps_auto_layout():
    cfg = get_model_config("tiny-llama")
    m = LlamaModel(cfg, dtype=torch.float32, seed=1).quantize_weights_(
        "mxfp4", simulate=True
    )
    assert m.weight_dtype == "auto"
    ref = LlamaModel(cfg, dtype=torch.float32, seed=1, weight_dtype="mxfp4")
    for lm, lr in zip(m.layers, ref.layers):
        for name in PROJ:
            want = ops.mxfp4_dequantize_weight(
                *ops.unswizzle_weight_frag_mxfp4(lr[name + "_q4"], lr[name + "_s4"]),
                torch.float32,
            )
            assert torch.equal(lm[name], want)


def test_env_fallback(monkeypatch):
    monkeypatch.setenv("LLMAPI_WEIGHT_DTYPE", "mxfp4")
    eng = _engine()
    assert eng.weight_dtype == "mxfp4" and eng.model.weight_dtype == "mxfp4"
    monkeypatch.delenv("LLMAPI_WEIGHT_DTYPE")
    assert _engine().weight_dtype == "auto"


# ---------- config ----------

def test_local_url_weight_dtype_and_engine_key():
    from llmapigateway_amd.config.loader import ProviderDetails
    from llmapigateway_amd.engine.registry import EngineRegistry

    spec = ProviderDetails(baseUrl="local://tiny-llama?weight_dtype=mxfp4").engine_spec()
    assert spec.model == "tiny-llama" and spec.weight_dtype == "mxfp4"
    fp8 = ProviderDetails(baseUrl="local://tiny-llama?weight_dtype=fp8").engine_spec()
    default = ProviderDetails(baseUrl="local://tiny-llama").engine_spec()
    reg = EngineRegistry()
    keys = {reg._engine_key(s) for s in (spec, fp8, default)}
    assert len(keys) == 3
    explicit = ProviderDetails(
        baseUrl="local://", engine={"model": "tiny-llama", "weight_dtype": "mxfp4"}
    ).engine_spec()
    assert reg._engine_key(explicit) == reg._engine_key(spec)


def test_engine_stats_report_weight_dtype():
    from llmapigateway_amd.config.loader import EngineSpec
    from llmapigateway_amd.engine.registry import EngineRegistry

    reg = EngineRegistry()
    try:
        reg.get_engine(EngineSpec(model="tiny-llama", weight_dtype="mxfp4"))
        rows = reg.stats()
        assert rows and rows[0]["weight_dtype"] == "mxfp4"
    finally:
        import asyncio

        asyncio.run(reg.aclose())
