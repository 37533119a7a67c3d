"""Mixture of experts on the CPU: the reference semantics, the presets, and
an engine on tiny-mixtral."""

import dataclasses

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.models.configs import get_model_config
from llmapigateway_amd.models.llama import LlamaModel
from llmapigateway_amd.ops import reference


def _layer_inputs(T=9, seed=0):
    model = LlamaModel(get_model_config("tiny-mixtral"), seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    H = model.config.hidden_size
    x = torch.randn(T, H, generator=g).bfloat16()
    res = torch.randn(T, H, generator=g).bfloat16()
    return model, model.layers[0], x, res, model.layers[1]["input_norm"]


def test_moe_mlp_equals_per_token_loop():
    model, layer, x, res, norm_w = _layer_inputs()
    k, inter = model.config.experts_per_token, model.config.intermediate_size
    got_n, got_r = ops.moe_mlp(
        x, layer["router"], layer["experts_gate_up"], layer["experts_down"], k,
        res.clone(), norm_w, 1e-5,
    )
    for t in range(x.shape[0]):
        probs = torch.softmax(x[t].float() @ layer["router"].float().T, dim=-1)
        # descending weight, then ascending index
        order = sorted(range(len(probs)), key=lambda e: (-probs[e].item(), e))[:k]
        total = sum(probs[e] for e in order)
        acc = torch.zeros(x.shape[1])
        for e in order:
            h = x[t].float() @ layer["experts_gate_up"][e].float().T
            act = (h[:inter] * torch.sigmoid(h[:inter]) * h[inter:]).bfloat16()
            y = act.float() @ layer["experts_down"][e].float().T
            acc = acc + ((probs[e] / total) * y).bfloat16().float()
        r = (acc + res[t].float()).bfloat16()
        # one bf16 ulp (2^-7 relative): a batched matmul and per-row matvecs
        # may differ in the last fp32 bit and flip a rounding
        ulp = lambda v: 2.0 ** -7 * v.float().abs() + 1e-30
        assert bool(((got_r[t].float() - r.float()).abs() <= ulp(r)).all())
        n = reference.rmsnorm(got_r[t], norm_w, 1e-5)
        assert bool(((got_n[t].float() - n.float()).abs() <= ulp(n)).all())


@pytest.mark.parametrize("k", [1, 2, 4])
def test_identical_experts_equal_the_dense_mlp(k):
    """All experts the same: the routing weights sum to 1, so the layer is
    the dense MLP up to the bf16 rounding of the k pair outputs."""
    model, layer, x, res, norm_w = _layer_inputs(seed=k)
    gu = layer["experts_gate_up"][:1].expand(4, -1, -1).contiguous()
    dn = layer["experts_down"][:1].expand(4, -1, -1).contiguous()
    _, got = ops.moe_mlp(x, layer["router"], gu, dn, k, res.clone(), norm_w, 1e-5)
    act = reference.swiglu(torch.nn.functional.linear(x, gu[0])).float()
    y = act @ dn[0].float().T
    # the k pair outputs and the new residual are each rounded once (2^-9
    # relative; 2^-8 allowed). The dense route also rounds gate and up to
    # bf16 before the swiglu: relative 2^-9 on u, and 2^-9 |1 + g (1 -
    # sigmoid(g))| <= 2^-8 on silu(g) for the |g| < 2 of this data, so act
    # moves by at most 2^-7 relative, carried through |down|
    bound = (2.0 ** -8 * y.abs() + 2.0 ** -8 * (y + res.float()).abs()
             + 2.0 ** -7 * (act.abs() @ dn[0].float().abs().T) + 1e-6)
    assert bool(((got.float() - (y + res.float())).abs() <= bound).all())


def test_pack_weights_round_trip():
    w = torch.randn(3, 128, 64).bfloat16()
    for gate_up in (True, False):
        packed = ops.moe_pack_weights(w, gate_up)
        assert packed.shape == (3, 2, 8, 64, 8)
        assert torch.equal(ops.moe_unpack_weights(packed, gate_up), w)


def test_engine_generates_and_chunked_prefill_equals_single_shot():
    from llmapigateway_amd.engine import LLMEngine, SamplingParams

    outs = []
    for budget in (4096, 16):
        eng = LLMEngine(model="tiny-mixtral", device="cpu", num_blocks=32,
                        block_size=16, prefill_budget=budget)
        req = eng.generate(list(range(3, 60)), SamplingParams(max_tokens=6, ignore_eos=True))
        assert req.state == "finished" and len(req.out_ids) == 6
        outs.append(req.out_ids)
    assert outs[0] == outs[1]


def test_presets_and_rejections():
    c = get_model_config("mixtral-8x7b")
    assert (c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads,
            c.num_kv_heads, c.vocab_size) == (4096, 14336, 32, 32, 8, 32000)
    assert (c.rope_theta, c.max_positions, c.sliding_window) == (1e6, 32768, None)
    assert (c.num_experts, c.experts_per_token) == (8, 2)
    tiny = get_model_config("tiny-mixtral")
    assert (tiny.num_experts, tiny.experts_per_token) == (4, 2)
    assert dataclasses.replace(tiny, num_experts=0, experts_per_token=0,
                               name="tiny-llama") == get_model_config("tiny-llama")
    for kw in ({"weight_dtype": "fp8"}, {"max_loras": 1}, {"tp_size": 2}):
        with pytest.raises(NotImplementedError):
            LlamaModel(tiny, **kw)
    with pytest.raises(ValueError):
        LlamaModel(dataclasses.replace(tiny, experts_per_token=5))


def test_gateway_serves_a_tiny_mixtral_provider(tmp_repo):
    import json

    from fastapi.testclient import TestClient

    (tmp_repo / "providers.json").write_text(json.dumps(
        [{"local-moe": {"baseUrl": "local://tiny-mixtral?device=0", "apikey": "",
                        "engine": {"model": "tiny-mixtral"}}}]
    ))
    (tmp_repo / "models_fallback_rules.json").write_text(json.dumps(
        [{"gateway_model_name": "llmgateway/moe",
          "fallback_models": [{"provider": "local-moe", "model": "tiny-mixtral"}]}]
    ))
    from llmapigateway_amd.gateway.app import create_app

    with TestClient(create_app()) as client:
        r = client.post(
            "/v1/chat/completions",
            json={"model": "llmgateway/moe", "max_tokens": 4, "ignore_eos": True,
                  "messages": [{"role": "user", "content": "hi"}]},
        )
        assert r.status_code == 200
        assert r.json()["usage"]["completion_tokens"] == 4
