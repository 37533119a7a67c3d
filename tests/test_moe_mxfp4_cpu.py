"""MXFP4 expert weights on the CPU: the resident layout round trip and the
mixture-of-experts model built with weight_dtype="mxfp4"."""

import dataclasses

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.engine.kvcache import PagedKVCache
from llmapigateway_amd.models.configs import ModelConfig
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel

TINY = ModelConfig(
    name="tiny-mixtral-256", hidden_size=256, intermediate_size=512,
    num_layers=2, num_heads=2, num_kv_heads=1, vocab_size=512, head_dim=128,
    rope_theta=10000.0, max_positions=512, num_experts=4, experts_per_token=2,
)


@pytest.mark.parametrize("gate_up", [True, False])
@pytest.mark.parametrize("N,K", [(128, 128), (192, 384)])
def test_pack_round_trip(N, K, gate_up):
    g = torch.Generator().manual_seed(N + K)
    packed = torch.randint(0, 256, (2, N, K // 2), generator=g).to(torch.uint8)
    scale = torch.randint(1, 255, (2, N, K // 32), generator=g).to(torch.uint8)
    q, s = ops.moe_pack_weights_mxfp4(packed, scale, gate_up)
    assert q.shape == (2, K // 128, N // 16, 64, 16) and s.shape == (2, K // 128, N // 16, 16, 4)
    back = ops.moe_unpack_weights_mxfp4(q, s, gate_up)
    assert torch.equal(back[0], packed) and torch.equal(back[1], scale)


def decode_logits(model, rows=5):
    """Logits of a `rows`-sequence decode batch on the model's device."""
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
    return model.forward(batch, kv.k_caches, kv.v_caches).float()


def test_model_is_the_quantisation_of_the_bf16_model():
    """Same seed, same draw order: the mxfp4 model is the quantisation of the
    bf16 model, and its logits equal the fake-quant bf16 model's bit for bit
    (the dense qkv/o reference casts the same dequantised values to fp32)."""
    model = LlamaModel(TINY, device="cpu", weight_dtype="mxfp4", seed=0)
    layer = model.layers[0]
    assert layer["router"].dtype == torch.bfloat16 and "qkv_q4" in layer
    assert layer["experts_gate_up_q4"].shape == (4, 1024, 128) and "experts_gate_up" not in layer
    sim = LlamaModel(TINY, device="cpu", seed=0).quantize_weights_("mxfp4", simulate=True)
    assert torch.equal(decode_logits(model), decode_logits(sim))
    real = LlamaModel(TINY, device="cpu", seed=0).quantize_weights_("mxfp4")
    assert torch.equal(real.layers[1]["experts_down_q4"], model.layers[1]["experts_down_q4"])


def test_unserved_intermediate_size_raises():
    with pytest.raises(ValueError, match="128"):
        LlamaModel(dataclasses.replace(TINY, intermediate_size=576), weight_dtype="mxfp4")
    LlamaModel(dataclasses.replace(TINY, intermediate_size=576, num_layers=1))  # bf16 serves it
