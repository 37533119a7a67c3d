"""Sliding-window attention in the engine on the GPU. tiny-llama-swa itself
has 64-wide heads, which the attention kernels do not take, so these tests
run its window (24) on the d128 tiny shape of test_engine_gpu.py."""

import dataclasses

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.engine import EngineRequest, LLMEngine, SamplingParams
from llmapigateway_amd.engine.kvcache import RELEASED
from llmapigateway_amd.models.configs import ModelConfig, get_model_config

pytestmark = pytest.mark.gpu

W = get_model_config("tiny-llama-swa").sliding_window
GPU_TINY = ModelConfig(
    name="gpu-tiny",
    hidden_size=512,
    intermediate_size=1024,
    num_layers=2,
    num_heads=4,
    num_kv_heads=2,
    vocab_size=2048,
    head_dim=128,
    rope_theta=10000.0,
    max_positions=1024,
)
GPU_TINY_SWA = dataclasses.replace(GPU_TINY, name="gpu-tiny-swa", sliding_window=W)
BS = 16


def _engine(model=GPU_TINY_SWA, **kw):
    assert torch.cuda.is_available() and ops.have_native()
    kw.setdefault("prefill_budget", 32)  # prompts longer than this are chunked
    return LLMEngine(model=model, device="cuda:0", dtype=torch.bfloat16,
                     block_size=BS, num_blocks=128, seed=0, max_batch_size=4, **kw)


def _prompts():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(3, 2000, (n,), generator=g).tolist() for n in (70, 9, 33)]


def _run(engine, max_tokens=48):
    """One batch of three requests: prompts above and below the window, every
    one decoding across it. Returns (ids, peak blocks held while decoding)."""
    free0 = engine.kv.manager.num_free_blocks
    reqs = [EngineRequest(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True,
                                            temperature=0.0)) for p in _prompts()]
    for r in reqs:
        engine.add_request(r)
    peak, steps = 0, 0
    while any(r.state in ("waiting", "running") for r in reqs):
        engine.step()
        steps += 1
        assert steps < 10_000
        for r in reqs:
            if len(r.out_ids) >= 3:
                peak = max(peak, sum(b is not RELEASED for b in r.block_table))
    engine._flush_pending()
    torch.cuda.synchronize()
    assert all(len(r.out_ids) == max_tokens for r in reqs)
    assert engine.kv.manager.num_free_blocks == free0
    return [r.out_ids for r in reqs], peak


@pytest.mark.parametrize("kv_dtype", ["auto", "fp8"])
def test_hipgraph_equals_eager_across_the_window(kv_dtype):
    graph = _engine(kv_dtype=kv_dtype)
    assert graph.graph_runner is not None and graph.sliding_window == W
    eager = _engine(kv_dtype=kv_dtype, use_hipgraph=False)
    assert eager.graph_runner is None
    ids_g, peak_g = _run(graph)
    ids_e, peak_e = _run(eager)
    assert graph.stats["graph_steps"] > 0 and graph.graph_runner is not None
    assert ids_g == ids_e
    # blocks were released on the way: a decoding sequence holds its window
    assert max(peak_g, peak_e) <= -(-W // BS) + 1 < -(-(70 + 48) // BS)


def test_release_does_not_change_the_ids():
    """Released blocks go back to the pool and are written by the other
    sequences of the batch; a kernel that still read them would differ."""
    on, peak_on = _run(_engine())
    kept = _engine()
    kept._swa_release = False
    off, peak_off = _run(kept)
    assert on == off
    assert peak_on < peak_off == -(-(70 + 48) // BS)


def test_window_changes_the_ids_and_short_prompts_do_not_see_it():
    swa, full = _engine(), _engine(GPU_TINY)
    ids_w, _ = _run(swa)
    ids_f, _ = _run(full)
    assert ids_w != ids_f
    p = _prompts()[1]  # 9 tokens + 10 stay inside the window
    sp = SamplingParams(max_tokens=10, ignore_eos=True, temperature=0.0)
    assert swa.generate(p, sp).out_ids == full.generate(p, sp).out_ids
