"""Multi-LoRA on the CPU: the reference ops, the model against merged
weights, and the engine's adapter bookkeeping (slots, mixed batches,
preemption, prefix-cache roots, config and gateway plumbing)."""

import inspect
import json

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.config.loader import AdapterSpec, EngineSpec, ProviderDetails
from llmapigateway_amd.engine import EngineRequest, LLMEngine, SamplingParams
from llmapigateway_amd.engine.kvcache import BlockManager
from llmapigateway_amd.models import get_model_config
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel
from llmapigateway_amd.ops import reference

CFG = get_model_config("tiny-llama")


# ---------- reference ops ----------

def _stack(S, N, K, R, nseg, ranks, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(S, nseg * R, K, dtype=dtype)
    B = torch.zeros(S, N, R, dtype=dtype)
    for s, r in enumerate(ranks):
        for seg in range(nseg):
            A[s, seg * R : seg * R + r] = torch.randn(r, K, generator=g, dtype=dtype)
        B[s, :, :r] = torch.randn(N, r, generator=g, dtype=dtype)
    return A, B


def test_reference_lora_add_is_the_low_rank_product():
    T, K, N, R = 6, 48, 40, 8
    ranks = torch.tensor([8, 3], dtype=torch.int32)
    scales = torch.tensor([2.0, 0.25])
    A, B = _stack(2, N, K, R, 1, ranks.tolist())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, K, generator=g, dtype=torch.float64)
    y0 = torch.randn(T, N, generator=g, dtype=torch.float64)
    ids = torch.tensor([0, 1, -1, 1, 0, -1], dtype=torch.int32)
    st = ops.LoraStack(A, B, ranks, scales, (N,))
    y = ops.lora_add(y0.clone(), x, st, ids)
    for i, s in enumerate(ids.tolist()):
        want = y0[i] if s < 0 else y0[i] + x[i] @ (float(scales[s]) * B[s] @ A[s]).T
        # t is fp32 between the two ops: fp32 rounding of a fp64 product
        assert torch.allclose(y[i], want, rtol=0, atol=1e-4), i
        if s < 0:
            assert torch.equal(y[i], y0[i])


def test_reference_qkv_three_segments_equal_merged_weight():
    T, K, R = 5, 32, 8
    bounds = (24, 32, 40)  # q | k | v
    N = bounds[-1]
    ranks = torch.tensor([5, 8], dtype=torch.int32)
    scales = torch.tensor([0.5, 3.0])
    g = torch.Generator().manual_seed(2)
    A, B = _stack(2, N, K, R, 3, ranks.tolist(), seed=3)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    x = torch.randn(T, K, generator=g, dtype=torch.float64)
    ids = torch.tensor([1, 0, 0, -1, 1], dtype=torch.int32)
    y = ops.lora_add(x @ W.T, x, ops.LoraStack(A, B, ranks, scales, bounds), ids)
    for i, s in enumerate(ids.tolist()):
        merged = W.clone()
        lo = 0
        for seg, hi in enumerate(bounds):
            if s >= 0:  # each segment has its own A: three adapters side by side
                merged[lo:hi] += float(scales[s]) * B[s, lo:hi] @ A[s, seg * R : (seg + 1) * R]
            lo = hi
        assert torch.allclose(y[i], merged @ x[i], rtol=0, atol=1e-4), i


def test_reference_shrink_zeroes_what_the_kernel_skips():
    A, _ = _stack(2, 8, 16, 8, 2, [3, 8], dtype=torch.float32)
    A[0, 3:8] = 1.0  # padding that is NOT zero: the rank must mask it
    x = torch.ones(3, 16)
    ids = torch.tensor([0, -1, 1], dtype=torch.int32)
    t = ops.lora_shrink(x, A, torch.tensor([3, 8], dtype=torch.int32), ids, 2)
    assert t.shape == (3, 16) and t.dtype == torch.float32
    assert bool((t[1] == 0).all()) and bool((t[0, 3:8] == 0).all())
    assert bool((t[0, :3] != 0).all()) and bool((t[2] != 0).all())


# ---------- model ----------

def _prefill_logits(model, ids_per_row, tokens, adapter_ids):
    """One single-token prompt per row (a flat prefill batch)."""
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    n = len(tokens)
    kv = PagedKVCache(model.config, n, 16, "cpu", model.dtype)
    batch = ForwardBatch(
        kind="prefill",
        token_ids=torch.tensor(tokens, dtype=torch.long),
        positions=torch.zeros(n, dtype=torch.long),
        slot_mapping=torch.arange(n) * 16,
        cu_seqlens=torch.arange(n + 1, dtype=torch.int32),
        max_seqlen=1,
        logits_indices=torch.arange(n),
        adapter_ids=adapter_ids,
    )
    return model.forward(batch, kv.k_caches, kv.v_caches)


def _model(**kw):
    return LlamaModel(CFG, device="cpu", dtype=torch.float32, seed=0, **kw)


def test_model_with_adapter_matches_merged_weights():
    model = _model(max_loras=2, max_lora_rank=12)
    assert model.max_lora_rank == 16  # rounded up to a multiple of 8
    adapter = model.random_adapter(12, seed=1)
    assert all(bool(t.abs().sum() > 0) for t in adapter.values())  # lora_B too
    model.set_adapter(1, adapter, alpha=24.0)
    scale = 24.0 / 12

    merged = _model()
    for i, layer in enumerate(merged.layers):
        for target, (name, seg) in LlamaModel.LORA_TARGETS.items():
            a = adapter[f"layers.{i}.{target}.lora_A"]
            b = adapter[f"layers.{i}.{target}.lora_B"]
            widths = model._lora_shapes()[name][1]
            lo = sum(widths[:seg])
            layer[name][lo : lo + widths[seg]] += scale * (b @ a)

    tokens = [3, 77, 200, 411]
    got = _prefill_logits(model, None, tokens, torch.full((4,), 1, dtype=torch.int32))
    want = _prefill_logits(merged, None, tokens, None)
    base = _prefill_logits(_model(), None, tokens, None)
    assert (want - base).abs().max() > 1e-2  # the adapter moves the logits
    assert torch.allclose(got, want, rtol=0, atol=1e-4)
    # an empty slot and slot -1 are the base model
    for ids in ([0] * 4, [-1] * 4):
        out = _prefill_logits(model, None, tokens, torch.tensor(ids, dtype=torch.int32))
        assert torch.allclose(out, base, rtol=0, atol=1e-5)
    assert torch.allclose(_prefill_logits(model, None, tokens, None), base, atol=1e-5)


def test_model_mixed_rows_equal_uniform_batches():
    model = _model(max_loras=2, max_lora_rank=8)
    model.set_adapter(0, model.random_adapter(8, seed=1), alpha=16.0)
    model.set_adapter(1, model.random_adapter(3, seed=2, targets=["q_proj", "down_proj"]))
    tokens = [3, 77, 200, 411]
    mix = torch.tensor([0, -1, 1, 0], dtype=torch.int32)
    got = _prefill_logits(model, None, tokens, mix)
    for row, slot in enumerate(mix.tolist()):
        uniform = _prefill_logits(
            model, None, tokens, torch.full((4,), slot, dtype=torch.int32)
        )
        assert torch.allclose(got[row], uniform[row], rtol=0, atol=1e-5), row
    assert not torch.allclose(got[0], got[1], atol=1e-3)


def test_set_adapter_rejects_bad_input():
    model = _model(max_loras=1, max_lora_rank=8)
    good = model.random_adapter(4, seed=0, targets=["o_proj"])
    model.set_adapter(0, good)
    with pytest.raises(ValueError):
        model.set_adapter(1, good)  # no such slot
    with pytest.raises(ValueError):
        model.set_adapter(0, model.random_adapter(9, seed=0))  # rank > max
    with pytest.raises(ValueError):
        model.set_adapter(0, {**good, "layers.0.bogus.lora_A": torch.zeros(4, 4)})
    bad = dict(good)
    bad["layers.0.o_proj.lora_B"] = torch.zeros(7, 4)
    with pytest.raises(ValueError):
        model.set_adapter(0, bad)
    with pytest.raises(ValueError):
        model.random_adapter(4, targets=["nope"])


# ---------- engine ----------

PROMPT = list(range(7, 47))  # 40 tokens: 2 full blocks of 16 are cacheable


def make_engine(**kw):
    kw.setdefault("model", "tiny-llama")
    kw.setdefault("device", "cpu")
    kw.setdefault("dtype", torch.float32)
    kw.setdefault("block_size", 16)
    kw.setdefault("num_blocks", 64)
    kw.setdefault("seed", 3)
    kw.setdefault("max_loras", 2)
    eng = LLMEngine(**kw)
    if eng.max_loras:
        eng.load_adapter("a", rank=8, alpha=64.0, seed=1)
        eng.load_adapter("b", rank=4, alpha=32.0, seed=2)
    return eng


def _gen(eng, adapter, prompt=PROMPT, n=8):
    return eng.generate(
        prompt, SamplingParams(max_tokens=n, ignore_eos=True, adapter=adapter)
    )


def _drain(eng, reqs):
    for _ in range(2000):
        if all(r.state in ("finished", "failed") for r in reqs):
            return
        eng.step()
    raise AssertionError("engine did not finish")


def test_engine_adapter_changes_greedy_tokens():
    eng = make_engine()
    base = _gen(eng, None).out_ids
    assert base == _gen(make_engine(max_loras=0), None).out_ids
    a = _gen(eng, "a").out_ids
    b = _gen(eng, "b").out_ids
    assert a != base and b != base and a != b
    assert [d["name"] for d in eng.list_adapters()] == ["a", "b"]
    assert [d["rank"] for d in eng.list_adapters()] == [8, 4]


def test_engine_two_adapters_in_one_batch_equal_solo_runs():
    solo = {ad: _gen(make_engine(), ad, n=10).out_ids for ad in ("a", "b", None)}
    eng = make_engine()
    reqs = [
        eng.add_request(EngineRequest(
            PROMPT, SamplingParams(max_tokens=10, ignore_eos=True, adapter=ad)))
        for ad in ("a", "b", None, "a")
    ]
    _drain(eng, reqs)
    assert eng.stats["decode_steps"] > 0
    assert [r.out_ids for r in reqs] == [solo["a"], solo["b"], solo[None], solo["a"]]


def test_engine_chunked_and_mixed_steps_carry_the_adapter():
    long_prompt = [(7 * i) % 500 + 1 for i in range(90)]
    want = {ad: _gen(make_engine(), ad, long_prompt).out_ids for ad in ("a", "b")}
    eng = make_engine(prefill_budget=32)  # 90 tokens: three chunks
    first = eng.add_request(EngineRequest(
        PROMPT, SamplingParams(max_tokens=12, ignore_eos=True, adapter="b")))
    eng.step()  # b is decoding when the long prompts arrive: mixed steps
    reqs = [
        eng.add_request(EngineRequest(
            long_prompt, SamplingParams(max_tokens=8, ignore_eos=True, adapter=ad)))
        for ad in ("a", "b")
    ]
    _drain(eng, [first] + reqs)
    assert eng.stats["mixed_steps"] > 0
    assert [r.out_ids for r in reqs] == [want["a"], want["b"]]
    assert first.out_ids == _gen(make_engine(), "b", n=12).out_ids


def test_engine_preemption_keeps_the_adapter():
    prompt = list(range(1, 20))
    want = {ad: _gen(make_engine(), ad, prompt, n=40).out_ids for ad in ("a", "b", None)}
    eng = make_engine(num_blocks=8, max_batch_size=4)
    preempted = []
    real = eng._preempt_youngest
    eng._preempt_youngest = lambda: (preempted.append(1), real())[1]
    reqs = [
        eng.add_request(EngineRequest(
            prompt, SamplingParams(max_tokens=40, ignore_eos=True, adapter=ad)))
        for ad in ("a", "b", None)
    ]
    _drain(eng, reqs)
    assert preempted, "the pool was meant to be too small"
    for r, ad in zip(reqs, ("a", "b", None)):
        # a preempted request carries its tokens over into prompt_ids
        assert (r.prompt_ids + r.out_ids)[len(prompt):][:40] == want[ad], ad


def test_engine_unknown_adapter_fails_that_request_only():
    eng = make_engine()
    ok = eng.add_request(EngineRequest(
        PROMPT, SamplingParams(max_tokens=4, ignore_eos=True, adapter="a")))
    bad = EngineRequest(PROMPT, SamplingParams(max_tokens=4, adapter="nope"))
    with pytest.raises(ValueError, match="unknown LoRA adapter 'nope'"):
        eng.add_request(bad)
    assert bad.state == "failed" and "nope" in bad.error
    _drain(eng, [ok])
    assert ok.state == "finished" and len(ok.out_ids) == 4
    with pytest.raises(ValueError):  # an engine without adapters knows none
        _gen(make_engine(max_loras=0), "a")


def test_engine_unload_raises_while_busy_and_slot_is_reused():
    eng = make_engine()
    req = eng.add_request(EngineRequest(
        PROMPT, SamplingParams(max_tokens=6, ignore_eos=True, adapter="a")))
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("a")  # waiting
    eng.step()
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("a")  # running
    with pytest.raises(RuntimeError, match="slots are in use"):
        eng.load_adapter("c", rank=4, seed=5)
    _drain(eng, [req])
    slot_a = next(d["slot"] for d in eng.list_adapters() if d["name"] == "a")
    uids = [d["uid"] for d in eng.list_adapters()]
    eng.unload_adapter("a")
    with pytest.raises(KeyError):
        eng.unload_adapter("a")
    with pytest.raises(ValueError):
        _gen(eng, "a")
    eng.load_adapter("c", rank=4, alpha=32.0, seed=5)
    c = next(d for d in eng.list_adapters() if d["name"] == "c")
    assert c["slot"] == slot_a and c["uid"] > max(uids)
    ref = make_engine()
    ref.unload_adapter("b")
    ref.load_adapter("c", rank=4, alpha=32.0, seed=5)
    assert _gen(eng, "c").out_ids == _gen(ref, "c").out_ids
    assert _gen(eng, "c").out_ids != req.out_ids


def test_load_adapter_from_tensors_and_path(tmp_path):
    eng = make_engine()
    tensors = eng.model.random_adapter(8, seed=1)
    torch.save(tensors, tmp_path / "a.pt")
    eng.unload_adapter("b")
    eng.load_adapter("from-path", path=str(tmp_path / "a.pt"), alpha=64.0)
    assert _gen(eng, "from-path").out_ids == _gen(eng, "a").out_ids
    eng.load_adapter("from-path", tensors, alpha=8.0)  # replace while idle
    assert _gen(eng, "from-path").out_ids != _gen(eng, "a").out_ids


# ---------- prefix cache ----------

def test_prefix_cache_never_crosses_adapters():
    plain = make_engine()
    want = {ad: _gen(plain, ad).out_ids for ad in (None, "a")}
    eng = make_engine(prefix_caching=True)
    r_base = _gen(eng, None)
    r_a1 = _gen(eng, "a")
    r_a2 = _gen(eng, "a")
    assert (r_base.num_cached, r_a1.num_cached, r_a2.num_cached) == (0, 0, 32)
    assert r_base.out_ids == want[None]
    assert r_a1.out_ids == want["a"] and r_a2.out_ids == want["a"]
    assert _gen(eng, None).num_cached == 32  # the base chain is still there
    assert _gen(eng, "b").num_cached == 0

    # the same name loaded again is another adapter to the cache
    eng.unload_adapter("a")
    eng.load_adapter("a", rank=8, alpha=64.0, seed=1)
    again = _gen(eng, "a")
    assert again.num_cached == 0 and again.out_ids == want["a"]
    assert _gen(eng, "a").num_cached == 32


def test_block_manager_root_separates_chains():
    m = BlockManager(num_blocks=16, block_size=4, prefix_caching=True)
    ids = list(range(9))
    bt, cached = m.allocate_with_prefix(ids)
    assert cached == 0
    m.register_prefix(ids, bt)
    assert m.allocate_with_prefix(ids)[1] == 8
    assert m.allocate_with_prefix(ids, root=-1)[1] == 8  # the default root
    assert m.allocate_with_prefix(ids, root=-2)[1] == 0
    bt2, _ = m.allocate_with_prefix(ids, root=-3)
    m.register_prefix(ids, bt2, root=-3)
    assert m.allocate_with_prefix(ids, root=-3)[1] == 8
    assert m.allocate_with_prefix(ids, root=-2)[1] == 0


# ---------- compatibility ----------

def test_max_loras_zero_changes_nothing():
    eng = make_engine(max_loras=0)
    assert eng.model.lora_layers == [] and not hasattr(eng.model, "lora_ranks")
    with pytest.raises(RuntimeError):
        eng.load_adapter("a", rank=4)
    assert eng.list_adapters() == []
    # the old call forms still work
    batch = ForwardBatch(
        "decode", torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long),
        torch.zeros(1, dtype=torch.long),
    )
    assert batch.adapter_ids is None
    m = BlockManager(num_blocks=8, block_size=4, prefix_caching=True)
    bt, n = m.allocate_with_prefix(list(range(6)))
    m.register_prefix(list(range(6)), bt)
    from llmapigateway_amd.engine.graph_runner import DecodeGraphRunner

    params = inspect.signature(DecodeGraphRunner.run).parameters
    assert list(params)[:6] == [
        "self", "tokens", "positions", "slots", "block_tables", "context_lens"
    ]
    assert params["adapter_ids"].default is None
    assert SamplingParams().adapter is None
    assert SamplingParams.from_payload({}).adapter is None
    assert SamplingParams.from_payload({"adapter": "x"}).adapter == "x"


def test_graph_runner_adapter_buffer_on_cpu():
    """The runner's buffers without capturing anything: the adapter column
    exists, and enters the batch only when the model has adapters."""
    from llmapigateway_amd.engine.graph_runner import DecodeGraphRunner

    for loras in (0, 2):
        model = _model(max_loras=loras)
        r = DecodeGraphRunner(model, [], [], max_batch=4, max_blocks=2)
        assert r.adapter_ids.dtype == torch.int32 and r.adapter_ids.tolist() == [-1] * 4
        view = r._batch_view(3)
        if loras:
            assert view.adapter_ids.shape == (3,)
            assert view.adapter_ids.data_ptr() == r.adapter_ids.data_ptr()
        else:
            assert view.adapter_ids is None


def test_tp_with_adapters_raises():
    with pytest.raises(NotImplementedError, match="not supported"):
        LLMEngine(model="tiny-llama", device="cpu", dtype=torch.float32,
                  num_blocks=8, tp_size=2, max_loras=1)
    LLMEngine(model="tiny-llama", device="cpu", dtype=torch.float32,
              num_blocks=8, max_loras=1)


# ---------- config and gateway ----------

def test_engine_spec_adapters_block():
    from llmapigateway_amd.engine.registry import EngineRegistry

    spec = EngineSpec(model="tiny-llama", adapters={
        "x": {"rank": 8, "alpha": 16, "seed": 1},
        "y": {"rank": 4, "targets": ["q_proj", "v_proj"]},
    })
    assert spec.max_loras == 2 and spec.max_lora_rank == 16
    assert isinstance(spec.adapters["x"], AdapterSpec)
    assert spec.adapters["y"].targets == ["q_proj", "v_proj"]
    assert EngineSpec().max_loras == 0 and EngineSpec().adapters == {}
    with pytest.raises(ValueError):
        EngineSpec(max_loras=1, adapters={"x": {"rank": 4}, "y": {"rank": 4}})

    reg = EngineRegistry()
    plain = EngineSpec(model="tiny-llama")
    other = spec.model_copy(update={"adapters": {"x": AdapterSpec(rank=8, seed=2)}})
    keys = {reg._engine_key(s) for s in (plain, spec, other)}
    assert len(keys) == 3
    assert reg._engine_key(plain) == "tiny-llama@0x1"  # as before
    # an engine object on a local:// entry keeps its adapters
    entry = ProviderDetails(
        baseUrl="local://tiny-llama?device=0",
        engine={"model": "tiny-llama", "max_loras": 3, "adapters": {"x": {"rank": 4}}},
    )
    assert entry.engine_spec().max_loras == 3
    assert list(entry.engine_spec().adapters) == ["x"]


PROVIDERS = """
[
    { "lora-engine": {
        "baseUrl": "local://tiny-llama?device=0", "apikey": "",
        "engine": { "model": "tiny-llama",
                    "adapters": { "x": { "rank": 8, "alpha": 64, "seed": 1 } } }
    } }
]
"""

RULES = """
[
    { "gateway_model_name": "local/base",
      "fallback_models": [ { "provider": "lora-engine", "model": "tiny-llama" } ] },
    { "gateway_model_name": "local/tuned",
      "fallback_models": [ { "provider": "lora-engine", "model": "tiny-llama",
                             "custom_body_params": { "adapter": "x" } } ] },
    { "gateway_model_name": "local/missing-then-base",
      "fallback_models": [
          { "provider": "lora-engine", "model": "tiny-llama",
            "custom_body_params": { "adapter": "nope" } },
          { "provider": "lora-engine", "model": "tiny-llama",
            "custom_body_params": { "adapter": null } } ] }
]
"""


@pytest.fixture
def client(tmp_path):
    from fastapi.testclient import TestClient

    from llmapigateway_amd.config.settings import Settings
    from llmapigateway_amd.gateway.app import create_app

    (tmp_path / "providers.json").write_text(PROVIDERS)
    (tmp_path / "models_fallback_rules.json").write_text(RULES)
    app = create_app(
        settings=Settings(fallback_provider="lora-engine"),
        providers_path=str(tmp_path / "providers.json"),
        fallback_rules_path=str(tmp_path / "models_fallback_rules.json"),
        db_dir=str(tmp_path / "db"),
        log_dir=str(tmp_path / "logs"),
    )
    with TestClient(app) as c:
        yield c


def _chat(client, model, **kw):
    return client.post(
        "/v1/chat/completions",
        json={
            "model": model,
            "messages": [{"role": "user", "content": "write a story"}],
            "max_tokens": 8, "ignore_eos": True, **kw,
        },
    )


def test_gateway_rule_selects_the_adapter(client, monkeypatch):
    seen = []
    real = SamplingParams.from_payload.__func__

    def spy(cls, payload, *a, **kw):
        params = real(cls, payload, *a, **kw)
        seen.append((payload.get("adapter"), params.adapter))
        return params

    monkeypatch.setattr(SamplingParams, "from_payload", classmethod(spy))
    base = _chat(client, "local/base")
    tuned = _chat(client, "local/tuned")
    assert base.status_code == 200 and tuned.status_code == 200, tuned.text
    assert seen == [(None, None), ("x", "x")]
    text = lambda r: r.json()["choices"][0]["message"]["content"]
    assert text(base) != text(tuned)
    assert text(tuned) == text(_chat(client, "local/tuned"))
    # the client can name the adapter itself, and n > 1 fans it out
    direct = _chat(client, "local/base", adapter="x", n=2)
    assert [c["message"]["content"] for c in direct.json()["choices"]] == [text(tuned)] * 2

    # an unknown adapter fails the attempt; the fallback chain moves on
    seen.clear()
    r = _chat(client, "local/missing-then-base")
    assert r.status_code == 200, r.text
    assert [s[1] for s in seen] == ["nope", None]
    assert text(r) == text(base)
    r = _chat(client, "local/base", adapter="nope")
    assert r.status_code == 503 and "unknown LoRA adapter" in r.json()["detail"]

    stats = client.get("/v1/api/engine-stats").json()["engines"]
    assert len(stats) == 1  # all three rules share one engine
    assert [a["name"] for a in stats[0]["adapters"]] == ["x"]
    assert stats[0]["adapters"][0]["rank"] == 8
    assert json.dumps(stats)  # serialisable
