"""Sliding-window attention above the kernels, on the CPU: the block
manager's release_before, the tiny-llama-swa engine (window 24) and the
provider option."""

import math

import pytest
import torch

from llmapigateway_amd.config.loader import EngineSpec, ProviderDetails, parse_providers
from llmapigateway_amd.engine import EngineRequest, LLMEngine, SamplingParams
from llmapigateway_amd.engine.kvcache import RELEASED, BlockManager
from llmapigateway_amd.models.configs import get_model_config

BS = 8
W = 24  # tiny-llama-swa


# ---------- presets ----------

def test_presets():
    swa = get_model_config("tiny-llama-swa")
    assert swa.sliding_window == W
    assert get_model_config("tiny-llama").sliding_window is None
    v01, base = get_model_config("mistral-7b-v0.1"), get_model_config("mistral-7b")
    assert base.sliding_window is None and base.max_positions == 8192
    assert v01.sliding_window == 4096 and v01.max_positions == 32768
    for f in ("hidden_size", "intermediate_size", "num_layers", "num_heads",
              "num_kv_heads", "vocab_size", "head_dim", "rope_theta"):
        assert getattr(v01, f) == getattr(base, f)
    assert v01.scaled_for_tp(2).sliding_window == 4096


# ---------- release_before ----------

def test_release_before_bounds_the_blocks_of_a_sequence():
    """A sequence that grows token by token and releases after each one
    holds at most ceil(W / BS) + 1 blocks; everything returns at the end."""
    m = BlockManager(64, BS)
    free0 = m.num_free_blocks
    bt = m.allocate(5)
    for n in range(5, 200):           # n tokens held, the next one is n
        m.extend(bt, n, n + 1)
        # the query at position n reads keys n - W + 1 .. n
        m.release_before(bt, n - W + 1)
        held = [b for b in bt if b is not RELEASED]
        assert len(held) <= math.ceil(W / BS) + 1
        assert free0 - m.num_free_blocks == len(held)
        assert len(bt) == m.blocks_needed(n + 1)      # positions stay absolute
        first = max(n - W + 1, 0) // BS
        assert all(b is RELEASED for b in bt[:first])
        assert all(b is not RELEASED for b in bt[first:])
        assert all(0 <= int(b) < 64 for b in bt)      # placeholders are in range
    m.free(bt)
    assert m.num_free_blocks == free0


def test_release_before_with_a_chunk_in_flight():
    m = BlockManager(64, BS)
    free0 = m.num_free_blocks
    L, chunk = 150, 40
    bt = m.allocate(L)
    for end in range(chunk, L, chunk):    # chunks [end - chunk, end) are written
        m.release_before(bt, end - W + 1)  # the next chunk starts at `end`
        held = sum(b is not RELEASED for b in bt[: m.blocks_needed(end + chunk)])
        assert held <= math.ceil(W / BS) + 1 + math.ceil(chunk / BS)
    m.free(bt)
    assert m.num_free_blocks == free0


def test_release_before_is_idempotent():
    m = BlockManager(32, BS)
    bt = m.allocate(100)
    assert m.release_before(bt, 50) == 50 // BS
    snap, free1 = list(bt), m.num_free_blocks
    assert m.release_before(bt, 50) == 0
    assert m.release_before(bt, 17) == 0      # lower than before: nothing
    assert m.release_before(bt, -5) == 0
    assert bt == snap and m.num_free_blocks == free1
    assert all(a is b for a, b in zip(bt, snap))
    assert m.release_before(bt, 10_000) == len(bt) - 50 // BS  # clamps to the table
    assert m.num_free_blocks == 32
    m.free(bt)                                # placeholders are not freed again
    assert m.num_free_blocks == 32


def test_free_keeps_the_real_block_zero_apart_from_placeholders():
    m = BlockManager(4, BS)
    bt = m.allocate(4 * BS)
    assert 0 in [int(b) for b in bt]
    m.release_before(bt, BS)                  # releases bt[0] only
    m.free(bt)
    assert m.num_free_blocks == 4
    assert sorted(m.allocate(4 * BS)) == [0, 1, 2, 3]  # each block once


def test_release_before_with_prefix_caching():
    """A block shared by two sequences survives while either needs it and
    goes back once."""
    m = BlockManager(32, BS, prefix_caching=True)
    free0 = m.num_free_blocks
    prompt = list(range(100, 100 + 5 * BS + 3))
    a, na = m.allocate_with_prefix(prompt)
    assert na == 0
    m.register_prefix(prompt, a)
    b, nb = m.allocate_with_prefix(prompt)
    assert nb == 5 * BS and a[:5] == b[:5]
    shared = a[0]
    m.release_before(a, 2 * BS)               # a lets go of blocks 0 and 1
    assert a[0] is RELEASED and b[0] == shared
    assert shared not in m._evictable and m._refs[shared] >= 1
    # nothing of b's may be handed out while b holds it
    got = m.allocate(BS * m.num_free_blocks)
    assert shared not in got
    m.free(got)
    m.release_before(b, 2 * BS)               # now nobody needs them
    m.release_before(b, 2 * BS)
    m.free(a)
    m.free(b)
    # every block is free or evictable-cached, none counted twice
    assert m.num_free_blocks + len(m._evictable) == free0
    everything = m.allocate(BS * free0)       # evicts the cached ones
    assert sorted(everything) == list(range(32))


def test_register_prefix_stops_at_a_released_block():
    m = BlockManager(32, BS, prefix_caching=True)
    prompt = list(range(7, 7 + 4 * BS + 1))
    bt, _ = m.allocate_with_prefix(prompt)
    m.release_before(bt, 2 * BS)
    m.register_prefix(prompt, bt)
    assert not any(b is RELEASED for b in m._block_key)
    assert 0 not in m._block_key or 0 in [int(b) for b in bt if b is not RELEASED]


# ---------- engine ----------

def _engine(model, chunk=4096, release=True, prefix_caching=False, **kw):
    e = LLMEngine(model=model, device="cpu", dtype=torch.float32, block_size=BS,
                  num_blocks=96, seed=3, prefill_budget=chunk, max_batch_size=4,
                  prefix_caching=prefix_caching, **kw)
    e._swa_release = release
    return e


def _prompt(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 500, (n,), generator=g).tolist()


def _greedy(engine, prompt, max_tokens):
    free0 = engine.kv.manager.num_free_blocks
    peak = 0
    req = EngineRequest(prompt, SamplingParams(max_tokens=max_tokens, ignore_eos=True,
                                               temperature=0.0))
    engine.add_request(req)
    while req.state in ("waiting", "running"):
        engine.step()
        # the prompt's blocks are allocated at admission, as before; the
        # bound is that of a decoding sequence (after its first decode step)
        if len(req.out_ids) >= 2:
            peak = max(peak, sum(b is not RELEASED for b in req.block_table))
    assert req.state == "finished" and len(req.out_ids) == max_tokens
    assert engine.kv.manager.num_free_blocks == free0
    return req.out_ids, peak


def test_engine_window_ids_agree_across_chunking_and_release():
    prompt = _prompt(50)                      # prompt + output cross W = 24
    base, peak = _greedy(_engine("tiny-llama-swa"), prompt, 40)
    chunked, peak_c = _greedy(_engine("tiny-llama-swa", chunk=16), prompt, 40)
    kept, peak_k = _greedy(_engine("tiny-llama-swa", release=False), prompt, 40)
    assert chunked == base
    assert kept == base
    # released: the window; kept: the whole sequence
    assert peak <= math.ceil(W / BS) + 1 and peak_c <= math.ceil(W / BS) + 1
    assert peak_k == math.ceil((50 + 40) / BS)
    # the window matters: full attention decodes something else
    full, _ = _greedy(_engine("tiny-llama"), prompt, 40)
    assert full != base


def test_engine_decode_holds_the_window_only():
    e = _engine("tiny-llama-swa")
    req = EngineRequest(_prompt(10), SamplingParams(max_tokens=150, ignore_eos=True,
                                                    temperature=0.0))
    e.add_request(req)
    while req.state in ("waiting", "running"):
        e.step()
        if req.state == "running":
            assert sum(b is not RELEASED for b in req.block_table) <= math.ceil(W / BS) + 1
    assert len(req.out_ids) == 150


def test_engine_short_prompt_equals_full_attention():
    prompt = _prompt(10, seed=2)              # 10 + 12 tokens stay inside W
    swa, _ = _greedy(_engine("tiny-llama-swa"), prompt, 12)
    full, _ = _greedy(_engine("tiny-llama"), prompt, 12)
    assert swa == full


def test_engine_sliding_window_argument_overrides_the_preset():
    prompt = _prompt(50)
    base, _ = _greedy(_engine("tiny-llama-swa"), prompt, 20)
    same, _ = _greedy(_engine("tiny-llama", sliding_window=W), prompt, 20)
    off, _ = _greedy(_engine("tiny-llama-swa", sliding_window=0), prompt, 20)
    full, _ = _greedy(_engine("tiny-llama"), prompt, 20)
    assert same == base and off == full
    assert _engine("tiny-llama-swa", sliding_window=0).sliding_window == 0


def test_engine_window_batch_with_prefix_caching():
    """Shared prompt prefixes and released blocks together: same ids as
    without the prefix cache, every block back at the end."""
    head = _prompt(40, seed=5)
    prompts = [head + _prompt(9, seed=6), head + _prompt(13, seed=7), head[:33]]

    def run(pc):
        e = _engine("tiny-llama-swa", prefix_caching=pc, chunk=32)
        free0 = e.kv.manager.num_free_blocks
        out = []
        for rnd in range(2):                  # the second round hits the cache
            reqs = [EngineRequest(p, SamplingParams(max_tokens=30, ignore_eos=True,
                                                    temperature=0.0)) for p in prompts]
            for r in reqs:
                e.add_request(r)
            while any(r.state in ("waiting", "running") for r in reqs):
                e.step()
            out.append([r.out_ids for r in reqs])
        m = e.kv.manager
        assert m.num_free_blocks + len(m._evictable) == free0
        return out, m.stats_prefix_hits

    plain, _ = run(False)
    cached, hits = run(True)
    assert hits > 0
    assert cached == plain and plain[0] == plain[1]


# ---------- provider option ----------

def test_provider_sliding_window_parsing():
    p = ProviderDetails(baseUrl="local://mistral-7b-v0.1?sliding_window=1024")
    assert p.engine_spec().sliding_window == 1024
    assert p.engine_spec().model == "mistral-7b-v0.1"
    assert ProviderDetails(baseUrl="local://mistral-7b-v0.1").engine_spec().sliding_window is None
    provs = parse_providers([
        {"swa": {"baseUrl": "local://", "apikey": "",
                 "engine": {"model": "tiny-llama-swa", "sliding_window": 16}}}])
    assert provs["swa"].engine_spec().sliding_window == 16


def test_provider_sliding_window_reaches_engine_and_stats():
    from llmapigateway_amd.engine.registry import EngineRegistry

    reg = EngineRegistry()
    k_none = reg._engine_key(EngineSpec(model="tiny-llama-swa"))
    k_16 = reg._engine_key(EngineSpec(model="tiny-llama-swa", sliding_window=16))
    assert k_none != k_16 and "sw16" in k_16
    try:
        h16 = reg.get_engine(EngineSpec(model="tiny-llama-swa", sliding_window=16))
        hdef = reg.get_engine(EngineSpec(model="tiny-llama-swa"))
        assert h16.engine.sliding_window == 16 and h16.engine.model.window == 16
        assert hdef.engine.sliding_window == W
        rows = {r["engine"]: r for r in reg.stats()}
        assert rows[k_16]["sliding_window"] == 16
        assert rows[k_none]["sliding_window"] == W
    finally:
        for h in list(reg._engines.values()):
            h.stop()
        reg._engines.clear()
