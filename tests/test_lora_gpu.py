"""Multi-LoRA on the GPU: the batched-gather shrink / expand kernels
(csrc/lora.hip), the model forward with mixed adapter rows on all three
weight routes, and the engine through captured decode graphs.

Oracle: the fp32 reference twins in ops.reference, run on the CPU."""

import copy
import dataclasses
import functools

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.models.configs import ModelConfig, get_model_config
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel
from llmapigateway_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 1024  # guard elements on each side
CANARY = 0x5A
# llama-1b regrouped to head_dim 128 (the GPU attention kernels cover no
# other), as tests/test_fp8_weights_gpu.py does, cut to 2 layers
LLAMA_1B = dataclasses.replace(
    get_model_config("llama-1b"), num_heads=16, num_kv_heads=4, head_dim=128,
    num_layers=2,
)
TINY = ModelConfig(
    name="tiny-llama-hd128", hidden_size=256, intermediate_size=512,
    num_layers=2, num_heads=2, num_kv_heads=1, vocab_size=512, head_dim=128,
    rope_theta=10000.0, max_positions=512,
)


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


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
        head = buf[:PAD].view(torch.uint8)
        tail = buf[PAD + numel :].view(torch.uint8)
        assert bool((head == CANARY).all()), f"{name}: guard before tensor clobbered"
        assert bool((tail == CANARY).all()), f"{name}: guard after tensor clobbered"

    return view, check


def _bounds(N, nseg):
    """Unequal segment widths: 2/3 | 1/6 | 1/6 of N (128 | 32 | 32 at 192)."""
    if nseg == 1:
        return (N,)
    assert nseg == 3 and N % 48 == 0
    return (N * 2 // 3, N * 5 // 6, N)


def _run_gpu(x, A, B, ranks, scales, ids, bounds, y0):
    """shrink + expand on the GPU with guards around t and y -> (t, y) on
    the CPU."""
    T, nR = x.shape[0], A.shape[1]
    t, tcheck = _guarded((T, nR), torch.float32)
    y, ycheck = _guarded(tuple(y0.shape), torch.bfloat16, fill=y0.to(DEV))
    d = lambda v: v.to(DEV)
    out_t = ops.lora_shrink(d(x), d(A), d(ranks), d(ids), len(bounds), out=t)
    assert out_t.data_ptr() == t.data_ptr()
    out_y = ops.lora_expand(y, t, d(B), d(ranks), d(scales), d(ids), bounds)
    assert out_y.data_ptr() == y.data_ptr()
    tcheck("lora_shrink t")
    ycheck("lora_expand y")
    return t.cpu(), y.cpu()


def _run_ref(x, A, B, ranks, scales, ids, bounds, y0):
    t = reference.lora_shrink(x, A, ranks, ids, len(bounds))
    y = reference.lora_expand(y0.clone(), t, B, ranks, scales, ids, bounds)
    return t, y


def _written(t, ids, ranks, nseg):
    """Mask of the entries of t the kernel writes: rows with a slot, and
    columns below that slot's rank in every segment."""
    R = t.shape[1] // nseg
    rk = torch.where(ids >= 0, ranks[ids.clamp(min=0).long()], torch.zeros_like(ids))
    return (torch.arange(R).repeat(nseg)[None, :] < rk[:, None])


# ---------- exact: integer data, every product, sum and rounding exact ----------

@functools.lru_cache(maxsize=None)
def _exact_case(T, N, rank, nseg):
    K, S = 64, 3
    R = ops.lora_padded_rank(rank)
    g = torch.Generator(device="cpu").manual_seed(T * 31 + N * 7 + rank * 3 + nseg)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    x = ri(-1, 2, (T, K)).bfloat16()
    # slot s has rank max(1, rank - s): different ranks in one stack
    ranks = torch.tensor([max(1, rank - s) for s in range(S)], dtype=torch.int32)
    A = torch.zeros(S, nseg * R, K)
    B = torch.zeros(S, N, R)
    for s in range(S):
        r = int(ranks[s])
        for seg in range(nseg):
            A[s, seg * R : seg * R + r] = ri(-1, 2, (r, K)).float()
        # one +-1 per row of B, within the slot's rank
        col = ri(0, r, (N,))
        B[s, torch.arange(N), col] = (ri(0, 2, (N,)) * 2 - 1).float()
    scales = torch.tensor([0.5, 1.0, 2.0])[ri(0, 3, (S,))]
    ids = ri(-1, S, (T,)).int()
    if T >= 3:
        ids[0], ids[1], ids[2] = 0, -1, S - 1  # every kind of row is present
    else:
        ids[0] = (rank + N) % S  # a single row is on an adapter
    y0 = ri(-64, 65, (T, N)).bfloat16()
    return x, A.bfloat16(), B.bfloat16(), ranks, scales, ids, _bounds(N, nseg), y0


@pytest.mark.parametrize("rank", [1, 8, 24, 64])
@pytest.mark.parametrize(
    "T,N,nseg",
    [(1, 64, 1), (17, 64, 1), (256, 64, 1), (1, 192, 1), (17, 192, 1),
     (256, 192, 1), (1, 192, 3), (17, 192, 3), (256, 192, 3)],
)
def test_exact_integer_data(T, N, nseg, rank):
    case = _exact_case(T, N, rank, nseg)
    x, A, B, ranks, scales, ids, bounds, y0 = case
    t_ref, y_ref = _run_ref(*case)
    # the fp32 reference is its own bf16 rounding: nothing rounds anywhere
    lo, y64 = 0, y0.double()
    for s, hi in enumerate(bounds):
        R = B.shape[2]
        for slot in range(A.shape[0]):
            rows = ids == slot
            y64[rows, lo:hi] += float(scales[slot]) * (
                x[rows].double() @ A[slot, s * R : (s + 1) * R].double().T
                @ B[slot, lo:hi].double().T
            )
        lo = hi
    assert torch.equal(y64.float().bfloat16().double(), y64)
    assert torch.equal(y_ref.double(), y64)

    t, y = _run_gpu(*case)
    m = _written(t_ref, ids, ranks, len(bounds))
    assert torch.equal(t[m], t_ref[m])
    assert torch.equal(y, y_ref)
    base = ids < 0
    assert torch.equal(y[base].view(torch.int16), y0[base].view(torch.int16))
    # what shrink does not write keeps the canary
    assert bool((t.view(torch.uint8).view(*t.shape, 4)[~m] == CANARY).all())


# ---------- numerics: random data, y0 = 0 so the output is the delta ----------

@functools.lru_cache(maxsize=None)
def _random_stack(N, K, rank, nseg):
    S = 4
    R = ops.lora_padded_rank(rank)
    g = torch.Generator(device="cpu").manual_seed(N * 5 + K + rank)
    ranks = torch.tensor([rank, max(1, rank // 2), max(1, rank - 1), 1], dtype=torch.int32)
    A = torch.zeros(S, nseg * R, K)
    B = torch.zeros(S, N, R)
    for s in range(S):
        r = int(ranks[s])
        for seg in range(nseg):
            A[s, seg * R : seg * R + r] = torch.randn(r, K, generator=g) * 0.02
        B[s, :, :r] = torch.randn(N, r, generator=g) * 0.02
    scales = torch.tensor([2.0, 0.5, 1.0, 16.0])
    return A.bfloat16(), B.bfloat16(), ranks, scales


def _delta_err(got, ref):
    # normalised max error, as _gemm_err of the GEMM tests defines it
    return ((got.float() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()


@pytest.mark.parametrize("T", [1, 7, 200])
@pytest.mark.parametrize("rank", [5, 16, 64])
@pytest.mark.parametrize("N", [64, 192, 6144])
@pytest.mark.parametrize("K", [64, 448, 4096])
def test_numerics_random(K, N, rank, T):
    nseg = 3 if N % 48 == 0 else 1  # q | k | v where N divides that way
    A, B, ranks, scales = _random_stack(N, K, rank, nseg)
    g = torch.Generator(device="cpu").manual_seed(T + N + K)
    x = (torch.randn(T, K, generator=g) * 0.5).bfloat16()
    ids = (torch.arange(T) % 4).int()  # neighbouring rows: different slots
    bounds = _bounds(N, nseg)
    y0 = torch.zeros(T, N).bfloat16()
    t_ref, y_ref = _run_ref(x, A, B, ranks, scales, ids, bounds, torch.zeros(T, N))
    t, y = _run_gpu(x, A, B, ranks, scales, ids, bounds, y0)
    m = _written(t_ref, ids, ranks, nseg)
    t_err = ((t[m] - t_ref[m]).abs().max() / (t_ref.abs().max() + 1e-3)).item()
    err = _delta_err(y, y_ref)
    print(f"T={T} N={N} K={K} rank={rank} nseg={nseg}: t err {t_err:.6f} y err {err:.5f}")
    assert t_err < 0.02
    assert err < 0.02


# ---------- sensitivity ----------

def test_swapping_two_slots_changes_those_rows_only():
    T, N, K, rank, nseg = 17, 192, 448, 16, 3
    A, B, ranks, scales = _random_stack(N, K, rank, nseg)
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(T, K, generator=g) * 0.5).bfloat16()
    y0 = torch.randn(T, N, generator=g).bfloat16()
    ids = (torch.arange(T) % 5 - 1).int()  # -1, 0, 1, 2, 3, -1, ...
    bounds = _bounds(N, nseg)
    _, y1 = _run_gpu(x, A, B, ranks, scales, ids, bounds, y0)
    swapped = ids.clone()
    swapped[2], swapped[9] = ids[9], ids[2]
    assert ids[2] != ids[9]
    _, y2 = _run_gpu(x, A, B, ranks, scales, swapped, bounds, y0)
    changed = (y1.view(torch.int16) != y2.view(torch.int16)).any(dim=1)
    assert changed.nonzero().flatten().tolist() == [2, 9]


def test_one_element_of_A_reaches_its_slot_and_segment_only():
    T, N, K, rank, nseg = 17, 192, 448, 16, 3
    A, B, ranks, scales = _random_stack(N, K, rank, nseg)
    R = B.shape[2]
    g = torch.Generator(device="cpu").manual_seed(4)
    x = (torch.randn(T, K, generator=g) * 0.5).bfloat16()
    y0 = torch.randn(T, N, generator=g).bfloat16()
    ids = (torch.arange(T) % 5 - 1).int()
    bounds = _bounds(N, nseg)
    _, y1 = _run_gpu(x, A, B, ranks, scales, ids, bounds, y0)
    A2 = A.clone()
    A2[2, 1 * R + 3, 100] += 8.0  # slot 2, segment 1
    _, y2 = _run_gpu(x, A2, B, ranks, scales, ids, bounds, y0)
    diff = y1.view(torch.int16) != y2.view(torch.int16)
    rows = diff.any(dim=1).nonzero().flatten().tolist()
    cols = diff.any(dim=0).nonzero().flatten()
    assert rows == (ids == 2).nonzero().flatten().tolist()
    assert len(cols) > 0
    assert int(cols.min()) >= bounds[0] and int(cols.max()) < bounds[1]


def test_rejected_calls():
    A, B, ranks, scales = (v.to(DEV) for v in _random_stack(192, 448, 16, 3))
    x = torch.zeros(4, 448, dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(4, dtype=torch.int32, device=DEV)
    y = torch.zeros(4, 192, dtype=torch.bfloat16, device=DEV)
    t = ops.lora_shrink(x, A, ranks, ids, 3)
    with pytest.raises(RuntimeError):
        ops.lora_shrink(x.float(), A, ranks, ids, 3)
    with pytest.raises(RuntimeError):
        ops.lora_shrink(x, A, ranks, ids.long(), 3)
    with pytest.raises(RuntimeError):
        ops.lora_shrink(x, A, ranks, ids[:3], 3)
    with pytest.raises(ValueError):
        ops.lora_expand(y, t, B, ranks, scales, ids, (128, 160))
    with pytest.raises(RuntimeError):
        ops.lora_expand(y, t, B, ranks, scales, ids, (100, 160, 192))
    with pytest.raises(RuntimeError):
        ops.lora_expand(y, t[:, :16], B, ranks, scales, ids, (128, 160, 192))


# ---------- model forward: mixed decode batch on the three weight routes ----------

ROWS = 17


def _with(model, **attrs):
    m = copy.copy(model)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _cpu_twin(model):
    """The same weights and adapter stacks on the CPU: forward() then runs
    the reference path of every op."""
    cpu = lambda t: t.cpu()
    twin = _with(
        model, device=torch.device("cpu"), embed=cpu(model.embed),
        lm_head=cpu(model.lm_head), final_norm=cpu(model.final_norm),
        cos_sin=cpu(model.cos_sin),
        layers=[
            {k: cpu(v) for k, v in layer.items() if not k.endswith(("_swz", "_int"))}
            for layer in model.layers
        ],
    )
    ranks, scales = cpu(model.lora_ranks), cpu(model.lora_scales)
    twin.lora_ranks, twin.lora_scales = ranks, scales
    twin.lora_layers = [
        {
            name: ops.LoraStack(cpu(st.A), cpu(st.B), ranks, scales, st.seg_bounds)
            for name, st in stacks.items()
        }
        for stacks in model.lora_layers
    ]
    return twin


def _decode_logits(model, ids):
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    dev = model.device
    rows = ROWS
    kv = PagedKVCache(model.config, rows, 16, dev, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(5)
    toks = torch.randint(0, model.config.vocab_size, (rows,), generator=g)
    batch = ForwardBatch(
        kind="decode",
        token_ids=toks.to(dev),
        positions=torch.zeros(rows, dtype=torch.long, device=dev),
        slot_mapping=(torch.arange(rows) * 16).to(dev),
        block_tables=torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1),
        context_lens=torch.ones(rows, dtype=torch.int32, device=dev),
        adapter_ids=None if ids is None else ids.to(dev),
    )
    return model.forward(batch, kv.k_caches, kv.v_caches).float().cpu()


@pytest.mark.parametrize("weight_dtype", ["auto", "fp8", "mxfp4"])
def test_model_forward_mixed_batch(weight_dtype):
    """17-row decode forward of 2-layer llama-1b, rows [a, base, b, a, ...].
    GPU logits against the CPU reference path of the same weights and
    adapters may differ by at most 1.5x what the base model (no adapters,
    same batch) differs by between the two: the two extra bf16 roundings per
    projection add to the error. Both figures are printed
    (profiles/r10_multi_lora.md records them)."""
    model = LlamaModel(
        LLAMA_1B, device=DEV, seed=0, weight_dtype=weight_dtype,
        max_loras=2, max_lora_rank=16,
    )
    model.set_adapter(0, model.random_adapter(16, seed=1), alpha=32.0)
    model.set_adapter(1, model.random_adapter(5, seed=2), alpha=10.0)
    ids = torch.tensor([0, -1, 1, 0] * 5, dtype=torch.int32)[:ROWS]
    twin = _cpu_twin(model)

    base_gpu = _decode_logits(_with(model, max_loras=0), None)
    base_cpu = _decode_logits(_with(twin, max_loras=0), None)
    base_err = (base_gpu - base_cpu).abs().max().item()

    got = _decode_logits(model, ids)
    ref = _decode_logits(twin, ids)
    err = (got - ref).abs().max().item()
    moved = (ref - base_cpu).abs().max().item()
    print(
        f"{weight_dtype}: base gpu-vs-cpu {base_err:.5f}, adapters gpu-vs-cpu "
        f"{err:.5f} (ratio {err / base_err:.3f}); adapters move logits by {moved:.4f}"
    )
    assert base_err > 0
    assert moved > 2 * base_err  # the adapters are not lost in the noise
    # base rows equal the base model's rows on the same (unfused) route
    all_base = _decode_logits(model, torch.full((ROWS,), -1, dtype=torch.int32))
    assert torch.equal(got[ids < 0], all_base[ids < 0])
    assert err <= 1.5 * base_err

    # per-row kernels: rows of adapter a do not see what the other rows use
    all_a = _decode_logits(model, torch.zeros(ROWS, dtype=torch.int32))
    assert torch.equal(got[0], all_a[0]) and torch.equal(got[3], all_a[3])
    assert not torch.equal(got[1], all_a[1])


# ---------- engine: captured decode graphs ----------

def _engine(use_hipgraph, **kw):
    from llmapigateway_amd.engine import LLMEngine

    return LLMEngine(
        model=TINY, device=DEV, dtype=torch.bfloat16, block_size=16,
        num_blocks=64, max_model_len=256, max_batch_size=4, seed=0,
        use_hipgraph=use_hipgraph, admit_min_batch=1, max_loras=2,
        max_lora_rank=16, **kw,
    )


def _run_batch(eng, adapters, max_tokens=17):
    from llmapigateway_amd.engine import EngineRequest, SamplingParams

    reqs = [
        eng.add_request(
            EngineRequest(
                list(range(3 + i, 35 + i)),
                SamplingParams(max_tokens=max_tokens, ignore_eos=True, adapter=a),
            )
        )
        for i, a in enumerate(adapters)
    ]
    while eng.has_work():
        eng.step()
    eng.step()  # deliver the deferred last tokens
    assert all(r.state == "finished" for r in reqs)
    return [r.out_ids for r in reqs]


def test_engine_mixed_batch_graph_equals_eager():
    mix = ["a", None, "b", "a"]
    outs = {}
    for graph in (True, False):
        eng = _engine(graph)
        eng.load_adapter("a", rank=16, alpha=64.0, seed=1)
        eng.load_adapter("b", rank=4, alpha=16.0, seed=2)
        outs[graph] = _run_batch(eng, mix)
        if graph:
            assert eng.stats["graph_steps"] >= 16
            base = _run_batch(eng, [None] * 4)
        else:
            assert eng.graph_runner is None
    assert all(len(o) == 17 for o in outs[True])
    assert outs[True] == outs[False]  # 1 prefill token + 16 decode steps each
    # the adapters show in the tokens
    assert outs[True][0] != base[0] and outs[True][2] != base[2]
    assert outs[True][1] == base[1]


def test_adapter_loaded_after_capture_runs_on_the_captured_graphs():
    eng = _engine(True)
    eng.load_adapter("a", rank=16, alpha=64.0, seed=1)
    eng.graph_runner.capture_all()
    graphs = dict(eng.graph_runner.graphs)
    eng.load_adapter("late", rank=8, alpha=32.0, seed=7)
    got = _run_batch(eng, ["late", "a", None, "late"])
    assert eng.stats["graph_steps"] >= 16
    assert eng.graph_runner.graphs == graphs  # nothing was captured again

    ref = _engine(False)
    ref.load_adapter("a", rank=16, alpha=64.0, seed=1)
    ref.load_adapter("late", rank=8, alpha=32.0, seed=7)
    assert got == _run_batch(ref, ["late", "a", None, "late"])
    assert got[0] != got[2] or got[3] != got[2]
