"""The macro-tile W8A16 decode GEMM (csrc/gemm_w8_m256.hip), its binding,
the ops functions and the opt-in routing (LLMAPI_W8_MACRO_MIN_M).

The kernel tests call the binding with an explicit nf and nsk, so routing
cannot go around the kernel. Shapes are the smallest that reach every path:
MW = 1, 2, 4, 8 waves, ragged last fragments and clamped rows; fewer W
units than waves (nf=4 at 8 waves), one unit per wave and several column
tiles; the prologue and every tail of the 2-buffer, loads-two-ahead
pipeline; even, uneven and empty split-K slices.

Bit-identity with the bf16 macro kernel (gemm_m256, register-staged
variant) on the dequantised weight must hold: both issue the same MFMAs in
the same k order per accumulator with the same slice cuts, e4m3 -> bf16 is
exact, and a power-of-two scale commutes with fp32 rounding at these
magnitudes (tests/test_gemm_stream_gpu.py rests on the same argument).
"""

import dataclasses
import functools

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.models.configs import get_model_config
from llmapigateway_amd.models.llama import ForwardBatch, LlamaModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
PAD = 1024  # guard elements on each side
CANARY = 0x5A
# llama-1b with its heads regrouped to head_dim 128 (see
# tests/test_fp8_weights_gpu.py: the GPU attention kernels cover 128 only)
LLAMA_1B = dataclasses.replace(
    get_model_config("llama-1b"), num_heads=16, num_kv_heads=4, head_dim=128
)

# M=100 (MW=4) is added to the issue's list so every wave count runs
MS = (1, 17, 33, 100, 129, 200, 256)
NS = ((64, 4), (192, 4), (128, 8), (256, 8))
# nsk=1 over 1..5 k64 tiles: prologue only, then every tail of the
# pipeline; K=448 splits 4+3 at nsk=2 and 2+2+2+1 at nsk=4
K_CASES = [(64 * s, 1) for s in (1, 2, 3, 4, 5)] + [(448, 2), (448, 4)]


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


@functools.lru_cache(maxsize=None)
def _weights(N, K):
    """(q_frag, scale, dequantised bf16 [N, K], its bf16 fragment twin, the
    dequantised fp32 [N, K] on the CPU, norm weight); computed once per
    shape and never modified."""
    g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    norm_w = torch.randn(N, generator=g).bfloat16().to(DEV)
    q, s = ops.fp8_quantize_weight(w)  # power-of-two scales
    w_dq = ops.fp8_dequantize_weight(q, s, torch.bfloat16).to(DEV)
    deq = ops.fp8_dequantize_weight(q, s, torch.float32)
    return (
        ops.swizzle_weight_frag_fp8(q).to(DEV), s.to(DEV), w_dq,
        ops.swizzle_weight_frag(w_dq), deq, norm_w,
    )


def _x(M, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 13 + K + seed)
    return (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)


def _residual(M, N, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 17 + N + seed)
    return torch.randn(M, N, generator=g).bfloat16().to(DEV)


def _gemm_err(got, x, deq):
    ref = x.float().cpu() @ deq.T
    return ((got.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()


def _macro(x, qf, s, nf, nsk, ws=None):
    """The binding itself, with a private workspace."""
    M, N = x.shape[0], qf.shape[1] * 16
    y = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    if nsk > 1 and ws is None:
        ws = torch.empty(nsk * M * N, dtype=torch.float32, device=DEV)
    ops._native().gemm_w8_m256(y, x, qf, s, ws, nsk, nf)
    return y


# ---------- 1. bit-identity with the bf16 macro kernel ----------

@pytest.mark.parametrize("M", MS)
def test_bit_identical_to_bf16_macro_kernel(M):
    for N, nf in NS:
        for K, nsk in K_CASES:
            qf, s, _, w_frag, deq, _ = _weights(N, K)
            x = _x(M, K)
            y8 = _macro(x, qf, s, nf, nsk)
            y16 = ops.gemm_m256(x, w_frag, nf=nf, nsk=nsk, variant=1)
            assert torch.equal(y8, y16), (M, N, nf, K, nsk)
            err = _gemm_err(y8, x, deq)
            assert err < 0.02, (M, N, nf, K, nsk, err)


# ---------- 2. empty split-K slice ----------

@pytest.mark.parametrize("M,N,nf", [(17, 192, 4), (200, 128, 8)])
def test_empty_splitk_slice_writes_zeros(M, N, nf):
    K, nsk = 192, 4  # 3 k64 tiles over 4 slices: the fourth has none
    qf, s, _, _, deq, _ = _weights(N, K)
    x = _x(M, K)
    ws = torch.full((nsk * M * N,), float("nan"), dtype=torch.float32, device=DEV)
    y4 = _macro(x, qf, s, nf, nsk, ws)
    y1 = _macro(x, qf, s, nf, 1)
    assert not torch.isnan(y4.float()).any()
    assert not torch.isnan(ws).any(), "every slab is fully written"
    assert bool((ws[3 * M * N :] == 0).all()), "the empty slice writes zeros"
    assert _gemm_err(y4, x, deq) < 0.02
    assert _gemm_err(y1, x, deq) < 0.02
    diff = (y4.float() - y1.float()).abs().max().item()
    assert diff / (y1.float().abs().max().item() + 1e-3) < 0.02


# ---------- 3. exact: integer data, every product and sum exact ----------

@pytest.mark.parametrize("M,N,nf", [(1, 64, 4), (17, 192, 4), (256, 128, 8)])
def test_exact_integer_data(M, N, nf):
    K = 128
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randint(-1, 2, (M, K), generator=g).bfloat16()
    wq = torch.randint(-1, 2, (N, K), generator=g).float()  # |y| <= 256: exact in bf16
    q = wq.to(torch.float8_e4m3fn).view(torch.uint8)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    exact = x.float() @ (wq * scale[:, None]).T
    ref = exact.bfloat16()
    assert torch.equal(ref.float(), exact)
    qf, sc = ops.swizzle_weight_frag_fp8(q).to(DEV), scale.to(DEV)
    for nsk in (1, 2):
        got = _macro(x.to(DEV), qf, sc, nf, nsk)
        assert torch.equal(got.cpu(), ref), nsk


# ---------- 4. fused reduce + residual + norm ----------

@pytest.mark.parametrize(
    "M,N,K,nf,nsk", [(17, 512, 448, 4, 2), (200, 2048, 1024, 8, 4)]
)
def test_fused_tail_bit_identical(M, N, K, nf, nsk):
    qf, s, _, _, _, norm_w = _weights(N, K)
    x, res0 = _x(M, K), _residual(M, N)
    assert ops._reduce_norm_covers(N)

    res_u = res0.clone()
    out_u, res_u = ops.rmsnorm_residual(
        ops.gemm_w8_m256(x, qf, s, nf=nf, nsk=nsk), res_u, norm_w, EPS
    )
    res_f = res0.clone()
    out_f, res_f2 = ops.gemm_w8_m256_rmsnorm_residual(
        x, qf, s, res_f, norm_w, EPS, nf, nsk
    )
    assert res_f2 is res_f
    assert torch.equal(res_f, res_u)
    assert torch.equal(out_f, out_u)


def test_fused_tail_needs_splitk():
    M, N, K = 17, 512, 448
    qf, s, _, _, _, norm_w = _weights(N, K)
    with pytest.raises(ValueError):
        ops.gemm_w8_m256_rmsnorm_residual(
            _x(M, K), qf, s, _residual(M, N), norm_w, EPS, 4, 1
        )


# ---------- 5. guards ----------

def _guarded(shape, dtype):
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.empty(numel + 2 * PAD, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(CANARY)
    view = buf[PAD : PAD + numel].view(shape)

    def check(name):
        torch.cuda.synchronize()
        head = buf[:PAD].view(torch.uint8)
        tail = buf[PAD + numel :].view(torch.uint8)
        assert bool((head == CANARY).all()), f"{name}: guard before tensor clobbered"
        assert bool((tail == CANARY).all()), f"{name}: guard after tensor clobbered"

    return view, check


def test_guards():
    M, N, K = 7, 64, 448
    qf, s, _, _, deq, _ = _weights(N, K)
    x = _x(M, K)
    nat = ops._native()
    y, ycheck = _guarded((M, N), torch.bfloat16)
    nat.gemm_w8_m256(y, x, qf, s, None, 1, 4)
    ycheck("gemm_w8_m256 y")
    assert _gemm_err(y, x, deq) < 0.02

    y2, y2check = _guarded((M, N), torch.bfloat16)
    ws, wcheck = _guarded((2 * M * N,), torch.float32)
    nat.gemm_w8_m256(y2, x, qf, s, ws, 2, 4)
    y2check("gemm_w8_m256 split-K y")
    wcheck("gemm_w8_m256 slab workspace")
    assert _gemm_err(y2, x, deq) < 0.02

    # the fused tail covers N % 512 == 0 only: its guards run at the
    # smallest such width
    N = 512
    qf, s, _, _, _, norm_w = _weights(N, K)
    out, ocheck = _guarded((M, N), torch.bfloat16)
    res, rcheck = _guarded((M, N), torch.bfloat16)
    res.copy_(_residual(M, N))
    ws, wcheck = _guarded((2 * M * N,), torch.float32)
    nat.gemm_w8_m256(out, x, qf, s, ws, 2, 4, res, norm_w, EPS, out)
    ocheck("gemm_w8_m256 fused out")
    rcheck("gemm_w8_m256 fused residual")
    wcheck("gemm_w8_m256 fused slab workspace")
    assert not torch.isnan(out.float()).any()


# ---------- 6. argument validation ----------

def test_argument_validation():
    M, N, K = 7, 64, 448
    qf, s, _, _, _, _ = _weights(N, K)
    qf192, s192 = _weights(192, K)[:2]
    x = _x(M, K)
    nat = ops._native()
    y, ycheck = _guarded((M, N), torch.bfloat16)
    y192, y192check = _guarded((M, 192), torch.bfloat16)

    with pytest.raises(RuntimeError):  # activation dtype
        nat.gemm_w8_m256(y, x.float(), qf, s, None, 1, 4)
    with pytest.raises(RuntimeError):  # weight dtype
        nat.gemm_w8_m256(y, x, qf.view(torch.int8), s, None, 1, 4)
    with pytest.raises(RuntimeError):  # scale dtype
        nat.gemm_w8_m256(y, x, qf, s.double(), None, 1, 4)
    with pytest.raises(RuntimeError):  # K % 64 != 0
        x_bad = torch.zeros(M, K + 32, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w8_m256(y, x_bad, qf, s, None, 1, 4)
    with pytest.raises(RuntimeError):  # nf = 8 needs N % 128 == 0
        nat.gemm_w8_m256(y192, x, qf192, s192, None, 1, 8)
    with pytest.raises(RuntimeError):  # nf = 3
        nat.gemm_w8_m256(y, x, qf, s, None, 1, 3)
    with pytest.raises(RuntimeError):  # short scale
        nat.gemm_w8_m256(y, x, qf, s[: N - 1].contiguous(), None, 1, 4)
    with pytest.raises(RuntimeError):  # short workspace
        ws = torch.zeros(2 * M * N - 1, dtype=torch.float32, device=DEV)
        nat.gemm_w8_m256(y, x, qf, s, ws, 2, 4)
    with pytest.raises(RuntimeError):  # split-K without a workspace
        nat.gemm_w8_m256(y, x, qf, s, None, 2, 4)
    with pytest.raises(RuntimeError):  # M = 257
        x257 = torch.zeros(257, K, dtype=torch.bfloat16, device=DEV)
        y257 = torch.zeros(257, N, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w8_m256(y257, x257, qf, s, None, 1, 4)
    with pytest.raises(RuntimeError):  # fusion request with nsk = 1
        qf512, s512, _, _, _, nw512 = _weights(512, K)
        out, ocheck = _guarded((M, 512), torch.bfloat16)
        nat.gemm_w8_m256(
            out, x, qf512, s512, None, 1, 4, _residual(M, 512), nw512, EPS, out
        )
    # nothing was launched: the outputs still hold their canary bytes
    torch.cuda.synchronize()
    for t in (y, y192, out):
        assert bool((t.view(torch.uint8) == CANARY).all())
    ycheck("rejected calls")
    y192check("rejected calls")
    ocheck("rejected fused call")


# ---------- 7. hipGraph replay ----------

def test_graph_replay():
    M, N, K = 17, 192, 4096
    qf, s, _, _, _, _ = _weights(N, K)
    assert ops._w8_m256_default(M, N, K)["nsk"] > 1  # slabs + reduce in the graph
    x_s = _x(M, K).clone()
    ops.gemm_w8_m256(x_s, qf, s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_s = ops.gemm_w8_m256(x_s, qf, s)
    eager = ops.gemm_w8_m256(x_s, qf, s)
    outs = []
    for _ in range(3):
        graph.replay()
        outs.append(y_s.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert torch.equal(outs[0], eager)
    # a replay follows new inputs
    x2 = _x(M, K, seed=1)
    x_s.copy_(x2)
    graph.replay()
    assert torch.equal(y_s, ops.gemm_w8_m256(x2, qf, s))


# ---------- 8. routing ----------

def _count_calls(monkeypatch):
    """Count calls per binding; macro calls record whether the fusion
    arguments were passed."""
    calls = {"gemm_w8": [], "gemm_w8_m256": [], "dequant_w8": []}
    for name in calls:
        real = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _n=name, _r=real: (calls[_n].append(len(a)), _r(*a))[1],
        )
    return calls


def test_routing(monkeypatch):
    N, K = 2048, 8192
    qf, s, _, _, deq, norm_w = _weights(N, K)
    calls = _count_calls(monkeypatch)

    def reset():
        for v in calls.values():
            v.clear()

    # knob unset: as today
    monkeypatch.delenv("LLMAPI_W8_MACRO_MIN_M", raising=False)
    x200 = _x(200, K)
    ops.linear_w8(x200, qf, s)
    assert len(calls["gemm_w8"]) == 1 and not calls["gemm_w8_m256"]

    monkeypatch.setenv("LLMAPI_W8_MACRO_MIN_M", "64")
    cfg = {"nf": 8, "nsk": 4}
    monkeypatch.setattr(ops, "_w8_m256_config", lambda M, N, K: dict(cfg))

    reset()
    y = ops.linear_w8(x200, qf, s)
    assert len(calls["gemm_w8_m256"]) == 1 and not calls["gemm_w8"]
    assert _gemm_err(y, x200, deq) < 0.02

    # the fused tail: fusion arguments passed, bit-identical to the
    # unfused pair on the same route
    reset()
    res0 = _residual(200, N)
    res_f = res0.clone()
    out_f, _ = ops.linear_w8_rmsnorm_residual(x200, qf, s, res_f, norm_w, EPS)
    assert calls["gemm_w8_m256"] == [11] and not calls["gemm_w8"]
    res_u = res0.clone()
    out_u, _ = ops.rmsnorm_residual(
        ops.gemm_w8_m256(x200, qf, s, **cfg), res_u, norm_w, EPS
    )
    assert torch.equal(out_f, out_u) and torch.equal(res_f, res_u)
    # LLMAPI_NO_DECODE_FUSION keeps the route and drops the fusion
    reset()
    monkeypatch.setenv("LLMAPI_NO_DECODE_FUSION", "1")
    res_n = res0.clone()
    out_n, _ = ops.linear_w8_rmsnorm_residual(x200, qf, s, res_n, norm_w, EPS)
    monkeypatch.delenv("LLMAPI_NO_DECODE_FUSION")
    assert calls["gemm_w8_m256"] == [7] and not calls["gemm_w8"]
    assert torch.equal(out_n, out_u) and torch.equal(res_n, res_u)

    reset()  # below the knob: the streaming kernel
    ops.linear_w8(_x(16, K), qf, s)
    assert len(calls["gemm_w8"]) == 1 and not calls["gemm_w8_m256"]

    reset()  # above 256: dequantise + library
    ops.linear_w8(_x(300, K), qf, s)
    assert len(calls["dequant_w8"]) == 1
    assert not calls["gemm_w8"] and not calls["gemm_w8_m256"]

    reset()  # no table entry: the streaming kernel
    monkeypatch.setattr(ops, "_w8_m256_config", lambda M, N, K: None)
    ops.linear_w8(x200, qf, s)
    ops.linear_w8_rmsnorm_residual(x200, qf, s, res0.clone(), norm_w, EPS)
    assert len(calls["gemm_w8"]) == 2 and not calls["gemm_w8_m256"]


# ---------- 9. model ----------

def _decode_logits(model, rows=16):
    from llmapigateway_amd.engine.kvcache import PagedKVCache

    kv = PagedKVCache(model.config, rows, 16, DEV, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(5)
    ids = torch.randint(0, model.config.vocab_size, (rows,), generator=g)
    batch = ForwardBatch(
        kind="decode",
        token_ids=ids.to(DEV),
        positions=torch.zeros(rows, dtype=torch.long, device=DEV),
        slot_mapping=(torch.arange(rows) * 16).to(DEV),
        block_tables=torch.arange(rows, dtype=torch.int32, device=DEV).view(rows, 1),
        context_lens=torch.ones(rows, dtype=torch.int32, device=DEV),
    )
    return model.forward(batch, kv.k_caches, kv.v_caches)


def test_model_matches_fake_quant(monkeypatch):
    """One 16-row decode forward of llama-1b with every projection on the
    macro kernel. Yardstick and bound are test_fp8_weights_gpu's: the
    max-abs logit difference between two bf16 routes of the same fake-quant
    weights; the fp8 model may sit at most 4x that far from the fake-quant
    model."""
    monkeypatch.delenv("LLMAPI_W8_MACRO_MIN_M", raising=False)
    model = LlamaModel(LLAMA_1B, device=DEV, seed=0)
    model.quantize_weights_(simulate=True)
    sim_twin = _decode_logits(model)

    monkeypatch.setenv("LLMAPI_NO_FRAG_WEIGHTS", "1")
    model.quantize_weights_(simulate=True)
    sim_lib = _decode_logits(model)

    model.quantize_weights_()
    assert model.weight_dtype == "fp8"
    monkeypatch.setenv("LLMAPI_W8_MACRO_MIN_M", "1")
    monkeypatch.setattr(ops, "_w8_m256_config", ops._w8_m256_default)
    calls = _count_calls(monkeypatch)
    fp8 = _decode_logits(model)
    n_layers = len(model.layers)
    assert len(calls["gemm_w8_m256"]) == 4 * n_layers  # qkv, o, gate_up, down
    assert not calls["gemm_w8"] and not calls["dequant_w8"]

    yard = (sim_twin - sim_lib).abs().max().item()
    diff = (fp8 - sim_twin).abs().max().item()
    print(f"yardstick {yard:.5f} fp8-macro-vs-fake-quant {diff:.5f} ratio {diff / yard:.3f}")
    assert yard > 0
    assert diff <= 4 * yard


# ---------- 10. engine ----------

def test_engine_fp8_hipgraph_macro(monkeypatch):
    from llmapigateway_amd.engine import LLMEngine, SamplingParams

    monkeypatch.setenv("LLMAPI_W8_MACRO_MIN_M", "1")
    monkeypatch.setattr(ops, "_w8_m256_config", ops._w8_m256_default)
    calls = _count_calls(monkeypatch)
    eng = LLMEngine(
        model=LLAMA_1B, device=DEV, dtype=torch.bfloat16, block_size=16,
        num_blocks=64, max_model_len=256, max_batch_size=4, seed=0,
        use_hipgraph=True, admit_min_batch=1, weight_dtype="fp8",
    )
    outs = [
        eng.generate(
            list(range(3, 35)), SamplingParams(max_tokens=8, ignore_eos=True)
        ).out_ids
        for _ in range(2)
    ]
    assert len(outs[0]) == 8 and outs[0] == outs[1]
    assert eng.stats["graph_steps"] > 0
    assert calls["gemm_w8_m256"], "the macro kernel must have run"
    assert not calls["gemm_w8"]
