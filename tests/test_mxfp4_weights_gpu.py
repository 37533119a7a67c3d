"""MXFP4 weights on the GPU: the W4A16 decode GEMM (csrc/gemm_w4.hip), its
dequantise kernel, the op-layer routing and the mxfp4 model / engine.

Oracle: ops.reference. MXFP4 dequantisation is exact in bf16 (one mantissa
bit, power-of-two block scales), so `x.float() @ dequant.float().T` is what
the kernel computes up to fp32 accumulation order and the final bf16
rounding — and with one-hot activations it is the dequantised weight itself,
bit for bit."""

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
# llama-1b regrouped to head_dim 128 (the GPU attention kernels cover only
# that), as in test_fp8_weights_gpu.py: every projection shape is the preset's
LLAMA_1B = dataclasses.replace(
    get_model_config("llama-1b"), num_heads=16, num_kv_heads=4, head_dim=128
)
PAD = 1024  # guard elements on each side
CANARY = 0x5A


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


def _to_dev(packed, scale):
    qf, sf = ops.reference.swizzle_weight_frag_mxfp4(packed, scale)
    return qf.to(DEV), sf.to(DEV)


@functools.lru_cache(maxsize=None)
def _weights(N, K):
    """(q_frag, s_frag, dequantised fp32 [N, K] on the CPU, norm weight)."""
    g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    norm_w = torch.randn(N, generator=g).bfloat16().to(DEV)
    q, s = ops.reference.mxfp4_quantize_weight(w)
    deq = ops.reference.mxfp4_dequantize_weight(q, s, torch.float32)
    return (*_to_dev(q, s), deq, norm_w)


def _x(M, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 13 + K + seed)
    return (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)


def _residual(M, N, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 17 + N + seed)
    return torch.randn(M, N, generator=g).bfloat16().to(DEV)


def _gemm_err(got, x, deq):
    ref = x.float().cpu() @ deq.T
    return ((got.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()


# ---------- identity probe: one wrong nibble or scale fails it ----------

@functools.lru_cache(maxsize=None)
def _probe_weights(N, K):
    """Random nibbles; scale bytes in [120, 134] that differ between any two
    blocks a layout slip could confuse: neighbours along k (+4 mod 15), rows
    1, 16 and 64 apart (+7, +7 and +13 mod 15)."""
    g = torch.Generator(device="cpu").manual_seed(N * 3 + K)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    n = torch.arange(N).view(N, 1)
    kb = torch.arange(K // 32).view(1, K // 32)
    scale = (120 + (n * 7 + kb * 4) % 15).to(torch.uint8)
    deq = ops.reference.mxfp4_dequantize_weight(packed, scale, torch.bfloat16)
    return (*_to_dev(packed, scale), deq)


@pytest.mark.parametrize("nsk", [None, 2])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_identity_probe(K, N, nsk):
    """X = I_K: every output is one exact product, y == dequant.T."""
    qf, sf, deq = _probe_weights(N, K)
    x = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    if nsk is not None and nsk > K // 64:
        # one k64 step cannot be split; the binding says so before any launch
        with pytest.raises(RuntimeError):
            ops.linear_w4(x, qf, sf, nsk=nsk)
        return
    y = ops.linear_w4(x, qf, sf, nsk=nsk)
    bad = (y.cpu() != deq.T).nonzero()
    assert torch.equal(y.cpu(), deq.T), (
        f"{len(bad)} wrong outputs, first (k, n) = {bad[0].tolist()}: "
        f"got {y[bad[0][0], bad[0][1]].item()} want {deq[bad[0][1], bad[0][0]].item()}"
    )


# ---------- exact: integer data, every product and sum exact ----------

@pytest.mark.parametrize("M,N", [(1, 64), (17, 192), (256, 64)])
def test_exact_integer_data(M, N):
    K = 128
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randint(-1, 2, (M, K), generator=g).bfloat16()
    e = torch.randint(-1, 2, (N, K), generator=g)  # elements in {-1, 0, 1}
    code = torch.tensor([0xA, 0x0, 0x2], dtype=torch.uint8)[e + 1]  # -1, 0, 1
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    sbyte = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    assert len(sbyte.unique()) == 3  # block scales 0.5, 1, 2
    w = e.float() * torch.ldexp(torch.ones(N, K // 32), sbyte.int() - 127).repeat_interleave(32, 1)
    assert torch.equal(ops.reference.mxfp4_dequantize_weight(packed, sbyte, torch.float32), w)
    ref = (x.float() @ w.T).bfloat16()  # |y| <= 256: exact in bf16
    assert torch.equal(ref.float(), x.float() @ w.T)
    got = ops.linear_w4(x.to(DEV), *_to_dev(packed, sbyte))
    assert torch.equal(got.cpu(), ref)


# ---------- numerics ----------

@pytest.mark.parametrize("M", [1, 7, 17, 200, 256])
def test_numerics_m(M):
    N, K = 192, 448
    qf, sf, deq, _ = _weights(N, K)
    x = _x(M, K)
    err = _gemm_err(ops.linear_w4(x, qf, sf), x, deq)
    print(f"M={M} N={N} K={K}: err {err:.5f}")
    assert err < 0.02


@pytest.mark.parametrize("steps", range(1, 10))
def test_numerics_pipeline_tails(steps):
    M, N, K = 16, 64, 64 * steps
    qf, sf, deq, _ = _weights(N, K)
    x = _x(M, K)
    assert ops._w4_nsk(N, K) == 1  # one slice: `steps` k64 steps in one pipeline
    err = _gemm_err(ops.linear_w4(x, qf, sf), x, deq)
    print(f"K={K}: err {err:.5f}")
    assert err < 0.02


@pytest.mark.parametrize(
    "M,N,K,nsk", [(17, 192, 448, 2), (16, 64, 4096, None), (16, 2048, 8192, None)]
)
def test_numerics_splitk(M, N, K, nsk):
    # K=448 at nsk=2 splits 7 k64 steps 4+3; (64, 4096) takes the default
    # nsk=8; (2048, 8192) is the llama-1b down projection
    qf, sf, deq, _ = _weights(N, K)
    x = _x(M, K)
    if nsk is None:
        assert ops._w4_nsk(N, K) > 1
    err = _gemm_err(ops.linear_w4(x, qf, sf, nsk=nsk), x, deq)
    print(f"M={M} N={N} K={K} nsk={nsk or ops._w4_nsk(N, K)}: err {err:.5f}")
    assert err < 0.02


def test_large_m_dequant_route(monkeypatch):
    M, N, K = 300, 192, 448
    qf, sf, deq, _ = _weights(N, K)
    x = _x(M, K)
    calls = []
    real = ops._native().dequant_w4
    monkeypatch.setattr(
        ops._C, "dequant_w4", lambda *a: (calls.append(1), real(*a))[1]
    )
    got = ops.linear_w4(x, qf, sf)
    assert calls, "M > 256 must dequantise and call the library"
    # the dequantised bf16 matrix itself is exact
    assert torch.equal(ops.dequant_w4(qf, sf).float().cpu(), deq)
    err = _gemm_err(got, x, deq)
    print(f"M={M}: err {err:.5f}")
    assert err < 0.02


# ---------- fused reduce + residual + norm ----------

@pytest.mark.parametrize("M,N,K", [(16, 512, 4096), (200, 2048, 8192)])
def test_fused_reduce_norm_bit_identical(M, N, K, monkeypatch):
    qf, sf, _, norm_w = _weights(N, K)
    x, res0 = _x(M, K), _residual(M, N)
    assert ops._w4_nsk(N, K) > 1 and ops._reduce_norm_covers(N)

    res_u = res0.clone()
    out_u, res_u = ops.rmsnorm_residual(ops.linear_w4(x, qf, sf), res_u, norm_w, EPS)

    fused = []
    real = ops._native().gemm_w4
    monkeypatch.setattr(
        ops._C, "gemm_w4", lambda *a: (fused.append(len(a) > 6), real(*a))[1]
    )
    res_f = res0.clone()
    out_f, res_f2 = ops.linear_w4_rmsnorm_residual(x, qf, sf, res_f, norm_w, EPS)
    assert fused == [True], "the fused reduce+norm path must have run"
    assert res_f2 is res_f
    assert torch.equal(res_f, res_u)
    assert torch.equal(out_f, out_u)

    # LLMAPI_NO_DECODE_FUSION=1 forces the unfused pair
    fused.clear()
    monkeypatch.setenv("LLMAPI_NO_DECODE_FUSION", "1")
    res_n = res0.clone()
    out_n, _ = ops.linear_w4_rmsnorm_residual(x, qf, sf, res_n, norm_w, EPS)
    assert fused == [False]
    assert torch.equal(out_n, out_u) and torch.equal(res_n, res_u)


# ---------- guards ----------

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
    M, N, K, nsk = 7, 64, 448, 2
    qf, sf, deq, _ = _weights(N, K)
    x = _x(M, K)
    y, ycheck = _guarded((M, N), torch.bfloat16)
    ops._native().gemm_w4(y, x, qf, sf, None, 1)
    ycheck("gemm_w4 y")
    assert _gemm_err(y, x, deq) < 0.02

    y2, y2check = _guarded((M, N), torch.bfloat16)
    ws, wcheck = _guarded((nsk * M * N,), torch.float32)
    ops._native().gemm_w4(y2, x, qf, sf, ws, nsk)
    y2check("gemm_w4 split-K y")
    wcheck("gemm_w4 slab workspace")
    assert _gemm_err(y2, x, deq) < 0.02

    buf, bcheck = _guarded((N, K), torch.bfloat16)
    ops._native().dequant_w4(buf, qf, sf)
    bcheck("dequant_w4 out")
    assert torch.equal(buf.float().cpu(), deq)


# ---------- hipGraph replay ----------

def test_graph_replay():
    M, N, K = 17, 192, 4096
    qf, sf, deq, _ = _weights(N, K)
    assert ops._w4_nsk(N, K) > 1  # slab workspace + reduce in the graph
    x_s = _x(M, K).clone()
    ops.linear_w4(x_s, qf, sf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_s = ops.linear_w4(x_s, qf, sf)
    eager = ops.linear_w4(x_s, qf, sf)
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
    assert torch.equal(y_s, ops.linear_w4(x2, qf, sf))


# ---------- argument validation ----------

def test_argument_validation():
    M, N, K = 7, 64, 448
    qf, sf, _, _ = _weights(N, K)
    x = _x(M, K)
    nat = ops._native()
    y, ycheck = _guarded((M, N), torch.bfloat16)

    with pytest.raises(RuntimeError):  # activation dtype
        nat.gemm_w4(y, x.float(), qf, sf, None, 1)
    with pytest.raises(RuntimeError):  # weight dtype
        nat.gemm_w4(y, x, qf.view(torch.int8), sf, None, 1)
    with pytest.raises(RuntimeError):  # scale dtype
        nat.gemm_w4(y, x, qf, sf.float(), None, 1)
    with pytest.raises(RuntimeError):  # K % 64 != 0
        x_bad = torch.zeros(M, K + 32, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w4(y, x_bad, qf, sf, None, 1)
    with pytest.raises(RuntimeError):  # short scale: one k64 plane missing
        nat.gemm_w4(y, x, qf, sf[:-1].contiguous(), None, 1)
    with pytest.raises(RuntimeError):  # short scale: flat and one byte short
        nat.gemm_w4(y, x, qf, sf.flatten()[:-1].contiguous(), None, 1)
    with pytest.raises(RuntimeError):  # fp8-shaped weight fragments
        nat.gemm_w4(y, x, torch.zeros(K // 64, N // 16, 64, 16, dtype=torch.uint8, device=DEV), sf, None, 1)
    with pytest.raises(RuntimeError):  # short workspace
        ws = torch.zeros(2 * M * N - 1, dtype=torch.float32, device=DEV)
        nat.gemm_w4(y, x, qf, sf, ws, 2)
    with pytest.raises(RuntimeError):  # M = 257
        x257 = torch.zeros(257, K, dtype=torch.bfloat16, device=DEV)
        y257 = torch.zeros(257, N, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w4(y257, x257, qf, sf, None, 1)
    with pytest.raises(RuntimeError):  # dequant target of the wrong dtype
        nat.dequant_w4(torch.zeros(N, K, dtype=torch.float16, device=DEV), qf, sf)
    # nothing was launched: y still holds its canary bytes
    torch.cuda.synchronize()
    assert bool((y.view(torch.uint8) == CANARY).all())
    ycheck("rejected calls")


# ---------- model: mxfp4 kernels against fake-quant on the bf16 kernels ----------

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
    """One 16-row decode forward of llama-1b. Yardstick: the max-abs logit
    difference between two bf16 routes of the SAME fake-quant weights
    (fragment-twin kernels vs LLMAPI_NO_FRAG_WEIGHTS=1); the mxfp4 model may
    sit at most 4x that far from the fake-quant model.

    Measured: yardstick 0.0, mxfp4 vs fake-quant 0.0. A bf16 activation times
    a weight with a 2-bit significand is exact in fp32 and so, nearly always,
    are the sums, so the accumulation order of the three routes does not
    show and the bound asks for bit-identical logits."""
    model = LlamaModel(LLAMA_1B, device=DEV, seed=0)
    model.quantize_weights_("mxfp4", simulate=True)
    assert any(k.endswith("_swz") for k in model.layers[0])
    sim_twin = _decode_logits(model)

    monkeypatch.setenv("LLMAPI_NO_FRAG_WEIGHTS", "1")
    model.quantize_weights_("mxfp4", simulate=True)  # same values again, twins dropped
    assert not any(k.endswith(("_swz", "_int")) for k in model.layers[0])
    sim_lib = _decode_logits(model)

    # quantising the dequantised values again gives the same values (a block
    # whose largest element rounded down to 3 takes the next scale down,
    # where all its elements still sit on the grid)
    model.quantize_weights_("mxfp4")
    assert model.weight_dtype == "mxfp4" and "qkv" not in model.layers[0]
    calls = []
    real = ops._native().gemm_w4
    monkeypatch.setattr(ops._C, "gemm_w4", lambda *a: (calls.append(1), real(*a))[1])
    mx = _decode_logits(model)
    assert len(calls) == 4 * len(model.layers), "every projection runs gemm_w4"
    assert bool(torch.isfinite(mx).all()) and mx.abs().max().item() > 1e-3

    yard = (sim_twin - sim_lib).abs().max().item()
    diff = (mx - sim_twin).abs().max().item()
    print(f"yardstick {yard:.6f} mxfp4-vs-fake-quant {diff:.6f}")
    assert diff <= 4 * yard


# ---------- engine ----------

def test_engine_mxfp4_hipgraph():
    from llmapigateway_amd.engine import LLMEngine, SamplingParams

    eng = LLMEngine(
        model=LLAMA_1B, device=DEV, dtype=torch.bfloat16, block_size=16,
        num_blocks=64, max_model_len=256, max_batch_size=4, seed=0,
        use_hipgraph=True, admit_min_batch=1, weight_dtype="mxfp4",
    )
    assert eng.weight_dtype == "mxfp4" and "qkv_q4" in eng.model.layers[0]
    outs = [
        eng.generate(
            list(range(3, 35)), SamplingParams(max_tokens=8, ignore_eos=True)
        ).out_ids
        for _ in range(2)
    ]
    assert len(outs[0]) == 8 and outs[0] == outs[1]
    assert eng.stats["graph_steps"] > 0
    fp8_model = LlamaModel(LLAMA_1B, device=DEV, seed=0, weight_dtype="fp8")
    assert eng.model.param_bytes() < fp8_model.param_bytes()
