"""The macro-tile W4A16 decode GEMM (csrc/gemm_w4_m256.hip), its binding,
the ops functions and the opt-in routing (LLMAPI_W4_MACRO_MIN_M).

The kernel tests call the binding with an explicit nf and nsk, so routing
cannot go around the kernel. Shapes are the smallest that reach every path:
MW = 1, 2, 4, 8 waves, ragged last fragments and clamped rows; fewer W
units than waves (nf=4 at 8 waves), one unit per wave and several column
tiles; a column tile that starts in scale group 2 (N=192 at nf=4) and a
stripe that spans two scale groups (nf=8); the prologue and every tail of
the 2-buffer, loads-two-ahead pipeline; even, uneven and empty split-K
slices.

Bit-identity with the bf16 macro kernel (gemm_m256, register-staged
variant) on the dequantised weight must hold: MXFP4 -> bf16 is exact with
the block scale applied, and both kernels issue the same MFMAs in the same
k order per accumulator with the same slice cuts. No scale commutes with
anything here: the accumulator takes no scale.
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
# tests/test_mxfp4_weights_gpu.py: the GPU attention kernels cover 128 only)
LLAMA_1B = dataclasses.replace(
    get_model_config("llama-1b"), num_heads=16, num_kv_heads=4, head_dim=128
)

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


def _to_dev(packed, scale):
    qf, sf = ops.reference.swizzle_weight_frag_mxfp4(packed, scale)
    return qf.to(DEV), sf.to(DEV)


@functools.lru_cache(maxsize=None)
def _weights(N, K):
    """(q_frag, s_frag, the bf16 fragment twin of the dequantised weight,
    the dequantised fp32 [N, K] on the CPU, norm weight); computed once per
    shape and never modified."""
    g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    norm_w = torch.randn(N, generator=g).bfloat16().to(DEV)
    q, s = ops.reference.mxfp4_quantize_weight(w)
    deq = ops.reference.mxfp4_dequantize_weight(q, s, torch.float32)
    w_dq = ops.reference.mxfp4_dequantize_weight(q, s, torch.bfloat16).to(DEV)
    assert torch.equal(w_dq.float().cpu(), deq)  # exact in bf16
    return (*_to_dev(q, s), ops.swizzle_weight_frag(w_dq), deq, norm_w)


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


def _x(M, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 13 + K + seed)
    return (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)


def _residual(M, N, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 17 + N + seed)
    return torch.randn(M, N, generator=g).bfloat16().to(DEV)


def _gemm_err(got, x, deq):
    ref = x.float().cpu() @ deq.T
    return ((got.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-3)).item()


def _macro(x, qf, sf, nf, nsk, ws=None):
    """The binding itself, with a private workspace."""
    M, N = x.shape[0], qf.shape[1] * 16
    y = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    if nsk > 1 and ws is None:
        ws = torch.empty(nsk * M * N, dtype=torch.float32, device=DEV)
    ops._native().gemm_w4_m256(y, x, qf, sf, ws, nsk, nf)
    return y


# ---------- 1. identity probe: one wrong nibble, scale, half or group ----------

@pytest.mark.parametrize("nsk", [1, 2])
@pytest.mark.parametrize("K", [64, 128, 192, 256])
def test_identity_probe(K, nsk):
    """X = I_K (M = K: MW = 2, 4, 8, 8): every output is one exact product,
    y == dequant.T. At K = 64 and nsk = 2 the second slice is empty."""
    x = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    for N, nf in NS:
        qf, sf, deq = _probe_weights(N, K)
        y = _macro(x, qf, sf, nf, nsk).cpu()
        bad = (y != deq.T).nonzero()
        assert torch.equal(y, deq.T), (
            f"N={N} nf={nf}: {len(bad)} wrong outputs, first (k, n) = "
            f"{bad[0].tolist()}: got {y[bad[0][0], bad[0][1]].item()} "
            f"want {deq[bad[0][1], bad[0][0]].item()}"
        )


# ---------- 2. bit-identity with the bf16 macro kernel ----------

@pytest.mark.parametrize("M", MS)
def test_bit_identical_to_bf16_macro_kernel(M):
    for N, nf in NS:
        for K, nsk in K_CASES:
            qf, sf, w_frag, deq, _ = _weights(N, K)
            x = _x(M, K)
            y4 = _macro(x, qf, sf, nf, nsk)
            y16 = ops.gemm_m256(x, w_frag, nf=nf, nsk=nsk, variant=1)
            assert torch.equal(y4, y16), (M, N, nf, K, nsk)
            err = _gemm_err(y4, x, deq)
            assert err < 0.02, (M, N, nf, K, nsk, err)


# ---------- 3. empty split-K slice ----------

@pytest.mark.parametrize("M,N,nf", [(17, 192, 4), (200, 128, 8)])
def test_empty_splitk_slice_writes_zeros(M, N, nf):
    K, nsk = 192, 4  # 3 k64 tiles over 4 slices: the fourth has none
    qf, sf, _, deq, _ = _weights(N, K)
    x = _x(M, K)
    ws = torch.full((nsk * M * N,), float("nan"), dtype=torch.float32, device=DEV)
    y4 = _macro(x, qf, sf, nf, nsk, ws)
    y1 = _macro(x, qf, sf, nf, 1)
    assert not torch.isnan(y4.float()).any()
    assert not torch.isnan(ws).any(), "every slab is fully written"
    assert bool((ws[3 * M * N :] == 0).all()), "the empty slice writes zeros"
    assert _gemm_err(y4, x, deq) < 0.02
    assert _gemm_err(y1, x, deq) < 0.02
    diff = (y4.float() - y1.float()).abs().max().item()
    assert diff / (y1.float().abs().max().item() + 1e-3) < 0.02


# ---------- 4. exact: integer data, every product and sum exact ----------

@pytest.mark.parametrize("M,N,nf", [(1, 64, 4), (17, 192, 4), (256, 128, 8)])
def test_exact_integer_data(M, N, nf):
    K = 128
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randint(-1, 2, (M, K), generator=g).bfloat16()
    e = torch.randint(-1, 2, (N, K), generator=g)  # elements in {-1, 0, 1}
    code = torch.tensor([0xA, 0x0, 0x2], dtype=torch.uint8)[e + 1]  # -1, 0, 1
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    sbyte = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    assert len(sbyte.unique()) == 3  # block scales 0.5, 1, 2
    w = e.float() * torch.ldexp(
        torch.ones(N, K // 32), sbyte.int() - 127
    ).repeat_interleave(32, 1)
    assert torch.equal(
        ops.reference.mxfp4_dequantize_weight(packed, sbyte, torch.float32), w
    )
    exact = x.float() @ w.T
    ref = exact.bfloat16()  # |y| <= 256: exact in bf16
    assert torch.equal(ref.float(), exact)
    qf, sf = _to_dev(packed, sbyte)
    for nsk in (1, 2):
        got = _macro(x.to(DEV), qf, sf, nf, nsk)
        assert torch.equal(got.cpu(), ref), nsk


# ---------- 5. fused reduce + residual + norm ----------

@pytest.mark.parametrize(
    "M,N,K,nf,nsk", [(17, 512, 448, 4, 2), (200, 2048, 1024, 8, 4)]
)
def test_fused_tail_bit_identical(M, N, K, nf, nsk):
    qf, sf, _, _, norm_w = _weights(N, K)
    x, res0 = _x(M, K), _residual(M, N)
    assert ops._reduce_norm_covers(N)

    res_u = res0.clone()
    out_u, res_u = ops.rmsnorm_residual(
        ops.gemm_w4_m256(x, qf, sf, nf=nf, nsk=nsk), res_u, norm_w, EPS
    )
    res_f = res0.clone()
    out_f, res_f2 = ops.gemm_w4_m256_rmsnorm_residual(
        x, qf, sf, res_f, norm_w, EPS, nf, nsk
    )
    assert res_f2 is res_f
    assert torch.equal(res_f, res_u)
    assert torch.equal(out_f, out_u)


def test_fused_tail_needs_splitk():
    M, N, K = 17, 512, 448
    qf, sf, _, _, norm_w = _weights(N, K)
    with pytest.raises(ValueError):
        ops.gemm_w4_m256_rmsnorm_residual(
            _x(M, K), qf, sf, _residual(M, N), norm_w, EPS, 4, 1
        )


# ---------- 6. guards ----------

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
    qf, sf, _, deq, _ = _weights(N, K)
    x = _x(M, K)
    nat = ops._native()
    y, ycheck = _guarded((M, N), torch.bfloat16)
    nat.gemm_w4_m256(y, x, qf, sf, None, 1, 4)
    ycheck("gemm_w4_m256 y")
    assert _gemm_err(y, x, deq) < 0.02

    y2, y2check = _guarded((M, N), torch.bfloat16)
    ws, wcheck = _guarded((2 * M * N,), torch.float32)
    nat.gemm_w4_m256(y2, x, qf, sf, ws, 2, 4)
    y2check("gemm_w4_m256 split-K y")
    wcheck("gemm_w4_m256 slab workspace")
    assert _gemm_err(y2, x, deq) < 0.02

    # the fused tail covers N % 512 == 0 only: its guards run at the
    # smallest such width
    N = 512
    qf, sf, _, _, norm_w = _weights(N, K)
    out, ocheck = _guarded((M, N), torch.bfloat16)
    res, rcheck = _guarded((M, N), torch.bfloat16)
    res.copy_(_residual(M, N))
    ws, wcheck = _guarded((2 * M * N,), torch.float32)
    nat.gemm_w4_m256(out, x, qf, sf, ws, 2, 4, res, norm_w, EPS, out)
    ocheck("gemm_w4_m256 fused out")
    rcheck("gemm_w4_m256 fused residual")
    wcheck("gemm_w4_m256 fused slab workspace")
    assert not torch.isnan(out.float()).any()


# ---------- 7. argument validation ----------

def test_argument_validation():
    M, N, K = 7, 64, 448
    qf, sf = _weights(N, K)[:2]
    qf192, sf192 = _weights(192, K)[:2]
    x = _x(M, K)
    nat = ops._native()
    y, ycheck = _guarded((M, N), torch.bfloat16)
    y192, y192check = _guarded((M, 192), torch.bfloat16)

    with pytest.raises(RuntimeError):  # activation dtype
        nat.gemm_w4_m256(y, x.float(), qf, sf, None, 1, 4)
    with pytest.raises(RuntimeError):  # weight dtype
        nat.gemm_w4_m256(y, x, qf.view(torch.int8), sf, None, 1, 4)
    with pytest.raises(RuntimeError):  # scale dtype
        nat.gemm_w4_m256(y, x, qf, sf.float(), None, 1, 4)
    with pytest.raises(RuntimeError):  # K % 64 != 0
        x_bad = torch.zeros(M, K + 32, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w4_m256(y, x_bad, qf, sf, None, 1, 4)
    with pytest.raises(RuntimeError):  # nf = 8 needs N % 128 == 0
        nat.gemm_w4_m256(y192, x, qf192, sf192, None, 1, 8)
    with pytest.raises(RuntimeError):  # nf = 3
        nat.gemm_w4_m256(y, x, qf, sf, None, 1, 3)
    with pytest.raises(RuntimeError):  # short scale: one k64 plane missing
        nat.gemm_w4_m256(y, x, qf, sf[:-1].contiguous(), None, 1, 4)
    with pytest.raises(RuntimeError):  # mis-shaped scale: flat, one byte short
        nat.gemm_w4_m256(y, x, qf, sf.flatten()[:-1].contiguous(), None, 1, 4)
    with pytest.raises(RuntimeError):  # short workspace
        ws = torch.zeros(2 * M * N - 1, dtype=torch.float32, device=DEV)
        nat.gemm_w4_m256(y, x, qf, sf, ws, 2, 4)
    with pytest.raises(RuntimeError):  # split-K without a workspace
        nat.gemm_w4_m256(y, x, qf, sf, None, 2, 4)
    with pytest.raises(RuntimeError):  # M = 257
        x257 = torch.zeros(257, K, dtype=torch.bfloat16, device=DEV)
        y257 = torch.zeros(257, N, dtype=torch.bfloat16, device=DEV)
        nat.gemm_w4_m256(y257, x257, qf, sf, None, 1, 4)
    with pytest.raises(RuntimeError):  # fusion request with nsk = 1
        qf512, sf512, _, _, nw512 = _weights(512, K)
        out, ocheck = _guarded((M, 512), torch.bfloat16)
        nat.gemm_w4_m256(
            out, x, qf512, sf512, None, 1, 4, _residual(M, 512), nw512, EPS, out
        )
    # nothing was launched: the outputs still hold their canary bytes
    torch.cuda.synchronize()
    for t in (y, y192, out):
        assert bool((t.view(torch.uint8) == CANARY).all())
    ycheck("rejected calls")
    y192check("rejected calls")
    ocheck("rejected fused call")


# ---------- 8. hipGraph replay ----------

def test_graph_replay():
    M, N, K = 17, 192, 4096
    qf, sf = _weights(N, K)[:2]
    assert ops._w4_m256_default(M, N, K)["nsk"] > 1  # slabs + reduce in the graph
    x_s = _x(M, K).clone()
    ops.gemm_w4_m256(x_s, qf, sf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_s = ops.gemm_w4_m256(x_s, qf, sf)
    eager = ops.gemm_w4_m256(x_s, qf, sf)
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
    assert torch.equal(y_s, ops.gemm_w4_m256(x2, qf, sf))


# ---------- 9. routing ----------

def _count_calls(monkeypatch):
    """Count calls per binding; macro calls record whether the fusion
    arguments were passed."""
    calls = {"gemm_w4": [], "gemm_w4_m256": [], "dequant_w4": []}
    for name in calls:
        real = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _n=name, _r=real: (calls[_n].append(len(a)), _r(*a))[1],
        )
    return calls


def test_routing(monkeypatch):
    N, K = 2048, 8192
    qf, sf, _, deq, norm_w = _weights(N, K)
    calls = _count_calls(monkeypatch)

    def reset():
        for v in calls.values():
            v.clear()

    # knob unset: as today, nothing reaches the new binding
    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M", raising=False)
    x200 = _x(200, K)
    res0 = _residual(200, N)
    ops.linear_w4(x200, qf, sf)
    ops.linear_w4_rmsnorm_residual(x200, qf, sf, res0.clone(), norm_w, EPS)
    assert len(calls["gemm_w4"]) == 2 and not calls["gemm_w4_m256"]

    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "64")
    cfg = {"nf": 8, "nsk": 4}
    monkeypatch.setattr(ops, "_w4_m256_config", lambda M, N, K: dict(cfg))

    reset()
    y = ops.linear_w4(x200, qf, sf)
    assert len(calls["gemm_w4_m256"]) == 1 and not calls["gemm_w4"]
    assert _gemm_err(y, x200, deq) < 0.02

    # the fused tail: fusion arguments passed, bit-identical to the
    # unfused pair on the same route
    reset()
    res_f = res0.clone()
    out_f, _ = ops.linear_w4_rmsnorm_residual(x200, qf, sf, res_f, norm_w, EPS)
    assert calls["gemm_w4_m256"] == [11] and not calls["gemm_w4"]
    res_u = res0.clone()
    out_u, _ = ops.rmsnorm_residual(
        ops.gemm_w4_m256(x200, qf, sf, **cfg), res_u, norm_w, EPS
    )
    assert torch.equal(out_f, out_u) and torch.equal(res_f, res_u)
    # LLMAPI_NO_DECODE_FUSION keeps the route and drops the fusion
    reset()
    monkeypatch.setenv("LLMAPI_NO_DECODE_FUSION", "1")
    res_n = res0.clone()
    out_n, _ = ops.linear_w4_rmsnorm_residual(x200, qf, sf, res_n, norm_w, EPS)
    monkeypatch.delenv("LLMAPI_NO_DECODE_FUSION")
    assert calls["gemm_w4_m256"] == [7] and not calls["gemm_w4"]
    assert torch.equal(out_n, out_u) and torch.equal(res_n, res_u)

    reset()  # below the knob: the streaming kernel
    ops.linear_w4(_x(16, K), qf, sf)
    assert len(calls["gemm_w4"]) == 1 and not calls["gemm_w4_m256"]

    reset()  # above 256: dequantise + library
    ops.linear_w4(_x(300, K), qf, sf)
    assert len(calls["dequant_w4"]) == 1
    assert not calls["gemm_w4"] and not calls["gemm_w4_m256"]

    reset()  # no table entry: the streaming kernel
    monkeypatch.setattr(ops, "_w4_m256_config", lambda M, N, K: None)
    ops.linear_w4(x200, qf, sf)
    ops.linear_w4_rmsnorm_residual(x200, qf, sf, res0.clone(), norm_w, EPS)
    assert len(calls["gemm_w4"]) == 2 and not calls["gemm_w4_m256"]


# ---------- 10. model ----------

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
    macro kernel. Yardstick and bound are test_mxfp4_weights_gpu's: the
    max-abs logit difference between two bf16 routes of the same fake-quant
    weights; the mxfp4 model may sit at most 4x that far from the
    fake-quant model."""
    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M", raising=False)
    model = LlamaModel(LLAMA_1B, device=DEV, seed=0)
    model.quantize_weights_("mxfp4", simulate=True)
    sim_twin = _decode_logits(model)

    monkeypatch.setenv("LLMAPI_NO_FRAG_WEIGHTS", "1")
    model.quantize_weights_("mxfp4", simulate=True)
    sim_lib = _decode_logits(model)

    model.quantize_weights_("mxfp4")
    assert model.weight_dtype == "mxfp4"
    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "1")
    monkeypatch.setattr(ops, "_w4_m256_config", ops._w4_m256_default)
    calls = _count_calls(monkeypatch)
    mx = _decode_logits(model)
    n_layers = len(model.layers)
    assert len(calls["gemm_w4_m256"]) == 4 * n_layers  # qkv, o, gate_up, down
    assert not calls["gemm_w4"] and not calls["dequant_w4"]
    assert bool(torch.isfinite(mx).all()) and mx.abs().max().item() > 1e-3

    yard = (sim_twin - sim_lib).abs().max().item()
    diff = (mx - sim_twin).abs().max().item()
    print(f"yardstick {yard:.6f} mxfp4-macro-vs-fake-quant {diff:.6f}")
    assert diff <= 4 * yard


# ---------- 11. engine ----------

def test_engine_mxfp4_hipgraph_macro(monkeypatch):
    from llmapigateway_amd.engine import LLMEngine, SamplingParams

    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "1")
    monkeypatch.setattr(ops, "_w4_m256_config", ops._w4_m256_default)
    calls = _count_calls(monkeypatch)
    eng = LLMEngine(
        model=LLAMA_1B, device=DEV, dtype=torch.bfloat16, block_size=16,
        num_blocks=64, max_model_len=256, max_batch_size=4, seed=0,
        use_hipgraph=True, admit_min_batch=1, weight_dtype="mxfp4",
    )
    outs = [
        eng.generate(
            list(range(3, 35)), SamplingParams(max_tokens=8, ignore_eos=True)
        ).out_ids
        for _ in range(2)
    ]
    assert len(outs[0]) == 8 and outs[0] == outs[1]
    assert eng.stats["graph_steps"] > 0
    assert calls["gemm_w4_m256"], "the macro kernel must have run"
    assert not calls["gemm_w4"]
