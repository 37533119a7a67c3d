"""Decode-step fusion: split-K reduce + residual add + RMSNorm in one kernel
(csrc/gemm_skinny.hip: gemm_reduce_rmsnorm_kernel) behind
ops.gemm_m256_rmsnorm_residual / ops.linear_rmsnorm_residual.

The fused kernel must reproduce the residual stream of the unfused pair
(gemm_m256 -> rmsnorm_residual) bit for bit; its normed output is allowed
one adjacent bf16 value of slack (a sum of squares reduced in another order
would move inv by fp32 ulps). The kernel re-adds the squares in the norm
kernels' own order, so in practice the printed distance is 0."""

import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from llmapigateway_amd import ops
from llmapigateway_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


def to_f32(x):
    return x.float().cpu()


def max_rel_err(got, ref, eps=1e-3):
    got, ref = to_f32(got), to_f32(ref)
    return ((got - ref).abs() / (ref.abs() + eps)).max().item()


def bf16_steps(a, b):
    """Largest distance between a and b counted in adjacent bf16 values."""
    def ordered(t):
        v = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(v >= 0, v, -(v & 0x7FFF))
    return (ordered(a) - ordered(b)).abs().max().item()


@functools.lru_cache(maxsize=None)
def _weights(N, K):
    g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(DEV)
    norm_w = torch.randn(N, generator=g).bfloat16().to(DEV)
    return w, ops.swizzle_weight_frag(w), norm_w


def _inputs(M, N, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(M * 13 + N + K + seed)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)
    # |residual| >= 2 keeps r = y + residual (|y| < ~1.5 here) away from
    # zero: the element-wise relative metric against the CPU reference is
    # then bounded by bf16 rounding (one step of y, r and out: < 0.03), not
    # by cancellation, where a one-step difference in y is unbounded in
    # relative terms
    r = torch.randn(M, N, generator=g)
    res = (torch.sign(r) * (r.abs() + 2.0)).bfloat16().to(DEV)
    return x, res


def _cfg(nsk):
    # the two production geometries: down-proj (nf 8, 3-deep ring) for the
    # deep split, o-proj (nf 4, 2-deep ring) for the shallow one
    return dict(nf=8, variant=0, pipe=0) if nsk == 8 else dict(nf=4, variant=0, pipe=4)


CASES = [
    (M, N, K, nsk)
    for M in (9, 33, 256)
    for N in (512, 4096, 8192)
    for K in (256, 1024)
    for nsk in (2, 8)
    if nsk <= (K // 64) // 2
]


@pytest.mark.parametrize("M,N,K,nsk", CASES)
def test_fused_reduce_norm(M, N, K, nsk):
    w, wf, norm_w = _weights(N, K)
    x, res0 = _inputs(M, N, K)
    cfg = _cfg(nsk)

    res_u = res0.clone()
    y = ops.gemm_m256(x, wf, nsk=nsk, **cfg)
    out_u, res_u = ops.rmsnorm_residual(y, res_u, norm_w, EPS)

    res_f = res0.clone()
    out_f, res_f2 = ops.gemm_m256_rmsnorm_residual(
        x, wf, res_f, norm_w, EPS, nsk=nsk, **cfg
    )
    assert res_f2 is res_f
    assert torch.equal(res_f, res_u)
    steps = bf16_steps(out_f, out_u)
    print(f"M={M} N={N} K={K} nsk={nsk}: out differs by {steps} bf16 step(s)")
    assert steps <= 1

    y_ref = (x.float().cpu() @ w.float().cpu().T).bfloat16()
    out_ref, res_ref = reference.rmsnorm_residual(y_ref, res0.cpu(), norm_w.cpu(), EPS)
    e_res, e_out = max_rel_err(res_f, res_ref), max_rel_err(out_f, out_ref)
    print(f"  vs reference: residual {e_res:.4f} out {e_out:.4f}")
    assert e_res < 0.05
    assert e_out < 0.05


def test_nsk1_rejected():
    w, wf, norm_w = _weights(512, 256)
    x, res = _inputs(9, 512, 256)
    with pytest.raises(ValueError):
        ops.gemm_m256_rmsnorm_residual(x, wf, res, norm_w, EPS, nf=4, nsk=1)
    out = torch.empty_like(res)
    with pytest.raises(RuntimeError):
        ops._native().gemm_m256(
            out, x, wf, None, 1, 4, 0, 0, 0, res, norm_w, EPS, out
        )


def _spy(monkeypatch):
    calls = []
    real = ops.gemm_m256_rmsnorm_residual

    def wrapped(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "gemm_m256_rmsnorm_residual", wrapped)
    return calls


def test_linear_rmsnorm_residual_takes_fused_path(monkeypatch):
    M, N, K = 64, 4096, 4096
    w, wf, norm_w = _weights(N, K)
    x, res0 = _inputs(M, N, K)
    calls = _spy(monkeypatch)
    res_f = res0.clone()
    out_f, _ = ops.linear_rmsnorm_residual(x, w, wf, res_f, norm_w, EPS)
    assert len(calls) == 1 and calls[0]["nsk"] > 1

    res_u = res0.clone()
    out_u, _ = ops.rmsnorm_residual(ops.linear(x, w, wf), res_u, norm_w, EPS)
    assert torch.equal(res_f, res_u)
    assert bf16_steps(out_f, out_u) <= 1

    # the opt-out restores the two-kernel sequence exactly
    monkeypatch.setenv("LLMAPI_NO_DECODE_FUSION", "1")
    res_o = res0.clone()
    out_o, _ = ops.linear_rmsnorm_residual(x, w, wf, res_o, norm_w, EPS)
    assert len(calls) == 1
    assert torch.equal(res_o, res_u) and torch.equal(out_o, out_u)


def test_linear_rmsnorm_residual_falls_back_at_small_m(monkeypatch):
    M, N, K = 4, 4096, 4096
    w, wf, norm_w = _weights(N, K)
    x, res0 = _inputs(M, N, K)
    calls = _spy(monkeypatch)
    res_f = res0.clone()
    out_f, _ = ops.linear_rmsnorm_residual(x, w, wf, res_f, norm_w, EPS)
    assert calls == []
    res_u = res0.clone()
    out_u, _ = ops.rmsnorm_residual(ops.linear(x, w, wf), res_u, norm_w, EPS)
    assert torch.equal(res_f, res_u) and torch.equal(out_f, out_u)


def test_fused_graph_replay():
    # the slab workspace is fully rewritten by every launch, so replays of a
    # captured fused op with new inputs stay correct
    M, N, K, nsk = 33, 4096, 1024, 8
    w, wf, norm_w = _weights(N, K)
    cfg = _cfg(nsk)
    x_s, res_s = _inputs(M, N, K)
    x_s, res_s = x_s.clone(), res_s.clone()
    ops.gemm_m256_rmsnorm_residual(x_s, wf, res_s.clone(), norm_w, EPS, nsk=nsk, **cfg)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, _ = ops.gemm_m256_rmsnorm_residual(
            x_s, wf, res_s, norm_w, EPS, nsk=nsk, **cfg
        )
    for seed in (1, 2):
        x, res0 = _inputs(M, N, K, seed=seed)
        x_s.copy_(x)
        res_s.copy_(res0)
        graph.replay()
        res_u = res0.clone()
        out_u, _ = ops.rmsnorm_residual(
            ops.gemm_m256(x, wf, nsk=nsk, **cfg), res_u, norm_w, EPS
        )
        assert torch.equal(res_s, res_u)
        assert bf16_steps(out_s, out_u) <= 1


# ---------- engine: fused vs LLMAPI_NO_DECODE_FUSION=1 ----------

_CHILD = r"""
import json, sys
import torch
from llmapigateway_amd import ops
from llmapigateway_amd.engine import LLMEngine, EngineRequest, SamplingParams
from llmapigateway_amd.models.configs import ModelConfig

n_prompts = int(sys.argv[1])
# hidden % 512 == 0 and o/down shapes the dispatch table gives split-K
# fragment twins (N = K = 2048 -> nsk 8)
cfg = ModelConfig(
    name="gpu-fusion-tiny", hidden_size=2048, intermediate_size=2048,
    num_layers=2, num_heads=16, num_kv_heads=4, vocab_size=2048,
    head_dim=128, rope_theta=10000.0, max_positions=1024,
)
engine = LLMEngine(
    model=cfg, device="cuda:0", dtype=torch.bfloat16, block_size=16,
    num_blocks=256, seed=0, use_hipgraph=True, admit_min_batch=1,
    max_batch_size=16,
)
assert "o_swz" in engine.model.layers[0] and "down_swz" in engine.model.layers[0]
fused = []
real = ops.gemm_m256_rmsnorm_residual
def spy(*a, **kw):
    fused.append(a[0].shape[0])
    return real(*a, **kw)
ops.gemm_m256_rmsnorm_residual = spy
first = []
run = engine.graph_runner.run
def rec(*a, **kw):
    logits = run(*a, **kw)
    if not first:
        first.append(logits.float().cpu())
    return logits
engine.graph_runner.run = rec
reqs = [
    EngineRequest([1 + i, 5 + 2 * i, 9, 40 + i, 7][: 3 + i % 3],
                  SamplingParams(max_tokens=8, ignore_eos=True))
    for i in range(n_prompts)
]
for r in reqs:
    engine.add_request(r)
steps = 0
while any(r.state in ("waiting", "running") for r in reqs):
    engine.step()
    steps += 1
    assert steps < 1000
assert engine.graph_runner is not None and engine.stats["graph_steps"] > 0
torch.save(first[0].bfloat16(), sys.argv[2])
print(json.dumps({"ids": [r.out_ids for r in reqs], "fused_rows": fused}))
"""


def _run_child(n_prompts, path, no_fusion):
    env = dict(os.environ)
    env.pop("LLMAPI_NO_DECODE_FUSION", None)
    if no_fusion:
        env["LLMAPI_NO_DECODE_FUSION"] = "1"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run(
        [sys.executable, "-c", _CHILD, str(n_prompts), str(path)],
        env=env, capture_output=True, text=True, timeout=300,
    )
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), torch.load(path)


# 3 prompts: the decode bucket (4 rows) is below the macro-tile GEMM's M
# range, so fusion acts through the prefill step; 12 prompts put the
# captured decode step itself (bucket 16) on the fused kernel
@pytest.mark.parametrize("n_prompts", [3, 12])
def test_engine_fusion_matches_unfused(tmp_path, n_prompts):
    a, la = _run_child(n_prompts, tmp_path / "fused.pt", no_fusion=False)
    b, lb = _run_child(n_prompts, tmp_path / "plain.pt", no_fusion=True)
    assert a["fused_rows"], "fused path never taken"
    if n_prompts > 8:
        assert 16 in a["fused_rows"], "captured decode step did not fuse"
    assert b["fused_rows"] == []
    steps = bf16_steps(la, lb)
    same = sum(x == y for x, y in zip(a["ids"], b["ids"]))
    print(f"first decode-step logits differ by {steps} bf16 step(s); "
          f"{same}/{n_prompts} sequences identical")
    print("fused ids:  ", a["ids"])
    print("unfused ids:", b["ids"])
    assert all(len(o) == 8 for o in a["ids"] + b["ids"])
    assert steps <= 1
