"""The macro-tile MXFP4 route's dispatch function is pure, and the opt-in
knob (LLMAPI_W4_MACRO_MIN_M) leaves the CPU reference path alone."""

import pytest
import torch

from llmapigateway_amd import ops

# the decode projection shapes tools/gemm_w4_bench.py measures: (name, N, K)
BENCH_SHAPES = [
    ("8b qkv", 6144, 4096),
    ("8b o", 4096, 4096),
    ("8b gate_up", 28672, 4096),
    ("8b down", 4096, 14336),
    ("70b qkv", 10240, 8192),
    ("70b o", 8192, 8192),
    ("70b gate_up", 57344, 8192),
    ("70b down", 8192, 28672),
]
MS = (64, 128, 256)


def _check(cfg, name, M, N, K):
    assert set(cfg) == {"nf", "nsk"}, (name, M, cfg)
    assert cfg["nf"] in (4, 8), (name, M, cfg)
    assert N % (16 * cfg["nf"]) == 0, (name, M, cfg)
    assert 1 <= cfg["nsk"] <= K // 64, (name, M, cfg)
    if name.split()[1] in ("o", "down") and ops._reduce_norm_covers(N):
        assert cfg["nsk"] > 1, (name, M, cfg)  # the fused tail needs slabs


@pytest.mark.parametrize("name,N,K", BENCH_SHAPES)
def test_config_is_valid_for_the_bench_shapes(name, N, K):
    for M in MS:
        cfg = ops._w4_m256_config(M, N, K)
        if cfg is not None:
            _check(cfg, name, M, N, K)
        # the defaults every entry starts from obey the same rules
        _check(ops._w4_m256_default(M, N, K), name, M, N, K)


def test_table_rows_cover_the_measured_batch_sizes():
    names = {(N, K) for _, N, K in BENCH_SHAPES}
    for shape, row in ops._W4_M256_TABLE.items():
        assert shape in names, shape  # entries only for measured shapes
        assert tuple(sorted(row)) == MS, shape


def test_config_is_pure(monkeypatch):
    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "1")
    a = [ops._w4_m256_config(M, N, K) for _, N, K in BENCH_SHAPES for M in MS]
    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M")
    b = [ops._w4_m256_config(M, N, K) for _, N, K in BENCH_SHAPES for M in MS]
    assert a == b
    assert ops._w4_m256_config(257, 4096, 4096) is None
    assert ops._w4_m256_config(0, 4096, 4096) is None
    assert ops._w4_m256_config(64, 4096, 4096 + 32) is None


def test_default_nf_falls_back_to_4():
    assert ops._w4_m256_default(256, 192, 448)["nf"] == 4  # N % 128 != 0
    assert ops._w4_m256_default(256, 2048, 8192)["nf"] == 8
    assert ops._w4_m256_default(64, 2048, 8192)["nf"] == 4


def test_knob_gates_the_macro_route(monkeypatch):
    monkeypatch.setattr(ops, "_w4_m256_config", lambda M, N, K: {"nf": 4, "nsk": 2})
    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M", raising=False)
    assert ops._w4_macro_config(200, 2048, 8192) is None
    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "")
    assert ops._w4_macro_config(200, 2048, 8192) is None
    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "64")
    assert ops._w4_macro_config(200, 2048, 8192) == {"nf": 4, "nsk": 2}
    assert ops._w4_macro_config(64, 2048, 8192) == {"nf": 4, "nsk": 2}
    assert ops._w4_macro_config(63, 2048, 8192) is None
    assert ops._w4_macro_config(257, 2048, 8192) is None


def test_the_fp8_knob_does_not_open_the_mxfp4_route(monkeypatch):
    monkeypatch.setattr(ops, "_w4_m256_config", lambda M, N, K: {"nf": 4, "nsk": 2})
    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M", raising=False)
    monkeypatch.setenv("LLMAPI_W8_MACRO_MIN_M", "64")
    assert ops._w4_macro_config(200, 2048, 8192) is None


def test_cpu_path_ignores_the_knob(monkeypatch):
    M, N, K = 70, 128, 192
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    res = torch.randn(M, N, generator=g).bfloat16()
    norm_w = torch.randn(N, generator=g).bfloat16()
    qf, sf = ops.swizzle_weight_frag_mxfp4(*ops.mxfp4_quantize_weight(w))

    def run():
        y = ops.linear_w4(x, qf, sf)
        out, r = ops.linear_w4_rmsnorm_residual(x, qf, sf, res.clone(), norm_w, 1e-5)
        return y, out, r

    monkeypatch.delenv("LLMAPI_W4_MACRO_MIN_M", raising=False)
    base = run()
    monkeypatch.setenv("LLMAPI_W4_MACRO_MIN_M", "1")
    monkeypatch.setattr(ops, "_w4_m256_config", ops._w4_m256_default)
    for a, b in zip(base, run()):
        assert torch.equal(a, b)
