"""The measured GEMM dispatch table (ops._m256_config) is data the
serving hot path depends on: these CPU tests pin which shapes route to
the custom macro-tile kernel vs the tuned library so a table edit can't
silently drop a measured entry (profiles/r02_gemm_m256_sweep.md)."""

import pytest

from llmapigateway_amd.ops import _m256_config


# llama-3-8b tp=1 decode projections (hidden 4096, inter 14336)
def test_8b_routing():
    assert _m256_config(256, 6144, 4096) is None        # qkv -> library
    assert _m256_config(256, 4096, 4096) is not None    # o -> custom
    assert _m256_config(256, 28672, 4096) is None       # gate_up -> library
    assert _m256_config(256, 4096, 14336) is not None   # down -> custom


# llama-3-70b tp=1 decode projections (hidden 8192, inter 28672)
def test_70b_routing():
    assert _m256_config(256, 10240, 8192) is None       # qkv -> library
    cfg = _m256_config(256, 8192, 8192)                 # o -> custom
    assert cfg == {"nf": 8, "nsk": 4, "variant": 0, "pipe": 0}
    assert _m256_config(256, 57344, 8192) is None       # gate_up -> library
    cfg = _m256_config(256, 8192, 28672)                # down -> custom
    assert cfg == {"nf": 8, "nsk": 4, "variant": 1, "pipe": 0}


# llama-3-8b tp=4 per-rank shard shapes
def test_8b_tp4_routing():
    assert _m256_config(256, 1536, 4096) is None        # qkv shard -> library
    cfg = _m256_config(256, 4096, 1024)                 # o shard -> custom
    assert cfg == {"nf": 4, "nsk": 1, "variant": 1, "pipe": 0}
    cfg = _m256_config(256, 7168, 4096)                 # gate_up shard -> custom
    assert cfg == {"nf": 4, "nsk": 3, "variant": 0, "pipe": 4}
    assert _m256_config(256, 4096, 3584) is not None    # down shard -> custom


def test_prefill_m_goes_to_library():
    # chunked-prefill token counts exceed the macro-tile M ceiling
    assert _m256_config(4096, 4096, 4096) is None


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 14336), (8192, 8192), (8192, 28672)])
def test_custom_configs_are_launchable_shapes(N, K):
    cfg = _m256_config(256, N, K)
    assert cfg is not None
    assert N % (16 * cfg["nf"]) == 0          # whole column tiles
    assert (K // 64) % cfg["nsk"] == 0 or cfg["nsk"] <= (K // 64)  # split-K fits


def test_swiglu_config_routing():
    from llmapigateway_amd.ops import _m256_swiglu_config

    assert _m256_swiglu_config(256, 28672, 4096) == {
        "nf": 8, "variant": 1, "pipe": 0}
    assert _m256_swiglu_config(100, 28672, 4096) == {
        "nf": 8, "variant": 0, "pipe": 0}          # M<=128 -> glds variant
    assert _m256_swiglu_config(256, 7168, 4096) is not None   # tp4 shard
    assert _m256_swiglu_config(4, 28672, 4096) is None        # skinny regime
    assert _m256_swiglu_config(256, 57344, 8192) is None      # 70B: library


def test_interleave_gate_up_mapping():
    # block-16 interleave must place gate block b at rows 32b..32b+16 and
    # the matching up block right after it — the fused epilogue contract
    import torch

    from llmapigateway_amd import ops

    I, K = 64, 8
    w = torch.arange(2 * I * K, dtype=torch.float32).view(2 * I, K)
    wi = ops.interleave_gate_up(w)
    for b in range(I // 16):
        assert torch.equal(wi[32 * b : 32 * b + 16], w[16 * b : 16 * b + 16])
        assert torch.equal(
            wi[32 * b + 16 : 32 * b + 32], w[I + 16 * b : I + 16 * b + 16]
        )


def test_interleaved_fused_matches_reference_math():
    # silu(gate-block) * up-block over the interleaved product equals
    # swiglu of the plain product (pure torch; the GPU kernel epilogue
    # implements exactly this block mapping)
    import torch
    import torch.nn.functional as F

    from llmapigateway_amd import ops

    torch.manual_seed(3)
    M, N, K = 8, 128, 64
    x = torch.randn(M, K)
    w = torch.randn(N, K)
    y = x @ ops.interleave_gate_up(w).T
    fused = torch.cat(
        [
            F.silu(y[:, 32 * b : 32 * b + 16]) * y[:, 32 * b + 16 : 32 * b + 32]
            for b in range(N // 32)
        ],
        dim=-1,
    )
    g, u = (x @ w.T).chunk(2, dim=-1)
    assert torch.allclose(fused, F.silu(g) * u, atol=1e-5)


# ---- linear() routing, pinned over a grid --------------------------------
# One row per M in _ROUTE_MS, one column per weight twin (none, k-major,
# fragment-major). LIB = tuned library, SKN / SWZ = streaming skinny kernel
# on the plain / k-major weight, a tuple = gemm_m256 (nf, nsk, variant,
# pipe). Recorded from linear() as it stood before the route became a
# function of its own (native calls stubbed), so the table is the yardstick
# and not an echo of _linear_route. (4096, 4128) has K % 64 == 32: the
# fragment twin cannot serve it and M <= 16 falls to the plain kernel.
LIB, SKN, SWZ = "LIB", "SKN", "SWZ"
_ROUTE_MS = (1, 8, 9, 16, 17, 64, 256, 257)
_ROUTE_TWINS = (None, "kmajor", "frag")
_ROUTES = {
    (6144, 4096): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, LIB),  # M=9
        (SKN, SWZ, LIB),  # M=16
        (LIB, SWZ, LIB),  # M=17
        (LIB, SWZ, LIB),  # M=64
        (LIB, SWZ, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (4096, 4096): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (4, 4, 0, 4)),  # M=9
        (SKN, SWZ, (4, 4, 0, 4)),  # M=16
        (LIB, SWZ, (4, 4, 0, 4)),  # M=17
        (LIB, SWZ, (4, 4, 0, 4)),  # M=64
        (LIB, SWZ, (4, 4, 0, 4)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (28672, 4096): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, LIB),  # M=9
        (SKN, SWZ, LIB),  # M=16
        (LIB, SWZ, LIB),  # M=17
        (LIB, SWZ, LIB),  # M=64
        (LIB, SWZ, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (4096, 14336): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (8, 8, 0, 0)),  # M=9
        (SKN, SWZ, (8, 8, 0, 0)),  # M=16
        (LIB, SWZ, (8, 8, 0, 0)),  # M=17
        (LIB, SWZ, (8, 8, 0, 0)),  # M=64
        (LIB, SWZ, (8, 8, 0, 0)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (10240, 8192): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, LIB),  # M=9
        (SKN, SWZ, LIB),  # M=16
        (LIB, SWZ, LIB),  # M=17
        (LIB, SWZ, LIB),  # M=64
        (LIB, SWZ, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (8192, 8192): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (8, 4, 0, 0)),  # M=9
        (SKN, SWZ, (8, 4, 0, 0)),  # M=16
        (LIB, SWZ, (8, 4, 0, 0)),  # M=17
        (LIB, SWZ, (8, 4, 0, 0)),  # M=64
        (LIB, SWZ, (8, 4, 0, 0)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (57344, 8192): [
        (LIB, LIB, LIB),  # M=1
        (LIB, LIB, LIB),  # M=8
        (LIB, LIB, LIB),  # M=9
        (LIB, LIB, LIB),  # M=16
        (LIB, LIB, LIB),  # M=17
        (LIB, LIB, LIB),  # M=64
        (LIB, LIB, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (8192, 28672): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (8, 4, 1, 0)),  # M=9
        (SKN, SWZ, (8, 4, 1, 0)),  # M=16
        (LIB, SWZ, (8, 4, 1, 0)),  # M=17
        (LIB, SWZ, (8, 4, 1, 0)),  # M=64
        (LIB, SWZ, (8, 4, 1, 0)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (1536, 4096): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, LIB),  # M=9
        (SKN, SWZ, LIB),  # M=16
        (LIB, SWZ, LIB),  # M=17
        (LIB, SWZ, LIB),  # M=64
        (LIB, SWZ, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (4096, 1024): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (4, 1, 1, 0)),  # M=9
        (SKN, SWZ, (4, 1, 1, 0)),  # M=16
        (LIB, SWZ, (4, 1, 1, 0)),  # M=17
        (LIB, SWZ, (4, 1, 1, 0)),  # M=64
        (LIB, SWZ, (4, 1, 1, 0)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (7168, 4096): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (4, 3, 0, 4)),  # M=9
        (SKN, SWZ, (4, 3, 0, 4)),  # M=16
        (LIB, SWZ, (4, 3, 0, 4)),  # M=17
        (LIB, SWZ, (4, 3, 0, 4)),  # M=64
        (LIB, SWZ, (4, 3, 0, 4)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (4096, 3584): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, (4, 4, 0, 4)),  # M=9
        (SKN, SWZ, (4, 4, 0, 4)),  # M=16
        (LIB, SWZ, (4, 4, 0, 4)),  # M=17
        (LIB, SWZ, (4, 4, 0, 4)),  # M=64
        (LIB, SWZ, (4, 4, 0, 4)),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
    (4096, 4128): [
        (SKN, SWZ, SKN),  # M=1
        (SKN, SWZ, SKN),  # M=8
        (SKN, SWZ, SKN),  # M=9
        (SKN, SWZ, SKN),  # M=16
        (LIB, SWZ, LIB),  # M=17
        (LIB, SWZ, LIB),  # M=64
        (LIB, SWZ, LIB),  # M=256
        (LIB, LIB, LIB),  # M=257
    ],
}


def _encode(route, kw):
    if route == "library":
        assert kw == {}
        return LIB
    if route == "skinny":
        assert set(kw) == {"swizzled"}
        return SWZ if kw["swizzled"] else SKN
    assert route == "m256" and set(kw) == {"nf", "nsk", "variant", "pipe"}
    return (kw["nf"], kw["nsk"], kw["variant"], kw["pipe"])


@pytest.mark.parametrize("N,K", sorted(_ROUTES))
def test_linear_route_grid(N, K):
    from llmapigateway_amd.ops import _linear_route

    for M, want in zip(_ROUTE_MS, _ROUTES[(N, K)]):
        got = tuple(_encode(*_linear_route(M, N, K, t)) for t in _ROUTE_TWINS)
        assert got == want, (M, N, K, got, want)
        # tensors the custom kernels cannot take always go to the library
        for t in _ROUTE_TWINS:
            assert _linear_route(M, N, K, t, eligible=False) == ("library", {})
