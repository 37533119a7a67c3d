"""The bf16 instantiation of the register-staged macro-tile pipeline
(csrc/gemm_macro.h; gemm_m256 variant 1).

tests/test_w8_macro_gpu.py and tests/test_w4_macro_gpu.py pin the quantised
kernels to this one bit for bit, which says nothing about this one. Here it
meets references of its own:

- exact integer data against an fp64 matmul, so a single wrong, missing or
  doubled fragment anywhere in the staging shows as an unequal integer;
- the non-temporal W loads (variant=1, pipe=1) against the plain loads;
- the fused swiglu epilogue after every tail of the 2-buffer, loads-two-ahead
  loop (1, 2 and 3 k64 tiles), against silu(g)*u of the glds kernel's plain
  output on the same interleaved twin.
"""

import functools

import pytest
import torch

from llmapigateway_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


# ---------- 1. exact data ----------

EXACT_K = 320  # 5 k64 tiles: 3 + 2 at nsk = 2


@functools.lru_cache(maxsize=None)
def _exact(M, N):
    """(x, w_frag, fp64 reference as bf16) of small-integer data: |x| <= 4,
    |w| <= 2, three w in four zero. Every product and every partial sum is
    an integer below 320 * 8 < 2^24, exact in fp32 in any order; the final
    sums stay below 256, where bf16 holds every integer."""
    g = torch.Generator(device="cpu").manual_seed(M * 31 + N)
    x = torch.randint(-4, 5, (M, EXACT_K), generator=g)
    w = torch.randint(-2, 3, (N, EXACT_K), generator=g)
    w = w * (torch.randint(0, 4, (N, EXACT_K), generator=g) == 0)
    assert x.abs().max() == 4 and w.abs().max() == 2
    ref = x.double() @ w.double().T
    assert ref.abs().max() < 256, ref.abs().max()
    assert torch.equal(ref.bfloat16().double(), ref)
    return (
        x.bfloat16().to(DEV),
        ops.swizzle_weight_frag(w.bfloat16().to(DEV)),
        ref.bfloat16(),
    )


@pytest.mark.parametrize(
    "M,N,nf", [(1, 64, 4), (17, 192, 4), (100, 128, 8), (256, 128, 8)]
)
@pytest.mark.parametrize("nsk", [1, 2])
def test_exact_integers_match_fp64(M, N, nf, nsk):
    x, w_frag, ref = _exact(M, N)
    y = ops.gemm_m256(x, w_frag, nf=nf, nsk=nsk, variant=1)
    assert torch.equal(y.cpu(), ref), (M, N, nf, nsk)


# ---------- 2. non-temporal W loads ----------

def _rand(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M * 13 + N * 7 + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(DEV)
    return x, w


@pytest.mark.parametrize("M,N,nf", [(17, 192, 4), (200, 128, 8)])
@pytest.mark.parametrize("K,nsk", [(320, 1), (448, 2)])
def test_nontemporal_w_loads_change_nothing(M, N, nf, K, nsk):
    x, w = _rand(M, N, K)
    w_frag = ops.swizzle_weight_frag(w)
    plain = ops.gemm_m256(x, w_frag, nf=nf, nsk=nsk, variant=1, pipe=0)
    nt = ops.gemm_m256(x, w_frag, nf=nf, nsk=nsk, variant=1, pipe=1)
    assert torch.equal(nt, plain), (M, N, nf, K, nsk)
    # and both are the product, not equal garbage
    ref = x.float() @ w.float().T
    err = (plain.float() - ref).abs().max().item() / (ref.abs().max().item() + 1e-3)
    assert err < 0.02, (M, N, nf, K, nsk, err)


# ---------- 3. pipeline tails through the swiglu epilogue ----------

@pytest.mark.parametrize("M", [17, 200])
@pytest.mark.parametrize("nf", [4, 8])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_swiglu_epilogue_after_every_pipeline_tail(M, nf, K):
    N = 256  # the stacked 2*I
    x, w = _rand(M, N, K)
    wi = ops.swizzle_weight_frag(ops.interleave_gate_up(w))
    got = ops.gemm_m256_swiglu(x, wi, nf=nf, variant=1)
    assert got.shape == (M, N // 2)
    # the glds kernel's plain output on the same twin: columns in block-16
    # interleaved order g0..15, u0..15, g16..31, ...
    y0 = ops.gemm_m256(x, wi, nf=nf, nsk=1, variant=0).float()
    gu = y0.view(M, N // 32, 2, 16)
    g, u = gu[:, :, 0].reshape(M, N // 2), gu[:, :, 1].reshape(M, N // 2)
    ref = torch.nn.functional.silu(g) * u
    # test_gemm_m256_fused_swiglu's tolerance
    err = (got.float() - ref).abs().max().item() / (ref.abs().max().item() + 1e-3)
    print(f"M={M} nf={nf} K={K} err={err:.5f}")
    assert err < 0.02, (M, nf, K, err)
