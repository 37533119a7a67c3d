"""The streaming decode GEMM (csrc/gemm_stream.h) exists once and is
instantiated for three weight layouts. These tests call the bindings with
an explicit nsk, so dispatch cannot route around the kernel, at the
smallest shapes that reach every path of its pipeline: the serial path
(fewer than 3 k-steps), every tail length r = 3..6 after zero, one or more
main-loop iterations, MF = 1 and 2, one and several waves, a ragged last
m-fragment, and even / uneven split-K slices.

The layouts must agree bit for bit: per accumulator every instantiation
issues the same MFMAs in the same (increasing-k) order on the same values.
For fp8 that holds because e4m3 -> bf16 is exact and the per-channel scale
is a power of two, so scaling the fp32 accumulator before the store
commutes with its rounding at these magnitudes.
"""

import pytest
import torch

from llmapigateway_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 128
MS = (1, 17, 129, 256)
# (K, nsk) in 32-deep k-steps: serial 1-2, tails 3-6, one main-loop trip
# with tails 3, 5 (7, 9), two trips with tails 3 (11) and 6 (14); then an
# even split and an uneven one whose last slice is short (11 + 11 + 10)
BF16_CASES = [(32 * s, 1) for s in (1, 2, 3, 4, 5, 6, 7, 9, 11, 14)] + [
    (1024, 2), (1024, 3)]
# the same in 64-deep steps; K/64 divisible by nsk so that both kernels cut
# their slices at the same k
FP8_CASES = [(64 * s, 1) for s in (1, 2, 3, 4, 5, 6, 7, 10)] + [(1024, 2)]


def _xw(M, K):
    g = torch.Generator(device="cpu").manual_seed(1000 * M + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(DEV)
    return x, w


def _skinny(x, w, swizzled, nsk):
    M = x.shape[0]
    y = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(nsk * M * N, dtype=torch.float32, device=DEV) if nsk > 1 else None
    ops._native().gemm_skinny(y, x, w, ws, nsk, swizzled)
    return y


def _rel_err(y, ref):
    return (y.float() - ref).abs().max().item() / (ref.abs().max().item() + 1e-3)


@pytest.mark.parametrize("M", MS)
def test_row_major_and_k_major_agree_exactly(M):
    for K, nsk in BF16_CASES:
        x, w = _xw(M, K)
        plain = _skinny(x, w, False, nsk)
        kmajor = _skinny(x, ops.swizzle_weight(w), True, nsk)
        assert torch.equal(plain, kmajor), (M, K, nsk)
        err = _rel_err(plain, x.float() @ w.float().T)
        assert err < 0.02, (M, K, nsk, err)


@pytest.mark.parametrize("M", MS)
def test_fp8_and_bf16_pipelines_agree_exactly(M):
    for K, nsk in FP8_CASES:
        x, w = _xw(M, K)
        q, s = ops.fp8_quantize_weight(w.cpu())  # power-of-two scales
        w_dq = ops.fp8_dequantize_weight(q, s, torch.bfloat16).to(DEV)
        qf, s = ops.swizzle_weight_frag_fp8(q).to(DEV), s.to(DEV)
        y8 = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        ws = torch.empty(nsk * M * N, dtype=torch.float32, device=DEV) if nsk > 1 else None
        ops._native().gemm_w8(y8, x, qf, s, ws, nsk)
        y16 = _skinny(x, w_dq, False, nsk)
        assert torch.equal(y8, y16), (M, K, nsk)
        err = _rel_err(y8, x.float() @ w_dq.float().T)
        assert err < 0.02, (M, K, nsk, err)
