"""The route to the 128-row prefill tile of the MoE expert GEMMs, from host
integers only."""

import pytest

from llmapigateway_amd import ops


@pytest.mark.parametrize("T,k,E,H,quantised,min_rows,big", [
    (511, 2, 8, 4096, False, 128, False),  # 127.75 pairs per expert
    (512, 2, 8, 4096, False, 128, True),
    (16, 2, 8, 256, False, 4, True),
    (4096, 2, 8, 4096, False, 1025, False),
    (4096, 2, 8, 4096, True, 128, False),  # MXFP4 experts keep their kernel
    (4096, 2, 8, 4160, False, 128, False),  # H % 128 != 0
])
def test_big_route(T, k, E, H, quantised, min_rows, big, monkeypatch):
    monkeypatch.setenv("LLMAPI_MOE_BIG_MIN_ROWS", str(min_rows))
    assert ops.moe_big_serves(H, 14336) == (H % 128 == 0)
    assert ops._moe_big_route(T, k, E, H, 14336, quantised) == big
    # without the variable the default decides, and it is at least 128
    monkeypatch.delenv("LLMAPI_MOE_BIG_MIN_ROWS")
    rows = ops.MOE_BIG_MIN_ROWS
    assert rows >= 128
    assert ops._moe_big_route(rows, 2, 2, 128, 64, False)
    assert not ops._moe_big_route(rows - 1, 2, 2, 128, 64, False)
