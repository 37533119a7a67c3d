"""moe_mlp's choice of the MXFP4 128-row prefill tile (host integers only)."""

import pytest

from llmapigateway_amd import ops

E, K = 8, 2


@pytest.mark.parametrize(
    "T,H,knob,default,want",
    [
        (512, 256, None, 128, True),    # 128 pairs per expert
        (511, 256, None, 128, False),   # 127.75
        (512, 192, None, 128, False),   # H % 128 != 0: the tile does not serve it
        (512, 256, "129", 128, False),  # the knob overrides the default
        (64, 256, "16", None, True),
        (4096, 256, None, None, False),  # no default and no knob: off
    ],
)
def test_big_w4_route(T, H, knob, default, want, monkeypatch):
    monkeypatch.setattr(ops, "MOE_W4_BIG_MIN_ROWS", default)
    if knob is None:
        monkeypatch.delenv("LLMAPI_MOE_W4_BIG_MIN_ROWS", raising=False)
    else:
        monkeypatch.setenv("LLMAPI_MOE_W4_BIG_MIN_ROWS", knob)
    assert ops._moe_big_w4_route(T, K, E, H, 512) is want
    # the bf16 route never takes quantised experts, whatever either knob says
    monkeypatch.setenv("LLMAPI_MOE_BIG_MIN_ROWS", "1")
    assert ops._moe_big_route(T, K, E, 256, 512, True) is False
