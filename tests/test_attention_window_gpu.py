"""GPU tests of sliding-window attention in the decode and prefill kernels
against the fp64 references of attn_window_cases.py, under its bounds (4 x
the noise floor measured on the CPU, as in attn_cases.py). The needle-edge / poison-out inputs make
a window edge that is off by one key an O(1) error (proved on the CPU by
test_attention_window_cases_cpu.py); block-table entries of blocks below the
window point at a NaN block, so a read of a released block shows as NaN.

Run with -s to see each case's figure."""

import pytest
import torch

from llmapigateway_amd import ops
from tests import attn_cases as ac
from tests import attn_window_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


def _dev(t):
    return None if t is None else t.to(DEV)


def _paged_args(p):
    return dict(k_cache=_dev(p.k_cache), v_cache=_dev(p.v_cache),
                block_tables=_dev(p.block_tables), lens=_dev(p.lens),
                k_scale=_dev(p.k_scale), v_scale=_dev(p.v_scale))


def _poison_split_scratch():
    ops._decode_acc.get(DEV, 1 << 20).fill_(NAN)
    ops._decode_ml.get(DEV, 1 << 14).fill_(NAN)


def _decode(case, window):
    a = _paged_args(case.paged)
    _poison_split_scratch()
    return ops.attention_decode(
        _dev(case.q), a["k_cache"], a["v_cache"], a["block_tables"], a["lens"],
        case.scale, k_scale=a["k_scale"], v_scale=a["v_scale"], window=window)


def _prefill(case, window):
    kw = {}
    if case.paged is not None:
        a = _paged_args(case.paged)
        kw = dict(k_cache=a["k_cache"], v_cache=a["v_cache"],
                  block_tables=a["block_tables"], cached_lens=a["lens"],
                  k_scale=a["k_scale"], v_scale=a["v_scale"])
    return ops.attention_prefill(
        _dev(case.q), _dev(case.k), _dev(case.v), _dev(case.cu_seqlens),
        max(case.spec.lens), case.scale, window=window, **kw)


def _check(tag, out, ref64, bound):
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), f"{tag}: NaN in the output"
    m = ac.metric(out, ref64)
    print(f"{tag}: metric {m:.5f} (bound {bound:.4f})")
    assert m <= bound, f"{tag}: metric {m} > {bound}"


def _bits_equal(a, b):
    torch.cuda.synchronize()
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------- decode ----------

@pytest.mark.parametrize("id", [c.id for c in wc.WIN_DECODE_CASES])
def test_decode_window_case(id):
    case, ref64 = wc.win_decode_case(id)
    _check(id, _decode(case, case.spec.W), ref64, wc.WIN_BOUND_DECODE)


def _binding_decode(case, version, nsplit, window):
    a = _paged_args(case.paged)
    q = _dev(case.q)
    B, Hq, D = q.shape
    out = torch.full_like(q, NAN)
    pa = pm = None
    if nsplit > 1:  # NaN: every launched split must overwrite what combine reads
        pa = torch.full((B * Hq * nsplit * D,), NAN, dtype=torch.float32, device=DEV)
        pm = torch.full((B * Hq * nsplit * 2,), NAN, dtype=torch.float32, device=DEV)
    ops._C.attention_decode(
        out, q, a["k_cache"], a["v_cache"], a["block_tables"], a["lens"],
        float(case.scale), pa, pm, nsplit, a["k_scale"], a["v_scale"], version,
        window)
    return out


@pytest.mark.parametrize("kind", ["needle-edge", "poison-out"])
@pytest.mark.parametrize("W", [64, 2048, 2100])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("version", [1, 2])
def test_decode_window_binding_version_nsplit(version, nsplit, cache, W, kind):
    """Both geometries, unsplit and with three splits measured from the
    window's start (W = 64 leaves two of them idle)."""
    id = f"split-{cache}-w{W}-{kind}"
    case, ref64 = wc.win_decode_case(id)
    out = _binding_decode(case, version, nsplit, W)
    _check(f"{id}/v{version}/nsplit{nsplit}", out, ref64, wc.WIN_BOUND_DECODE)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("id", ["long16400-w100-poison-out", "long16400-w16390-needle-edge",
                                "split-bf16-mix-w64-needle-edge"])
def test_decode_window_binding_long_and_mix(id, version, nsplit):
    case, ref64 = wc.win_decode_case(id)
    out = _binding_decode(case, version, nsplit, case.spec.W)
    _check(f"{id}/v{version}/nsplit{nsplit}", out, ref64, wc.WIN_BOUND_DECODE)


@pytest.mark.parametrize(
    "id", ["ragged-bs16-needle-last", "ragged-bs64-flat", "ragged-fp8-flat",
           "G7-flat", "split-bf16-needle-2048", "split-fp8-mix-flat",
           "long16400-needle-16384", "empty-row-nonsplit", "empty-row-split"])
def test_decode_wide_window_is_bit_identical(id):
    """W >= max(lens): the same bits as the windowless call, non-split and
    split (the split geometry then equals the windowless one)."""
    case, _ = ac.decode_case(id)
    base = _decode(case, 0).clone()
    for W in (max(case.spec.lens), 1 << 20):
        assert _bits_equal(_decode(case, W), base), (id, W)


# ---------- prefill ----------

@pytest.mark.parametrize("id", [c.id for c in wc.WIN_PREFILL_CASES])
def test_prefill_window_case(id):
    case, ref64 = wc.win_prefill_case(id)
    _check(id, _prefill(case, case.spec.W), ref64, wc.WIN_BOUND_PREFILL)


@pytest.mark.parametrize("id", [c.id for c in ac.PREFILL_CASES])
def test_prefill_wide_window_is_bit_identical(id):
    case, _ = ac.prefill_case(id)
    base = _prefill(case, 0).clone()
    total = max(case.spec.lens) + (max(case.spec.cached) if case.spec.cached else 0)
    for W in (total, 1 << 20):
        assert _bits_equal(_prefill(case, W), base), (id, W)


def test_prefill_window_noncausal_still_raises():
    case, _ = wc.win_prefill_case("varlen-w16-flat")
    with pytest.raises(NotImplementedError):
        ops.attention_prefill(
            _dev(case.q), _dev(case.k), _dev(case.v), _dev(case.cu_seqlens),
            max(case.spec.lens), case.scale, causal=False, window=16)
