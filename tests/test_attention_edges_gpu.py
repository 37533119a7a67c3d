"""GPU edge tests of the decode and prefill attention kernels against the
fp64 references of attn_cases.py. Every assertion is metric <= bound (4 x
the measured fp32/bf16 noise floor, see attn_cases.py) and no NaN; the
needle / diagonal / poison inputs make one wrong, missing or leaked key an
O(1) error (proved on the CPU by test_attention_cases_cpu.py), and every
unused cache slot is NaN, so a kernel that reads past a context shows it.

Run with -s to see each case's figure."""

import pytest
import torch

from llmapigateway_amd import ops
from tests import attn_cases as ac

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
    """NaN in the flash-decode partial buffers that ops reuses across calls:
    whatever the combine kernel reads must have been written by this launch."""
    ops._decode_acc.get(DEV, 1 << 20).fill_(NAN)  # >= B*Hq*nsplit*D of any case
    ops._decode_ml.get(DEV, 1 << 14).fill_(NAN)


def _decode(case, q=None):
    a = _paged_args(case.paged)
    _poison_split_scratch()
    return ops.attention_decode(
        _dev(case.q) if q is None else q, a["k_cache"], a["v_cache"],
        a["block_tables"], a["lens"], case.scale,
        k_scale=a["k_scale"], v_scale=a["v_scale"])


def _check(tag, out, ref64, bound):
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), f"{tag}: NaN in the output"
    m = ac.metric(out, ref64)
    print(f"{tag}: metric {m:.5f} (bound {bound:.4f})")
    assert m <= bound, f"{tag}: metric {m} > {bound}"


def _fused_views(parts):
    """Each [T, H_i, D] tensor as a strided view into one fused row buffer
    (how the model hands q, k and v to the kernels); the gaps are NaN."""
    T = parts[0].shape[0]
    widths = [p.shape[1] * ac.D for p in parts]
    buf = torch.full((T, sum(widths) + ac.D), NAN, dtype=torch.bfloat16, device=DEV)
    views, col = [], ac.D  # one NaN head of padding in front
    for p, w in zip(parts, widths):
        v = buf[:, col:col + w].view(T, p.shape[1], ac.D)
        v.copy_(p)
        views.append(v)
        col += w
    return views


# ---------- decode through ops.attention_decode ----------

_OPS_DECODE = [c.id for c in ac.DECODE_CASES if not c.id.startswith("binding-")]


@pytest.mark.parametrize("id", _OPS_DECODE)
def test_decode_case(id):
    case, ref64 = ac.decode_case(id)
    out = _decode(case)
    _check(id, out, ref64, ac.ATTN_BOUND_DECODE)
    for b, L in enumerate(case.spec.lens):
        if L == 0:  # an empty context is defined as zeros, as on the CPU
            assert (out[b] == 0).all(), f"{id}: row {b} with context_lens == 0"


@pytest.mark.parametrize(
    "id", ["ragged-bs16-needle-last", "ragged-bs16-flat", "split-bf16-needle-last",
           "split-fp8-flat"])
def test_decode_strided_q(id):
    """q as a view into the fused qkv row: q.stride(0) != Hq * D."""
    case, ref64 = ac.decode_case(id)
    B, Hq, _ = case.q.shape
    Hkv = case.spec.Hkv
    pad = torch.zeros(B, Hkv, ac.D, dtype=torch.bfloat16)
    (q, _, _) = _fused_views([case.q, pad, pad])
    assert q.stride(0) != Hq * ac.D
    _check(id + "/strided", _decode(case, q=q), ref64, ac.ATTN_BOUND_DECODE)


@pytest.mark.parametrize(
    "id", ["ragged-bs16-flat", "split-bf16-flat", "split-fp8-mix-flat", "long16400-flat"])
def test_decode_two_calls_bit_identical(id):
    case, _ = ac.decode_case(id)
    a = _decode(case).clone()
    b = _decode(case)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------- decode through the binding: explicit version / nsplit ----------

def _binding_decode(case, version, nsplit):
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
        float(case.scale), pa, pm, nsplit, a["k_scale"], a["v_scale"], version)
    return out


@pytest.mark.parametrize("G", [4, 7])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("version", [1, 2])
def test_decode_binding_version_nsplit(version, nsplit, cache, G):
    """v1 without split (LLMAPI_DECODE_VER=1) and v2 with split are compiled
    for every G and both cache types but never chosen by ops' defaults."""
    id = f"binding-G{G}-{cache}"
    case, ref64 = ac.decode_case(id)
    out = _binding_decode(case, version, nsplit)
    _check(f"{id}/v{version}/nsplit{nsplit}", out, ref64, ac.ATTN_BOUND_DECODE)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("version", [1, 2])
def test_decode_binding_long_block_table(version, nsplit):
    """Block-table index >= 1024 (global-memory fallback) in both geometries,
    unsplit and with a span that must stretch to cover 16400 positions."""
    case, ref64 = ac.decode_case("long16400-needle-16399")
    out = _binding_decode(case, version, nsplit)
    _check(f"long16400/v{version}/nsplit{nsplit}", out, ref64, ac.ATTN_BOUND_DECODE)


# ---------- prefill through ops.attention_prefill ----------

def _prefill(case, q=None, k=None, v=None):
    kw = {}
    if case.paged is not None:
        a = _paged_args(case.paged)
        kw = dict(k_cache=a["k_cache"], v_cache=a["v_cache"],
                  block_tables=a["block_tables"], cached_lens=a["lens"],
                  k_scale=a["k_scale"], v_scale=a["v_scale"])
    return ops.attention_prefill(
        _dev(case.q) if q is None else q, _dev(case.k) if k is None else k,
        _dev(case.v) if v is None else v, _dev(case.cu_seqlens),
        max(case.spec.lens), case.scale, **kw)


@pytest.mark.parametrize("id", [c.id for c in ac.PREFILL_CASES])
def test_prefill_case(id):
    case, ref64 = ac.prefill_case(id)
    _check(id, _prefill(case), ref64, ac.ATTN_BOUND_PREFILL)


@pytest.mark.parametrize("id", ["varlen-diag", "varlen-poison", "cached-bf16-needle-last"])
def test_prefill_strided_qkv(id):
    case, ref64 = ac.prefill_case(id)
    q, k, v = _fused_views([case.q, case.k, case.v])
    assert q.stride(0) != case.q.shape[1] * ac.D and k.stride(0) != case.k.shape[1] * ac.D
    _check(id + "/strided", _prefill(case, q, k, v), ref64, ac.ATTN_BOUND_PREFILL)
