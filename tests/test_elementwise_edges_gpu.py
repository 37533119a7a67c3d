"""GPU edge tests of the elementwise kernels (csrc/elementwise.hip) against
the fp64 oracles of elem_cases.py: every rmsnorm dispatch instance (wave
form VPL 1..8, block form cached and re-read), rope at D 32/64/128 on the
fused qkv buffer, swiglu at the __expf overflow edge, the bf16 KV scatter
and every fp8_write_row layout. Assertions are metric <= bound (2 x the
measured bf16 floor, see elem_cases.py), bitwise equality where the op only
moves or quantises data, and no NaN where the oracle has none;
test_elem_cases_cpu.py proves on the CPU that each listed mistake fails them.

Run with -s to see each case's figure."""

import pytest
import torch

from llmapigateway_amd import ops
from tests import elem_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _require_native():
    assert torch.cuda.is_available(), "GPU required"
    assert ops.have_native(), (
        "HIP extension is not loaded on a GPU box — the native path MUST run"
    )


def _check(tag, m, bound):
    print(f"{tag}: metric {m:.6f} (bound {bound:.5f})")
    assert ec.passes(m, bound), f"{tag}: metric {m} > {bound}"


# ---------- rmsnorm ----------

@pytest.mark.parametrize("id", [c.id for c in ec.RMS_CASES])
def test_rmsnorm(id):
    c = ec.rms_case(id)
    ref, _ = ec.rmsnorm_oracle(c)
    x = c.x.to(DEV)
    out = ops.rmsnorm(x, c.weight.to(DEV), c.spec.eps)
    torch.cuda.synchronize()
    assert torch.equal(ec.bits(x), ec.bits(c.x)), "rmsnorm changed its input"
    assert not torch.isnan(out).any()
    _check(f"rmsnorm {id}", ec.rel_metric(out, ref), ec.RMSNORM_BOUND)


@pytest.mark.parametrize("id", [c.id for c in ec.RMS_CASES])
def test_rmsnorm_residual(id):
    c = ec.rms_case(id)
    ref, new_res = ec.rmsnorm_oracle(c, fused=True)
    res = c.residual.to(DEV)
    out, res_out = ops.rmsnorm_residual(c.x.to(DEV), res, c.weight.to(DEV), c.spec.eps)
    torch.cuda.synchronize()
    assert res_out.data_ptr() == res.data_ptr()
    assert torch.equal(ec.bits(res), ec.bits(new_res)), (
        f"{id}: the updated residual is not bf16(fp32(x + residual)) bit for bit")
    assert not torch.isnan(out).any()
    _check(f"rmsnorm_residual {id}", ec.rel_metric(out, ref), ec.RMSNORM_RESIDUAL_BOUND)


# ---------- rope ----------

@pytest.mark.parametrize("id", [c.id for c in ec.ROPE_CASES])
def test_rope(id):
    c = ec.rope_case(id)
    ref, den = ec.rope_oracle(c.qkv, c.positions, c.cos_sin)
    buf = c.qkv.buf.to(DEV)
    q, k, _ = c.qkv.views(buf)
    ops.rope_inplace(q, k, c.positions.to(DEV), c.cos_sin.to(DEV))
    torch.cuda.synchronize()
    m = ec.rope_check_buffer(f"rope {id}", buf, c.qkv, ref, den, ec.ROPE_BOUND)
    print(f"rope {id}: metric {m:.6f} (bound {ec.ROPE_BOUND:.5f})")


# ---------- swiglu ----------

@pytest.mark.parametrize("id", [c.id for c in ec.SWIGLU_CASES])
def test_swiglu(id):
    x = ec.swiglu_case(id)
    ref = ec.swiglu_oracle(x)
    out = ops.swiglu(x.to(DEV))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), f"swiglu {id}: NaN"
    _check(f"swiglu {id}", ec.swiglu_metric(out, ref), ec.SWIGLU_BOUND)


# ---------- KV write ----------

def _dev_cache(spec):
    return tuple(None if t is None else t.to(DEV) for t in ec.empty_cache(spec))


def _assert_caches(tag, got, want):
    for name, a, b in zip(("k_cache", "v_cache", "k_scale", "v_scale"), got, want):
        if b is None:
            continue
        same = ec.bits(a) == ec.bits(b)
        assert bool(same.all()), (
            f"{tag}: {name} differs from the oracle in {int((~same).sum())} elements "
            f"(first at flat index {int((~same).flatten().nonzero()[0])})")


@pytest.mark.parametrize("id", [c.id for c in ec.KV_CASES + ec.KV_FP8_CASES])
def test_kv_cache_write(id):
    """Plain scatter: the whole cache (and the scales) bit for bit,
    sentinels included; k and v untouched."""
    c = ec.kv_case(id)
    buf = c.qkv.buf.to(DEV)
    _, k, v = c.qkv.views(buf)
    _, k0, v0 = c.qkv.views()
    got = _dev_cache(c.spec)
    ops.kv_cache_write(k, v, got[0], got[1], c.slots.to(DEV), got[2], got[3])
    torch.cuda.synchronize()
    assert torch.equal(ec.bits(buf), ec.bits(c.qkv.buf)), "kv_cache_write changed k or v"
    _assert_caches(f"kv_cache_write {id}", got, ec.kv_write_oracle(c.spec, k0, v0, c.slots))


@pytest.mark.parametrize("id", [c.id for c in ec.KV_CASES + ec.KV_FP8_CASES])
def test_rope_and_kv_write(id):
    """The fused op against the oracle (fp64 rope -> bf16 -> scatter), not
    against the separate GPU ops: q and k within the rope bound, v and the
    padding bit-unchanged, and the caches bit for bit what the scatter /
    quantisation oracle gives for the k the op itself left in place."""
    c = ec.kv_case(id)
    ref, den = ec.rope_oracle(c.qkv, c.positions, c.cos_sin)
    buf = c.qkv.buf.to(DEV)
    q, k, v = c.qkv.views(buf)
    got = _dev_cache(c.spec)
    ops.rope_and_kv_write(q, k, v, got[0], got[1], c.positions.to(DEV),
                          c.cos_sin.to(DEV), c.slots.to(DEV), got[2], got[3])
    torch.cuda.synchronize()
    m = ec.rope_check_buffer(f"rope_and_kv_write {id}", buf, c.qkv, ref, den, ec.ROPE_BOUND)
    print(f"rope_and_kv_write {id}: metric {m:.6f} (bound {ec.ROPE_BOUND:.5f})")
    _, k_left, v_left = c.qkv.views(buf.cpu())
    _assert_caches(f"rope_and_kv_write {id}", got,
                   ec.kv_write_oracle(c.spec, k_left, v_left, c.slots))
