"""GPU edge tests of the sampling kernels (csrc/sampling.hip) against the
fp64 oracles of elem_cases.py: greedy ties inside a wave, across waves,
across splits and in the combine kernel, -inf rows, small V with empty
splits, Gumbel-max rows whose fp64 winner leads by a recorded gap (so the
index must match exactly), and the top-k/top-p filter on random, peaked,
tied, pre-masked and deep rows. test_elem_cases_cpu.py proves on the CPU
that the inputs decide the answer and that each listed mistake changes it."""

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


@pytest.mark.parametrize("id", [c.id for c in ec.SAMPLE_CASES])
def test_sample(id):
    c = ec.sample_case(id)
    B, V = c.logits.shape
    want = ec.sample_oracle(ec.sample_scores(c.logits, c.temperature, c.noise))
    logits = c.logits.to(DEV)
    got = ops.sample(logits, c.temperature.to(DEV),
                     None if c.noise is None else c.noise.to(DEV))
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(ec.bits(logits), ec.bits(c.logits)), "sample changed the logits"
    assert bool(((got >= 0) & (got < V)).all()), f"{id}: index out of range: {got.tolist()}"
    wrong = (got != want).nonzero().flatten().tolist()
    print(f"sample {id}: {B - len(wrong)} of {B} rows match")
    assert not wrong, (
        f"{id}: rows {wrong}: got {got[wrong].tolist()}, oracle {want[wrong].tolist()}")


@pytest.mark.parametrize("id", [c.id for c in ec.FILTER_CASES])
def test_topk_topp_filter(id):
    c = ec.filter_case(id)
    oracle = ec.filter_oracle(c)
    logits = c.logits.to(DEV)
    out = ops.topk_topp_filter(logits, c.topp.to(DEV), c.topk.to(DEV))
    torch.cuda.synchronize()
    assert out.data_ptr() == logits.data_ptr()
    after = logits.cpu()
    failures = []
    for b, (fr, o) in enumerate(zip(c.rows, oracle)):
        tag = f"filter {id} row {b} ({fr.kind}, p={float(c.topp[b]):g}, k={int(c.topk[b])})"
        kept = int((after[b] != ec.NEG_INF).sum())
        print(f"{tag}: kept {kept}, oracle {int((o.keep & torch.isfinite(c.logits[b])).sum())}")
        try:
            ec.filter_check_row(tag, fr, c.logits[b], after[b], o)
        except AssertionError as e:  # report every row, then fail
            failures.append(str(e))
    assert not failures, "\n".join(failures)
