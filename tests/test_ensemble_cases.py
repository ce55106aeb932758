"""tests/ensemble_cases.py without a GPU: the fp64 reference against torch's operators, the f32 emulation of ensemble_mix inside the
derived bound at every case, and the seeded faults outside it."""
import pytest
import torch

from tests import ensemble_cases as EC
from tests.aux_cases import Mismatch

# the emulation of the largest rows at V = 10000 adds nothing to what rows = 3 shows of the kernel's order; the GPU runs them all
EMULATED = [c for c in EC.CASES if not (c.V == 10000 and c.rows == 65)]


def test_case_table_covers_the_issue():
    ids = {c.id for c in EC.CASES}
    assert len(ids) == len(EC.CASES)
    for mode in EC.MODES:
        cs = [c for c in EC.CASES if c.mode == mode]
        assert {c.rows for c in cs} >= {1, 3, 65}
        assert {c.V for c in cs} >= {2, 5, 64, 67, 1028, 10000}
        assert {c.M for c in cs} >= {1, 2, 3, 4}
        assert any(c.weights == (0.7, 0.2, 0.1) for c in cs) and any(c.weights is None for c in cs)
        assert any(c.scale == 1e4 for c in cs) and any(c.scale == 80.0 for c in cs)
        assert any(c.special == "const" for c in cs) and any(c.special == "dominate" for c in cs)
    assert {EC.lanes(c.V) for c in EC.CASES} == {64, 256}            # both row forms


def test_reference_is_the_definition():
    x, w = EC.make_inputs(EC.BY_ID["prob-M3-uneven"])
    lp = torch.log_softmax(x.double(), -1)
    wn = torch.tensor(w, dtype=torch.float32).double()              # the library reads the weights as f32
    wn = wn / wn.sum()
    p = (lp.exp() * wn.view(-1, 1, 1)).sum(0)
    assert torch.allclose(EC.reference(x, w, "prob"), p.log(), rtol=0, atol=1e-12)
    assert torch.allclose(EC.reference(x, w, "prob").exp().sum(-1), torch.ones(3, dtype=torch.float64), atol=1e-12)      # normalised
    assert torch.allclose(EC.reference(x, w, "logprob"), (lp * wn.view(-1, 1, 1)).sum(0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", EC.MODES)
def test_one_member_is_log_softmax(mode):
    x, w = EC.make_inputs(EC.BY_ID[f"{mode}-M1-r3-V67"])
    assert torch.allclose(EC.reference(x, w, mode), torch.log_softmax(x[0].double(), -1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", EC.MODES)
def test_underflowing_member(mode):
    """Where member 0's probability underflows it adds nothing in prob and its true log-probability in logprob."""
    case = EC.BY_ID[f"{mode}-dominate"]
    x, w = EC.make_inputs(case)
    z = EC.emulate(x, w, mode)
    assert torch.isfinite(z).all()
    lp = torch.log_softmax(x.double(), -1)
    assert float(lp[0, :, 0].max()) < -104.0                         # exp underflows in f32
    wn, logw = EC.normalised(w)
    if mode == "prob":
        rest = torch.logsumexp(lp[1:, :, 0] + torch.from_numpy(logw[1:]).view(-1, 1), 0)
        assert torch.allclose(z[:, 0].double(), rest, rtol=0, atol=1e-4)
    else:
        assert float((z[:, 0].double() - (lp[:, :, 0] * torch.from_numpy(wn).view(-1, 1)).sum(0)).abs().max()) < 1e-3
        assert float(z[:, 0].max()) < -0.7 * 104.0


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.id)
def test_emulation_inside_the_bound(case):
    x, w = EC.make_inputs(case)
    z = EC.emulate(x, w, case.mode)
    assert torch.isfinite(z).all()
    assert EC.check_case(case, z, x, w) <= 1.0


@pytest.mark.parametrize("mode", EC.MODES)
@pytest.mark.parametrize("fault", EC.FAULTS)
def test_seeded_fault_outside_the_bound(fault, mode):
    case = EC.BY_ID[f"{mode}-{EC.FAULT_CASES[fault]}"]
    x, w = EC.make_inputs(case)
    EC.check_case(case, EC.emulate(x, w, case.mode), x, w)            # the sound kernel passes this very case
    with pytest.raises(Mismatch):
        EC.check_case(case, EC.emulate(x, w, case.mode, fault=fault), x, w)


def test_bound_is_tight_enough_to_mean_something():
    """At the workload's V and logits of magnitude 80 the bound stays below 1e-3 nats: far under any selection margin the search
    tests compare at (1e-4 is their threshold for ids; scores are compared at 1e-3)."""
    for mode in EC.MODES:
        case = EC.BY_ID[f"{mode}-M2-r3-V10000"]
        x, w = EC.make_inputs(case)
        assert float(EC.bound(x, w, mode).max()) < 1e-3
