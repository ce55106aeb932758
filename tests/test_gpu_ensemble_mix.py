"""ensemble_mix on the GPU (csrc/ensemble.hip through engine.ensemble_mix): every case of tests/ensemble_cases.py element-wise against
the fp64 reference within the derived bound, the two row forms, both modes; M = 1 against log_softmax; two calls give the same bits."""
import pytest
import torch

from tests import ensemble_cases as EC
from tests.aux_cases import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def worst():
    seen = {}
    yield seen
    print("\nensemble_mix largest err / bound per mode:", {k: round(v, 4) for k, v in seen.items()})


def _run(case, dev):
    from gan_image_captioning_amd import engine
    x, w = EC.make_inputs(case)
    z = engine.ensemble_mix(x.to(dev), None if case.weights is None else w, case.mode)
    torch.cuda.synchronize()
    return x, w, z


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.id)
def test_case_inside_the_bound(dev, worst, case):
    x, w, z = _run(case, dev)
    assert z.shape == (case.rows, case.V) and z.dtype == torch.float32
    assert torch.isfinite(z).all()
    ratio = EC.check_case(case, z.cpu(), x, w)
    print(f"{case.id}: err / bound {ratio:.4f}")
    worst[case.mode] = max(worst.get(case.mode, 0.0), ratio)


@pytest.mark.parametrize("mode", EC.MODES)
@pytest.mark.parametrize("V", [5, 67, 1028, 10000])
def test_one_member_is_log_softmax(dev, mode, V):
    case = EC.Case(f"{mode}-one-V{V}", 1, 3, V, mode, None)
    x, w, z = _run(case, dev)
    check("ensemble_mix", case.id, "z", z.cpu(), torch.log_softmax(x[0].double(), -1), EC.bound(x, w, mode))


@pytest.mark.parametrize("cid", ["prob-M4-r65-V10000", "logprob-M4-r65-V10000", "prob-M2-r65-V67", "logprob-M3-uneven"])
def test_two_calls_give_the_same_bits(dev, cid):
    from gan_image_captioning_amd import engine
    case = EC.BY_ID[cid]
    x, w = EC.make_inputs(case)
    xd = x.to(dev)
    a = engine.ensemble_mix(xd, w, case.mode)
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        b = engine.ensemble_mix(xd, w, case.mode)
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_prob_mode_is_normalised_and_underflow_adds_nothing(dev):
    case = EC.BY_ID["prob-dominate"]
    x, w, z = _run(case, dev)
    assert float(torch.logsumexp(z.double(), -1).abs().max()) < 1e-5
    case = EC.BY_ID["logprob-dominate"]
    x, w, z = _run(case, dev)
    assert torch.isfinite(z).all() and float(z[:, 0].max()) < -0.7 * 104.0        # member 0's true log-probability, not a clamp
