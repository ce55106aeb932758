"""The host schedule of the fused train step against a recorded ledger (tests/step_ledger.py, tests/golden/step_ledger.json).

The value tests pin what a step computes.  This one pins what they cannot see: which library entry point is enqueued on which stream
(main, s_real, s_gen, the look-ahead's, the reducer's), in which order, and behind which event; which stretches are captured and
replayed as graphs; which spans the gradient reducer is handed and where they are awaited.  A launch moved to another stream, a wait
dropped or added, a host-side query added to the hot path all change the ledger.  Tensor-level torch operations are not recorded
(tests/step_ledger.py says which tests cover them).

Every case runs three step calls from a fresh instructor (the first call allocates, a trunk's second call captures its graph, the
third is the steady state), the GIC_STEP_GRAPH cases four (eager, capture, two replays): B = 4, L = 6, V = 64, E = 16, H = 32, fp32,
device-drawn noise, resnet18 at 32 x 32 and attn_dim 32 where a trunk is needed.

The fixture was recorded on an MI355X from commit 7d00bef ("Pin the data-parallel gradient schedule with a simulated second rank"),
the last one whose fused_step.py wrote the step out twice (FusedAdvStep._body for eager launches, _segments / _call_graph for the
replayed step), with `python -m tests.step_ledger`; two recordings, the cases in either order, agreed.  It is not regenerated from
later code: a driver that disagrees with it has changed the step's schedule."""
import pytest

from tests import step_ledger as SL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return SL.load()


def test_the_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(SL.CASES)


@pytest.mark.parametrize("name", list(SL.CASES))
def test_step_ledger(golden, name):
    got = SL.run_case(name)
    want = golden[name]
    assert len(got) == len(want) == (4 if SL.CASES[name][1].get("graph") else 3)
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            pytest.fail(f"{name}, call {k}: {len(g)} entries against {len(w)} recorded; first difference at entry {i}:\n"
                        f"  got      {g[max(i - 2, 0):i + 3]}\n  recorded {w[max(i - 2, 0):i + 3]}")
