"""The simulated second rank's own tools (tests/dp_sim.py), on the CPU: the ledger check on made-up span lists, the fake collective
through ``GradReducer``'s CPU branch, the optimizer interceptor's two modes."""
import pytest
import torch

from tests import dp_sim as S


class _Arena:
    """The two members of a ParamArena that the collective reads."""

    def __init__(self, n):
        self.grad = torch.zeros(n)
        self.numel = n


# ------------------------------------------------------------------------------------------------ ledger
@pytest.mark.parametrize("spans", [[(0, 10)], [(4, 7), (0, 4), (7, 10)], [(0, 1), (1, 10)]])
def test_ledger_accepts_an_exact_tiling(spans):
    assert S.tiling_faults(spans, 10, "gen") == []


@pytest.mark.parametrize("spans,kind,interval", [
    ([(0, 4), (7, 10)], "gap", "[4, 7)"),                 # a span in the middle never reduced
    ([(0, 4), (4, 7)], "gap", "[7, 10)"),                 # the tail dropped
    ([(4, 10)], "gap", "[0, 4)"),                         # the head dropped
    ([], "gap", "[0, 10)"),                               # no collective at all
    ([(0, 6), (4, 10)], "overlap", "[4, 6)"),
    ([(0, 10), (0, 10)], "repeat", "[0, 10)"),            # the whole arena reduced twice
    ([(0, 4), (4, 10), (4, 10)], "repeat", "[4, 10)"),
    ([(0, 12)], "outside", "[0, 12)"),
])
def test_ledger_flags_gap_overlap_and_double_reduction(spans, kind, interval):
    faults = S.tiling_faults(spans, 10, "disc")
    assert faults, spans
    assert any(f.startswith("disc: " + kind) and interval in f for f in faults), faults


def test_ledger_names_the_parameter_a_fault_falls_into(monkeypatch):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.optim import ParamArena
    monkeypatch.setattr(engine, "require_gpu", lambda *t: None)       # the arena's layout alone: no kernel runs here
    w, b = torch.nn.Parameter(torch.ones(3, 2)), torch.nn.Parameter(torch.ones(5))
    arena = ParamArena([w, b])
    assert arena.offsets == [0, 8] and arena.numel == 16
    names = {id(w): "lin.weight", id(b): "lin.bias"}
    faults = S.tiling_faults([(0, 8)], arena.numel, "gen", arena, names)
    assert len(faults) == 1 and "gap: [8, 16)" in faults[0] and "lin.bias" in faults[0] and "(5,)" in faults[0], faults
    faults = S.tiling_faults([(0, 16), (0, 8)], arena.numel, "gen", arena, names)
    assert any("overlap" in f and "lin.weight" in f for f in faults), faults


def test_collective_refuses_a_foreign_tensor():
    a = _Arena(16)
    fake = S.FakeCollective({S.GEN: a}, {S.GEN: torch.ones(16)})
    with pytest.raises(AssertionError, match="foreign tensor"):
        fake.all_reduce(torch.zeros(4))
    with pytest.raises(AssertionError, match="foreign tensor"):
        fake.all_reduce(a.grad[::2])                                    # strided: not a span
    assert fake.locate(a.grad[4:12]) == (S.GEN, 4, 12)


# ------------------------------------------------------------------------------------------------ collective through the reducer
@pytest.mark.parametrize("world", [1, 2])
def test_fake_collective_averages_through_the_reducers_cpu_branch(monkeypatch, world):
    from gan_image_captioning_amd import parallel
    g = torch.Generator().manual_seed(3)
    arenas = {S.GEN: _Arena(24), S.DISC: _Arena(12)}
    mine = {k: torch.randn(a.numel, generator=g) for k, a in arenas.items()}
    other = {k: torch.randn(a.numel, generator=g) for k, a in arenas.items()}
    for k, a in arenas.items():
        a.grad.copy_(mine[k])
    fake = S.FakeCollective(arenas, other, world=world)
    S.attach(monkeypatch, fake)
    red = parallel.GradReducer(parallel.DistInfo(0, 0, world), force=True)
    assert red.start(arenas[S.GEN].grad[8:16]) is None                   # synchronous branch
    red.start(arenas[S.DISC].grad)
    red.start(arenas[S.GEN].grad[:8])
    red.start(arenas[S.GEN].grad[16:])
    red.wait_all()
    for k, a in arenas.items():
        assert torch.equal(a.grad, (mine[k] + other[k]) * 0.5), k
        spans = [(r["lo"], r["hi"]) for r in fake.ledger.open[k]]
        assert S.tiling_faults(spans, a.numel, k) == []
        for r in fake.ledger.open[k]:
            assert torch.equal(r["in"], mine[k][r["lo"]:r["hi"]])
        assert S.averaging_faults(fake.ledger.open[k], other[k], a.grad, k) == []
    # a gradient that was NOT averaged is reported
    stale = mine[S.GEN].clone()
    faults = S.averaging_faults(fake.ledger.open[S.GEN], other[S.GEN], stale, S.GEN)
    assert len(faults) == 3 and all("un-reduced" in f for f in faults), faults


# ------------------------------------------------------------------------------------------------ interceptor
class _SGD:
    def __init__(self, arena):
        self.arena, self.steps = arena, 0

    def step(self):
        self.arena.flat.sub_(self.arena.grad)
        self.steps += 1


@pytest.mark.parametrize("mode", ["call", "skip"])
def test_interceptor_snapshots_closes_the_window_and_calls_or_skips(monkeypatch, mode):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.optim import ParamArena
    monkeypatch.setattr(engine, "require_gpu", lambda *t: None)
    arena = ParamArena([torch.nn.Parameter(torch.ones(3, 2)), torch.nn.Parameter(torch.ones(5))])
    opt_a, opt_b = _SGD(arena), _SGD(arena)                              # two optimizers on one arena, as pretrain_opt / gen_opt
    ledger = S.Ledger((S.GEN,))
    ic = S.OptInterceptor({"a": (S.GEN, opt_a), "b": (S.GEN, opt_b)}, ledger, mode)
    before = arena.flat.clone()
    arena.grad.fill_(0.25)
    ledger.add(S.GEN, {"lo": 0, "hi": arena.numel})
    opt_a.step()
    arena.grad.fill_(0.5)                                                # the snapshot is a copy: later writes do not reach it
    opt_b.step()
    assert ic.calls == ["a", "b"]
    assert torch.equal(ic.seen[S.GEN][0], torch.full((arena.numel,), 0.25)) and torch.equal(ic.seen[S.GEN][1], torch.full((arena.numel,), 0.5))
    assert [len(w) for w in ledger.windows[S.GEN]] == [1, 0] and ledger.open[S.GEN] == []
    if mode == "call":
        assert (opt_a.steps, opt_b.steps) == (1, 1) and torch.equal(arena.flat, before - 0.75)
    else:
        assert (opt_a.steps, opt_b.steps) == (0, 0) and torch.equal(arena.flat, before)
    ic.restore()
    opt_a.step()
    assert opt_a.steps == (2 if mode == "call" else 1) and len(ic.calls) == 2
