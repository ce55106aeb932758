"""A simulated second data-parallel rank on ONE device (no GPU, no process group at import): tools of tests/test_dp_sim.py and
tests/test_gpu_dp_schedule.py.

An average over one rank is the identity, so a one-rank communicator cannot tell an optimizer that waited for its collective from one
that did not, nor a span that was reduced once from one reduced never or twice.  Here the collective is a NON-identity: the production
``GradReducer(DistInfo(0, 0, 1), force=True)`` runs unchanged, and ``parallel.dist.all_reduce`` / ``get_backend`` are replaced
(``attach``) by ``FakeCollective``, which averages the span it is handed with the same span of a second rank's gradient computed
beforehand.  Ordering, coverage and averaging then show up in VALUES:

  * ``FakeCollective``   runs on whatever stream is current when the reducer calls it (the reducer's side stream in the device branch);
                         finds ``flat`` inside one of the arenas' ``grad`` by ``data_ptr()``, writes ``(arena, lo, hi)`` into the ledger,
                         clones its input, optionally enqueues a bounded device-side delay, then ``flat.add_(other[lo:hi]).mul_(0.5)``;
  * ``OptInterceptor``   wraps ``step()`` of every optimizer in play: clones ``arena.grad`` on the stream that is current at the call
                         (exactly what clip + Adam would read), closes the arena's ledger window, then calls the real step or skips it;
  * ``tiling_faults``    between two optimizer steps on an arena the recorded spans must tile [0, numel) exactly once.
"""
from __future__ import annotations

import torch

GEN, DISC = "gen", "disc"


# ------------------------------------------------------------------------------------------------ the ledger
def _owner(lo, hi, arena, names=None):
    """' (inside <parameter k, shape>)' when [lo, hi) lies inside one parameter's slot of ``arena`` (a ParamArena), else ''."""
    if arena is None:
        return ""
    for k, (p, o, n) in enumerate(zip(arena.params, arena.offsets, arena.sizes)):
        end = arena.offsets[k + 1] if k + 1 < len(arena.offsets) else arena.numel
        if o <= lo and hi <= end:
            name = (names or {}).get(id(p), f"params[{k}]")
            return f" (inside {name}, shape {tuple(p.shape)}, grad view [{o}, {o + n}))"
    return ""


def tiling_faults(spans, numel, name="arena", arena=None, names=None):
    """Faults of ``spans`` (a list of (lo, hi)) as a tiling of [0, numel): every element exactly once.  Returns a list of strings, each
    naming the arena and the offending interval: ``gap``, ``overlap``, ``repeat`` (the same span twice), ``outside``.
    ``arena`` (a ParamArena) and ``names`` ({id(parameter): name}) let a fault inside one parameter name it."""
    faults = []
    seen = set()
    for lo, hi in spans:
        if lo < 0 or hi > numel or lo >= hi:
            faults.append(f"{name}: outside: span [{lo}, {hi}) is not a non-empty part of [0, {numel})")
        if (lo, hi) in seen:
            faults.append(f"{name}: repeat: span [{lo}, {hi}) was reduced more than once{_owner(lo, hi, arena, names)}")
        seen.add((lo, hi))
    at = 0
    for lo, hi in sorted(seen):
        if lo > at:
            faults.append(f"{name}: gap: [{at}, {lo}) was never reduced{_owner(at, lo, arena, names)}")
        elif lo < at:
            faults.append(f"{name}: overlap: [{lo}, {min(at, hi)}) was reduced by two different spans{_owner(lo, min(at, hi), arena, names)}")
        at = max(at, hi)
    if at < numel:
        faults.append(f"{name}: gap: [{at}, {numel}) was never reduced{_owner(at, numel, arena, names)}")
    return faults


class Ledger:
    """Per arena: the collectives since the last optimizer step on it (``open``) and the closed windows, one per optimizer step."""

    def __init__(self, names=(GEN, DISC)):
        self.open = {n: [] for n in names}
        self.windows = {n: [] for n in names}

    def add(self, name, rec):
        self.open[name].append(rec)

    def close(self, name):
        w, self.open[name] = self.open[name], []
        self.windows[name].append(w)
        return w


# ------------------------------------------------------------------------------------------------ the collective
class Delay:
    """A fixed, bounded device-side delay of about ``ms`` milliseconds on the current stream: ``torch.cuda._sleep`` with a cycle count
    calibrated once (and clamped), or a fixed chain of element-wise passes where that is unavailable.  No host condition is involved."""

    def __init__(self, ms=2.0):
        self.ms = float(ms)
        self.cycles = None
        self.chain = None

    def _calibrate(self):
        sleep = getattr(torch.cuda, "_sleep", None)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):                       # the shortest of three: whatever else the device is doing only lengthens a measurement
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0.record(); fn(); t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1)
                best = ms if best is None else min(best, ms)
            return max(best, 1e-3)
        if sleep is not None:
            probe = 200_000
            sleep(probe)                     # first launch: code-object load
            per = timed(lambda: sleep(probe)) / probe
            self.cycles = int(min(max(self.ms / per, 10_000), 50_000_000))       # clamped: a 100 MHz .. 3 GHz clock stays bounded
        else:
            x = torch.zeros(1 << 22, device="cuda")
            x.add_(1.0)

            def chain():
                for _ in range(16):
                    x.add_(1.0)
            per = timed(chain) / 16
            self.chain = (x, int(min(max(self.ms / per, 1), 2000)))

    def __call__(self):
        if self.cycles is None and self.chain is None:
            self._calibrate()
        if self.cycles is not None:
            torch.cuda._sleep(self.cycles)
        else:
            x, n = self.chain
            for _ in range(n):
                x.add_(1.0)


def concurrent_stream(others, delay, tries=10, log=None):
    """A new stream on which work runs CONCURRENTLY with each stream of ``others``, found by measurement, or None.

    Streams share a small number of hardware queues, and two streams on one queue run in submission order: a missing wait between
    them then changes nothing, and forced timing shows nothing.  Which streams share a queue depends on how many the process has
    created before, so it is probed: ``delay`` is enqueued on one stream, a small launch and an event on the other right behind it;
    the pair is concurrent when that event completes in under half the delay while the delay itself lasts at least half of what was asked for
    (both directions).  Rejected candidates are kept alive until the search ends, so that later ones land on other queues; the last
    two candidates are high-priority streams, which have queues of their own."""
    tick = torch.zeros(64, device="cuda")

    def overtakes(sleeper, other):
        torch.cuda.synchronize()
        t0, e_s, e_o = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t0.record(other)
        with torch.cuda.stream(sleeper):
            delay()
            e_s.record(sleeper)
        with torch.cuda.stream(other):       # a real launch in front of the event: it takes its place in the hardware queue
            tick.add_(1.0)
            e_o.record(other)
        torch.cuda.synchronize()
        return t0.elapsed_time(e_o) < 0.5 * delay.ms and t0.elapsed_time(e_s) >= 0.5 * delay.ms

    kept = []
    for k in range(tries):
        cand = torch.cuda.Stream(priority=-1) if k >= tries - 2 else torch.cuda.Stream()
        kept.append(cand)
        if all(overtakes(cand, o) and overtakes(o, cand) for o in others):
            if log is not None:
                log.append(k + 1)            # how many candidates it took
            return cand
    return None


class FakeCollective:
    """``all_reduce`` of a two-rank pair of which this process is rank 0.  ``arenas``: {name: ParamArena} (anything with ``grad`` and
    ``numel``); ``other``: {name: the second rank's flat gradient of that arena}; ``delay``: callable enqueueing a bounded delay on the
    current stream before ``flat`` is touched, or None.  ``world``: the reducer's world size -- its CPU branch sums and then scales by
    1 / world, its device branch asks for the average; either way ``flat`` ends as ``(flat + other) * 0.5`` (two f32 operations)."""

    def __init__(self, arenas, other, ledger=None, delay=None, world=1):
        self.arenas, self.other, self.delay, self.world = arenas, other, delay, int(world)
        self.ledger = ledger if ledger is not None else Ledger(tuple(arenas))

    def locate(self, flat):
        esz = flat.element_size()
        for name, a in self.arenas.items():
            off = flat.data_ptr() - a.grad.data_ptr()
            if off >= 0 and off % esz == 0 and off // esz + flat.numel() <= a.grad.numel() and flat.is_contiguous():
                return name, off // esz, off // esz + flat.numel()
        raise AssertionError(f"foreign tensor: a collective was started on {flat.numel()} elements at {flat.data_ptr():#x}, which lie "
                             f"in no gradient arena ({', '.join(self.arenas)})")

    def get_backend(self, *a, **k):
        return "nccl"

    def all_reduce(self, flat, op=None, **kw):
        name, lo, hi = self.locate(flat)
        rec = {"arena": name, "lo": lo, "hi": hi, "in": flat.clone()}
        self.ledger.add(name, rec)
        if self.delay is not None:
            self.delay()
        flat.add_(self.other[name][lo:hi])
        # ReduceOp.AVG (device branch): the average itself.  ReduceOp.SUM (CPU branch): the reducer multiplies by 1 / world afterwards
        is_sum = op is not None and "SUM" in str(op).upper()
        flat.mul_(0.5 * self.world if is_sum else 0.5)
        return None


# ------------------------------------------------------------------------------------------------ the optimizer interceptor
class OptInterceptor:
    """Wraps ``step`` of the optimizers ``opts`` ({label: (arena name, optimizer)}; an optimizer is anything with ``arena`` and ``step``).
    ``mode``: "call" | "skip".  ``seen[arena name]``: the clones of ``arena.grad`` taken at each intercepted step, in order;
    ``calls``: the labels in call order."""

    def __init__(self, opts, ledger=None, mode="call"):
        assert mode in ("call", "skip")
        self.mode, self.ledger = mode, ledger
        self.seen = {}
        self.calls = []
        self._real = {}
        for label, (aname, opt) in opts.items():
            self.seen.setdefault(aname, [])
            self._real[label] = (opt, opt.step)
            opt.step = self._wrap(label, aname, opt, opt.step)

    def _wrap(self, label, aname, opt, real):
        def step():
            self.seen[aname].append(opt.arena.grad.clone())       # on the current stream: what clip + Adam would read
            self.calls.append(label)
            if self.ledger is not None:
                self.ledger.close(aname)
            if self.mode == "call":
                real()
        return step

    def restore(self):
        for opt, real in self._real.values():
            opt.step = real


def attach(monkeypatch, fake):
    """Route the production reducer's collective through ``fake``: nothing else of ``GradReducer.start`` changes (event record, side
    stream, ``record_stream``, ``_pending``)."""
    from gan_image_captioning_amd import parallel
    monkeypatch.setattr(parallel.dist, "all_reduce", fake.all_reduce)
    monkeypatch.setattr(parallel.dist, "get_backend", fake.get_backend)


def averaging_faults(window, other, seen, name):
    """Check (b): the gradient the optimizer read (``seen``) equals ``(in + other[lo:hi]) * 0.5`` on every span of ``window``, bit for bit."""
    faults = []
    for rec in window:
        lo, hi = rec["lo"], rec["hi"]
        want = (rec["in"] + other[lo:hi]) * 0.5
        got = seen[lo:hi]
        if not torch.equal(got, want):
            n = int((got != want).sum())
            raw = " (it read the un-reduced gradient)" if torch.equal(got, rec["in"]) else ""
            faults.append(f"{name}: the optimizer did not read the average on [{lo}, {hi}): {n} of {hi - lo} elements differ{raw}")
    return faults
