"""The host schedule of one FusedAdvStep call as a list: which library entry point is enqueued on which stream, behind which event.

``recording(fused)`` is a context manager; ``rec.step(...)`` runs one step call and appends its ledger to ``rec.steps``.  An entry is
one of
  ("call", symbol, stream)           a ``gic_*`` function of libgicap.so was called with ``stream`` current (host-only queries included);
  ("record", stream)                 ``Stream.record_event`` (or a bare ``Event.record``, as the gradient reducer uses);
  ("wait", stream, k)                ``Stream.wait_event``: k is the ledger index of the record that made the event, "ext" for an
                                     event from before this call (a pending trunk look-ahead, an earlier synchronous trunk pass);
  ("capture_begin" | "capture_end" | "replay", stream)      ``torch.cuda.CUDAGraph``, the trunk's graph included;
  ("reduce_start", stream, arena, lo, hi)                   ``GradReducer.start`` on ``arena.grad[lo:hi]``;
  ("reduce_wait", stream, k) / ("reduce_wait_all", stream)  k: the ledger index of the ``reduce_start`` whose collective is awaited.
Streams are named by role, never by handle: ``main`` is the stream current at step entry, ``s_real`` / ``s_gen`` are
``fused._streams(dev)``, every other one (the trunk look-ahead's, the reducer's, torch's capture stream) is ``other0``, ``other1``, ...
in order of first appearance within the call.

NOT recorded: tensor-level torch operations (``zero_``, ``cat``, ``roll``, ``copy_``, ``clone``, ``one_hot``) -- the value tests
(tests/test_gpu_step.py, test_gpu_deterministic_steps.py, test_gpu_step_state.py, test_gpu_device_noise.py, test_gpu_dp_schedule.py)
cover what they compute -- and launches inside a replayed graph, which appear once, at capture.

``CASES`` / ``run_case`` are shared by tests/test_gpu_step_ledger.py and by the recorder: ``python -m tests.step_ledger OUT.json``
writes the fixture with the code the test compares with.
"""
from __future__ import annotations

import contextlib
import json
import os
import sys

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_ledger.json")
B, L, V, E, H = 4, 6, 64, 16, 32
BASE = dict(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, compute_dtype="fp32", clip_norm=0.05, adv_train_batch_size=B,
            adv_eval_batch_size=B, num_workers=0, device="cuda", log_file=None, model_dir=None, save_dir=None)
TRUNK = dict(conditional_gan=1, image_size=32, encoder_arch="resnet18")
ATTN = dict(TRUNK, decoder="attention", attn_dim=32)
COND = dict(TRUNK, disc_cond="projection")

# name -> (instructor arguments, options).  Options: env (set while the instructor is built: FusedAdvStep reads them in __init__),
# call (keyword arguments of every step call), ahead (pass the next batch's images), reducer, graph (four calls, not three)
CASES = {
    "lstm-cgan0": (dict(conditional_gan=0), {}),
    "lstm-cgan1-lookahead": (TRUNK, dict(ahead=True)),
    "attention-lookahead": (ATTN, dict(ahead=True)),
    "rsgan": (dict(conditional_gan=0, adv_loss_type="rsgan"), {}),
    "real-as-ids0": (dict(conditional_gan=0, real_as_ids=0), {}),
    "cond-mismatch0.5": (dict(COND, disc_mismatch_weight=0.5), {}),
    "cond-mismatch0": (dict(COND, disc_mismatch_weight=0.0), {}),
    "eval": (dict(conditional_gan=0), dict(call=dict(train=False))),
    "no-opt-step": (dict(conditional_gan=0), dict(call=dict(opt_step=False))),
    "no-stream-overlap": (dict(conditional_gan=0), dict(env={"GIC_NO_STREAM_OVERLAP": "1"})),
    "reducer-lstm": (dict(conditional_gan=0), dict(reducer=True)),
    "reducer-attention": (ATTN, dict(reducer=True)),
    "graph-lstm": (dict(conditional_gan=0), dict(env={"GIC_STEP_GRAPH": "1"}, graph=True)),
    "graph-attention": (ATTN, dict(env={"GIC_STEP_GRAPH_ATTN": "1"}, graph=True)),
}
STEP_ENV = ("GIC_STEP_GRAPH", "GIC_STEP_GRAPH_ATTN", "GIC_NO_STEP_GRAPH", "GIC_NO_GRAPH", "GIC_NO_STREAM_OVERLAP")


class _LibProxy:
    """Stands in for the loaded library: every ``gic_*`` function logs itself, then runs."""

    def __init__(self, real, log):
        self.__dict__["_real"], self.__dict__["_log"] = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gic_"):
            return fn

        def logged(*a):
            self._log("call", name)
            return fn(*a)
        self.__dict__[name] = logged
        return logged


class Recording:
    def __init__(self, fused):
        self.fused = fused
        self.steps = []
        self._cur = None            # the ledger of the call in flight
        self._labels = {}           # stream handle -> role
        self._made = {}             # id(event) -> (event, ledger index); the reference keeps the id from being reused
        self._undo = []

    # ---- naming
    def _label(self, stream=None):
        h = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        if h not in self._labels:
            self._labels[h] = f"other{sum(v.startswith('other') for v in self._labels.values())}"
        return self._labels[h]

    def _log(self, kind, *rest, stream=None):
        if self._cur is None:
            return None
        if kind == "call":
            self._cur.append(("call", rest[0], self._label()))
        else:
            self._cur.append((kind, self._label(stream)) + rest)
        return len(self._cur) - 1

    def _event(self, ev, idx):
        if idx is not None:
            self._made[id(ev)] = (ev, idx)

    def _origin(self, ev):
        hit = self._made.get(id(ev))
        return hit[1] if hit is not None and hit[0] is ev else "ext"

    # ---- patches
    def _patch(self, owner, name, make):
        real = owner.__dict__[name] if name in getattr(owner, "__dict__", {}) else None
        inherited = real is None
        wrapped = make(getattr(owner, name))
        setattr(owner, name, wrapped)
        self._undo.append((owner, name, real, inherited))

    def __enter__(self):
        from gan_image_captioning_amd import _lib
        rec = self
        real_lib = _lib.load()
        _lib._lib = _LibProxy(real_lib, self._log)
        self._undo.append((_lib, "_lib", real_lib, False))
        nested = [0]                # Stream.record_event records through Event.record: one entry, not two

        def record_event(real):
            def f(stream, event=None):
                idx = rec._log("record", stream=stream)
                nested[0] += 1
                try:
                    ev = real(stream, event)
                finally:
                    nested[0] -= 1
                rec._event(ev, idx)
                return ev
            return f

        def event_record(real):
            def f(ev, stream=None):
                if not nested[0]:
                    rec._event(ev, rec._log("record", stream=stream))
                return real(ev, stream)
            return f

        def wait_event(real):
            def f(stream, event):
                rec._log("wait", rec._origin(event), stream=stream)
                return real(stream, event)
            return f

        def graph_call(kind):
            def make(real):
                def f(g, *a, **k):
                    rec._log(kind)
                    return real(g, *a, **k)
                return f
            return make

        self._patch(torch.cuda.Stream, "record_event", record_event)
        self._patch(torch.cuda.Event, "record", event_record)
        self._patch(torch.cuda.Stream, "wait_event", wait_event)
        for kind in ("capture_begin", "capture_end", "replay"):
            self._patch(torch.cuda.CUDAGraph, kind, graph_call(kind))
        red = self.fused.reducer
        if red is not None:
            arenas = {"gen": self.fused.gen_arena, "disc": self.fused.disc_arena}
            started = {}

            def span(flat):
                for name, a in arenas.items():
                    off = (flat.data_ptr() - a.grad.data_ptr()) // flat.element_size()
                    if 0 <= off and off + flat.numel() <= a.grad.numel():
                        return name, off, off + flat.numel()
                return "foreign", 0, flat.numel()

            def start(real):
                def f(flat):
                    idx = rec._log("reduce_start", *span(flat))
                    done = real(flat)
                    if done is not None and idx is not None:
                        started[id(done)] = (done, idx)
                    return done
                return f

            def wait(real):
                def f(done):
                    hit = started.get(id(done))
                    rec._log("reduce_wait", hit[1] if hit is not None and hit[0] is done else "ext")
                    return real(done)
                return f

            def wait_all(real):
                def f():
                    rec._log("reduce_wait_all")
                    return real()
                return f
            self._started = started
            self._patch(red, "start", start)
            self._patch(red, "wait", wait)
            self._patch(red, "wait_all", wait_all)
        return self

    def __exit__(self, *exc):
        for owner, name, real, inherited in reversed(self._undo):
            if inherited:
                delattr(owner, name)
            else:
                setattr(owner, name, real)
        self._undo.clear()
        return False

    # ---- one call
    def step(self, images, captions, max_len, **kw):
        dev = captions.device
        s_real, s_gen = self.fused._streams(dev)
        self._labels = {torch.cuda.current_stream(dev).cuda_stream: "main"}
        self._labels.setdefault(s_real.cuda_stream, "s_real")
        self._labels.setdefault(s_gen.cuda_stream, "s_gen")
        self._made.clear()
        if self.fused.reducer is not None:
            self._started.clear()
        self._cur = []
        try:
            out = self.fused(images, captions, max_len, **kw)
        finally:
            ledger, self._cur = self._cur, None
        self.steps.append(ledger)
        return out


def recording(fused) -> Recording:
    return Recording(fused)


# ------------------------------------------------------------------------------------------------ the cases
@contextlib.contextmanager
def _env(values):
    before = {k: os.environ.get(k) for k in STEP_ENV}
    for k in STEP_ENV:
        os.environ.pop(k, None)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(name, fused_cls=None):
    """The ledgers of the case's step calls (three, graph cases four), as JSON gives them back: lists of lists.
    ``fused_cls``: another FusedAdvStep class to drive the instructor's step with (the parity job's parent copy)."""
    from gan_image_captioning_amd import engine, parallel
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.fused_step import FusedAdvStep
    from gan_image_captioning_amd.generator import SEEDS
    from gan_image_captioning_amd.training import GANInstructor
    from tests import dp_sim
    kw, opt = CASES[name]
    det = engine.deterministic()
    undo = []
    try:
        engine.set_deterministic(False)
        with _env(opt.get("env", {})):
            torch.manual_seed(1008)
            inst = GANInstructor(default_args(**dict(BASE, **kw)), None, None)
            red = parallel.GradReducer(parallel.DistInfo(0, 0, 1), force=True) if opt.get("reducer") else None
            if red is not None or fused_cls is not None:
                inst.fused = (fused_cls or FusedAdvStep)(inst.gen, inst.disc, inst.gen_arena, inst.disc_arena, inst.args,
                                                         red).bind_optimizers(inst.gen_opt, inst.disc_opt)
        inst.gen.train()
        inst.disc.train()
        fused = inst.fused
        if red is not None:                  # the fake collective of tests/dp_sim.py; the second rank's gradient is all zeros
            arenas = {dp_sim.GEN: inst.gen_arena, dp_sim.DISC: inst.disc_arena}
            fake = dp_sim.FakeCollective(arenas, {a: torch.zeros_like(ar.grad) for a, ar in arenas.items()})
            for fn in ("all_reduce", "get_backend"):
                undo.append((fn, getattr(parallel.dist, fn)))
                setattr(parallel.dist, fn, getattr(fake, fn))
        n = 4 if opt.get("graph") else 3
        if opt.get("graph"):
            assert fused.use_graph
            if not fused.attn:           # (the attention engine has one roll-out path and no such query)
                assert fused.dec.fused_rollout_rows() >= B, "device scalars need the LSTM decoder's fused step kernels"
        g = torch.Generator().manual_seed(2024)
        dev = inst.args.device
        body = torch.randint(4, V, (n, B, L - 2), generator=g)
        one = torch.ones(B, 1, dtype=torch.long)
        caps = [torch.cat([one, body[k], 2 * one], 1).to(dev) for k in range(n)]
        images = [None] * (n + 1)
        if int(inst.args.conditional_gan):
            images = [torch.randn(B, 3, 32, 32, generator=g).to(dev) for _ in range(n + 1)]
        SEEDS.reset(77)
        with recording(fused) as rec:
            for k in range(n):
                call = dict(opt.get("call", {}))
                if opt.get("ahead"):
                    call["next_images"] = images[k + 1]
                rec.step(images[k], caps[k], L, **call)
            torch.cuda.synchronize()
        if opt.get("graph"):
            assert len(fused._graphs) == 1 and len(next(iter(fused._graphs.values()))["graphs"]) == 6, "the step was not captured"
        return json.loads(json.dumps(rec.steps))
    finally:
        for fn, real in undo:
            setattr(parallel.dist, fn, real)
        engine.set_deterministic(det)


def dump(ledgers, path):
    """One step call per line."""
    with open(path, "w") as fh:
        fh.write("{\n")
        for i, (name, steps) in enumerate(ledgers.items()):
            lines = ",\n".join("  " + json.dumps(s, separators=(",", ":")) for s in steps)
            fh.write(f" {json.dumps(name)}: [\n{lines}\n ]" + (",\n" if i + 1 < len(ledgers) else "\n"))
        fh.write("}\n")


def load(path=GOLDEN):
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    names = list(CASES)
    if len(sys.argv) > 2 and sys.argv[2] == "reversed":
        names.reverse()
    got = {nm: run_case(nm) for nm in names}
    dump({nm: got[nm] for nm in CASES}, sys.argv[1])
    print("recorded", {nm: [len(s) for s in got[nm]] for nm in CASES})
