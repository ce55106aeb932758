"""Device-drawn noise, pinned: every kernel that draws its own uniforms (Philox4x32-10, csrc/common.h) against the same launch given
the uniforms / keep masks the host replica computes (tests/philox_ref.py, anchored in tests/test_philox_ref.py).  A kernel differs
between its two modes only in where `u` comes from, and u01 = k 2^-24 is exact in float32: so the two launches must agree BIT FOR BIT
in everything they write.  No tolerance, no exempted elements.  That carries everything the explicit-noise path is pinned against
(the oracles of the other test modules) over to the path that training and bench.py run.

Every case first shows that two explicit launches give equal bits (so a nondeterministic launch is not misread as a noise mismatch:
the LSTM decoder's and the discriminator's bf16 products and both composed steps run in deterministic mode, whose sums are
order-independent; the attention decoder refuses that mode and needs none, like the scheduled-sampling decode: their products never
split) and, where the launch goes through the GEMM selection, that both modes select the same kernel (engine.route_only: the line of
the last product the call selects).  A route-only pass skips the products and still launches everything else, so it runs on zeroed
buffers (or, the composed step, on those a complete step has just filled): nothing then indexes by an uninitialised value.  The fused
step kernels (lstm_step / vocab_step / sample_finish) are not selected per call: decoder_fused_rows is a function of the shapes
alone; nor are the segments of the replayed graphs, which make the calls of the eager step.  Two seeds everywhere: 1 and one with a non-zero upper
half; the two must give different results (the comparison is not vacuous).

Which case reaches which Philox::gen / gen4 call site (DESIGN.md section 2 has the same table):
  decoder.hip  gumbel_softmax_argmax_kernel (gen)        test_lstm_separate_launches[scalar-*], test_teacher_forced_with_noise
  decoder.hip  gumbel_softmax_argmax_reg_kernel (gen4)   test_lstm_separate_launches[reg-*], test_gumbelmax_threshold[384], test_attn_rollout
  decoder_step.hip  vocab_step (gen4)                    test_lstm_fused_rollout, test_attn_fused_rollout, test_composed_step
  gemm.hip  EPI_GUMBELMAX (gen4)                         test_gumbelmax_threshold[385], test_attn_rollout[386]
  gemm_device.h  highway_keep4 (gen4)                    test_highway_dropout (gemm_kernel, tile8 and the redrop kernel), test_composed_step
  sample.hip  sample_select (gen4)                       test_sample_logits, test_sample_captions
  sched_sample.hip  coin (gen4), vector noise (gen4), scalar noise (gen)   test_scheduled_sampling[V = 12: vector; V = 70: scalar]

The module prints its wall time after every run under -s."""
import contextlib
import functools
import time

import numpy as np
import pytest
import torch

from tests import attn_cases as A
from tests import decoder_cases as D
from tests import disc_cases as DC
from tests import philox_ref as R
from tests import sched_sample_cases as SC
from tests.disc_cases import HIGHWAY, TD
from tests.golden_io import Golden, initial_params
from tests.test_gpu_disc_stages import alloc_state as disc_alloc_state
from tests.test_gpu_disc_stages import assert_guards as disc_assert_guards
from tests.test_gpu_disc_stages import live as disc_live
from tests.test_gpu_disc_stages import make_engine as disc_make_engine
from tests.test_gpu_step import load_params, make_instructor

pytestmark = pytest.mark.gpu

SEEDS = (1, 0x9E3779B97F4A7C15)                                  # the second: a non-zero upper half
SLOT_SEEDS = SEEDS + (0xD1B54A32D192ED03, 0x0123456789ABCDEF)    # four different seeds for the four gic_step_scalars slots
DT = {"f32": 0, "bf16": 1}
DTYPES = ("f32", "bf16")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[device noise] wall time of the module: {time.perf_counter() - t0:.1f} s")


def stops_on_fault(test):
    """A GPU fault (not a wrong result) ends the run: nothing more is launched on a device that has faulted."""
    @functools.wraps(test)
    def wrapped(*a, **kw):
        try:
            return test(*a, **kw)
        except RuntimeError as exc:
            if "HIP error" in str(exc) or "illegal memory access" in str(exc):
                pytest.exit(f"GPU fault: {exc}", returncode=3)
            raise
    return wrapped


@contextlib.contextmanager
def det_mode(E, on):
    before = E.deterministic()
    E.set_deterministic(bool(on))
    try:
        yield
    finally:
        E.set_deterministic(before)


# ---------------------------------------------------------------------------------------------------------------- comparing bits
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    t = t.detach().contiguous()
    return t.view(_INT[t.element_size()]) if t.is_floating_point() else t


def flat(x, name="", out=None):
    """Every tensor inside nested dicts / lists / tuples, with a name."""
    out = [] if out is None else out
    if torch.is_tensor(x):
        out.append((name, x))
    elif isinstance(x, dict):
        for k in sorted(x):
            flat(x[k], f"{name}.{k}" if name else str(k), out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            flat(v, f"{name}[{i}]", out)
    return out


def same_bits(a, b, what):
    fa, fb = flat(a), flat(b)
    assert [n for n, _ in fa] == [n for n, _ in fb], what
    assert fa, what
    bad = []
    for (n, x), (_, y) in zip(fa, fb):
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {n}"
        if not torch.equal(bits(x), bits(y)):
            ne = (bits(x) != bits(y)).reshape(-1)
            first = int(ne.nonzero()[0])
            bad.append(f"{n} differs in {int(ne.sum())} of {ne.numel()} elements, the first at flat index {first}: "
                       f"{x.reshape(-1)[first].item()!r} != {y.reshape(-1)[first].item()!r}")
    assert not bad, f"{what}: " + "; ".join(bad)


def differs(a, b):
    return any(not torch.equal(bits(x), bits(y)) for (_, x), (_, y) in zip(flat(a), flat(b)))


def on(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def twin(run, make_noise, dev, what, seeds=SEEDS):
    """The pattern of every case.  run(seed=s) draws on the device, run(noise=...) takes the host's tensors; per seed: two explicit runs
    agree, the device run equals them; across seeds: the results differ.  Returns the explicit results."""
    res = []
    for s in seeds:
        noise = make_noise(s)
        a, b = run(noise=noise), run(noise=noise)
        same_bits(a, b, f"{what}, seed {s:#x}: two explicit launches")
        same_bits(run(seed=s), a, f"{what}, seed {s:#x}: device-drawn launch vs the host's uniforms")
        res.append(a)
    for i in range(1, len(res)):
        assert differs(res[0], res[i]), f"{what}: seeds {seeds[0]:#x} and {seeds[i]:#x} give the same result"
    return res


def same_route(E, run, noise, seed, what):
    """Both modes select the same kernel: the line of the last product the call selected (the vocabulary product of the last step)."""
    with E.route_only() as r:
        run(seed=seed)
        line_dev = r.last()
    with E.route_only() as r:
        run(noise=noise)
        line_exp = r.last()
    assert line_dev == line_exp and line_dev, f"{what}: device-drawn {line_dev!r}, explicit {line_exp!r}"
    return line_dev


def zeroed(st):
    """A state whose every buffer starts at zero: what a launch does not write compares equal, and a route-only pass (whose products
    are skipped) leaves the element-wise kernels finite zeros to read."""
    for _, t in flat(st):
        t.zero_()
    return st


# ---------------------------------------------------------------------------------------------------------------- LSTM roll-out
@functools.lru_cache(maxsize=None)
def lstm_problem(B, L, V, dtype, part=True):
    case = D.Case("noise", B, L, V, 8, 8, 1, dtype, "", part=part)
    gen = torch.Generator().manual_seed(D.SEED)
    P = D.make_params(case, gen)
    feats = torch.randn(B, case.E, generator=gen)
    return case, P, feats


def lstm_runner(E, dev, case, P, feats, ids_only=False, scal=None, slot=0):
    eng = E.DecoderEngine(case.V, case.E, case.H, case.NL, DT[case.dtype])
    params, f = [p.to(dev) for p in P], feats.to(dev)

    def run(seed=0, noise=None):
        st = zeroed(eng.alloc_state(case.B, case.L, dev))
        if not case.part:
            st["part"] = None
        out = torch.zeros(case.B, case.L, case.V, device=dev, dtype=TD[case.dtype])
        ids = torch.full((case.B, case.L), -7, device=dev, dtype=torch.int64)
        eng.sample_fwd(params, f, case.L, D.TEMPERATURE, False, noise_u=noise, seed=seed, state=st, out=out, ids=ids, ids_only=ids_only,
                       dev_scalars=scal, seed_slot=slot)
        torch.cuda.synchronize()
        res = {"ids": ids, "state": {k: v for k, v in st.items() if v is not None}}
        if not ids_only:
            res["out"] = out
        return res
    return eng, run


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [68, 260])
@pytest.mark.parametrize("B", [1, 17, 65])
@stops_on_fault
def test_lstm_fused_rollout(E, dev, B, V, dtype):
    """lstm_step / vocab_step / sample_finish: the tails of the 16- and 64-caption sub-tiles, a 64-entry vocabulary tile plus a 4-entry
    tail and several tiles, three steps (stream t).  ids, probabilities and the whole saved state (x | h rows, gates, cell states,
    hout, the tile partials and argmax keys).  Then the seed through gic_step_scalars: slot k holds seed k, every slot is read."""
    case, P, feats = lstm_problem(B, 3, V, dtype)
    assert D.select(case)["fwd"] == "fused"
    with det_mode(E, dtype == "bf16"):
        eng, run = lstm_runner(E, dev, case, P, feats)
        assert B <= eng.fused_rollout_rows()
        res = twin(run, lambda s: on(R.rollout_us(s, case.L, B, V), dev), dev, f"fused roll-out B={B} V={V} {dtype}")
        scal = E.StepScalarsBuffer(dev)
        scal.set(D.TEMPERATURE, SLOT_SEEDS)
        want = {s: r for s, r in zip(SEEDS, res)}
        for slot, s in enumerate(SLOT_SEEDS):
            if s not in want:
                want[s] = run(noise=on(R.rollout_us(s, case.L, B, V), dev))
            _, run_slot = lstm_runner(E, dev, case, P, feats, scal=scal, slot=slot)
            same_bits(run_slot(seed=SLOT_SEEDS[(slot + 1) % 4]), want[s], f"fused roll-out B={B} V={V} {dtype}: the seed of slot {slot}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,B,V,L", [("reg", 513, 8, 2), ("reg", 513, 4100, 2), ("scalar", 3, 70, 3), ("scalar", 3, 257, 3)],
                         ids=["reg-b513-v8", "reg-b513-v4100", "scalar-v70", "scalar-v257"])
@stops_on_fault
def test_lstm_separate_launches(E, dev, kind, B, V, L, dtype):
    """The roll-out as separate products and launches.  reg: one row past the fused kernels' limit (crossed by shape), the register
    kernel with one quad per thread and, at V = 4100, a second quad for thread 0.  scalar: V % 4 != 0, where a counter's four lanes
    straddle two rows (70 = 17 * 4 + 2) and, at V = 257, a thread makes a second pass."""
    case, P, feats = lstm_problem(B, L, V, dtype)
    sel = D.select(case)
    assert sel["fwd"] == "generic" and sel["argmax"] == {"reg": "reg4" if V > 4096 else "reg1", "scalar": "scalar"}[kind]
    with det_mode(E, dtype == "bf16"):
        eng, run = lstm_runner(E, dev, case, P, feats)
        assert eng.fused_rollout_rows() == (B - 1 if kind == "reg" else 0)       # one row past the limit / shapes the step kernels decline
        make = lambda s: on(R.rollout_us(s, L, B, V), dev)
        same_route(E, run, make(SEEDS[0]), SEEDS[0], f"separate launches {kind} B={B} V={V} {dtype}")
        twin(run, make, dev, f"separate launches {kind} B={B} V={V} {dtype}")


@pytest.mark.parametrize("rows", [385, 384])
@stops_on_fault
def test_gumbelmax_threshold(E, dev, rows):
    """bf16, ids only, V = 5120: from 385 rows the vocabulary product carries the Gumbel-max in its epilogue (40 x 4 tiles of 128 x 128,
    row and column tails; operands swapped: counter n (M >> 2) + (m0 >> 2)); at 384 rows the same call falls back to the plain product
    and the register kernel.  Both against the SAME host map: the two index the draw alike."""
    V, L = 5120, 2
    case, P, feats = lstm_problem(rows, L, V, "bf16", part=False)
    with det_mode(E, True):
        eng, run = lstm_runner(E, dev, case, P, feats, ids_only=True)
        make = functools.lru_cache(maxsize=None)(lambda s: on(R.rollout_us(s, L, rows, V), dev))
        line = same_route(E, run, make(SEEDS[0]), SEEDS[0], f"gumbelmax rows={rows}")
        assert line.startswith("tile8<f32,128,3,") == (rows >= 385), line        # (3: EPI_GUMBELMAX)
        twin(run, make, dev, f"gumbelmax rows={rows}")


# ---------------------------------------------------------------------------------------------------------------- attention decoder
@functools.lru_cache(maxsize=None)
def attn_problem(family, B, L, V, dtype, N=0):
    case = A.Case("noise", family, B, L, V, 8, 16, 24, 9, 16, dtype, N=N, states=False)       # E, H, C, P, A of its base case
    return case, A.data(case)


def attn_engine(E, case):
    return E.AttnDecoderEngine(case.V, case.E, case.H, case.C, case.P, case.A, DT[case.dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [68, 260])
@pytest.mark.parametrize("B", [1, 17, 65])
@stops_on_fault
def test_attn_fused_rollout(E, dev, B, V, dtype):
    """The attention decoder's roll-out on the same step kernels (vocab_step, stream t), value seed and every gic_step_scalars slot."""
    case, (P, X) = attn_problem("train", B, 3, V, dtype)
    eng = attn_engine(E, case)
    params, feats, fmap = [p.to(dev) for p in P], X["features"].to(dev), X["fmap"].to(dev)

    def runner(scal=None, slot=0):
        def run(seed=0, noise=None):
            st = zeroed(eng.alloc_state(B, case.L, dev))
            out = torch.zeros(B, case.L, V, device=dev, dtype=TD[dtype])
            ids = torch.full((B, case.L), -7, device=dev, dtype=torch.int64)
            eng.sample_fwd(params, feats, fmap, case.L, X["T"], False, noise_u=noise, seed=seed, state=st, out=out, ids=ids,
                           dev_scalars=scal, seed_slot=slot)
            torch.cuda.synchronize()
            return {"ids": ids, "out": out, "state": st}
        return run

    what = f"attention fused roll-out B={B} V={V} {dtype}"
    res = twin(runner(), lambda s: on(R.rollout_us(s, case.L, B, V), dev), dev, what)
    scal = E.StepScalarsBuffer(dev)
    scal.set(X["T"], SLOT_SEEDS)
    want = {s: r for s, r in zip(SEEDS, res)}
    for slot, s in enumerate(SLOT_SEEDS):
        if s not in want:
            want[s] = runner()(noise=on(R.rollout_us(s, case.L, B, V), dev))
        same_bits(runner(scal, slot)(seed=SLOT_SEEDS[(slot + 1) % 4]), want[s], f"{what}: the seed of slot {slot}")


@pytest.mark.parametrize("B,N", [(1, 193), (3, 64)], ids=["386-rows", "384-rows"])
@stops_on_fault
def test_attn_rollout(E, dev, B, N):
    """gic_attn_rollout, bf16, V = 5120, L = 3: step t runs t N B rows.  386 rows: step 1 (193 rows) takes the plain product and the
    register kernel, step 2 (386 >= 385) the product with the Gumbel-max epilogue -- its logits scratch holds 384 rows, so it cannot
    have run otherwise; 384 rows: both steps the separate launches.  One host map for all of them."""
    L, V = 3, 5120
    case, (P, X) = attn_problem("rollout", B, L, V, "bf16", N=N)
    rows = case.rows
    assert A.gumbelmax_from(case) == 385 and rows == 2 * N * B
    eng = attn_engine(E, case)
    lay, total = A.rollout_layout(case)
    assert eng.rollout_ws_bytes(B, L, rows) == total and lay["logits"][1] == min(rows, 384) * V * 4
    params, feats, fmap, Y = [p.to(dev) for p in P], X["features"].to(dev), X["fmap"].to(dev), X["Y"].to(dev)
    saved = eng.forward_tf(params, feats, fmap, Y[:, :-1], [L] * B, 1.0, pretrain=True, keep_state=True)[3]

    def run(seed=0, noise=None):
        ws = torch.zeros(total + 256, device=dev, dtype=torch.uint8)          # (zeroed: a route-only pass skips the products that fill it)
        off = (-ws.data_ptr()) % 256
        ids = eng.rollout(params, saved, Y, N, noise_u=noise, seed=seed, ws=ws[off:off + total])
        torch.cuda.synchronize()
        return {"ids": ids}

    make = functools.lru_cache(maxsize=None)(lambda s: on(R.rollout_us(s, L, rows, V), dev))
    line = same_route(E, run, make(SEEDS[0]), SEEDS[0], f"attention roll-out of {rows} rows")
    assert line.startswith("tile8<f32,128,3,") == (rows >= 385), line        # the last step's vocabulary product (3: EPI_GUMBELMAX)
    twin(run, make, dev, f"attention roll-out of {rows} rows")


# ---------------------------------------------------------------------------------------------------------------- teacher forcing
TF_LENGTHS = (4, 2, 3)
SS_LENGTHS = (4, 2, 3, 4, 1)


@functools.lru_cache(maxsize=None)
def seq_problem(kind, B, T, V, lengths, scale=SC.SCALE):
    extra = dict(C=24, P=9, A=16) if kind == "attn" else {}
    return SC.make(kind, B, T, V, 8, 16, list(lengths), seed=97 + V, scale=scale, **extra)


def seq_engine(E, pr, dtype):
    d = pr["dims"]
    if pr["kind"] == "lstm":
        return E.DecoderEngine(d["V"], d["E"], d["H"], d["NL"], DT[dtype])
    return E.AttnDecoderEngine(d["V"], d["E"], d["H"], d["C"], d["P"], d["A"], DT[dtype])


def maps_of(pr, dev):
    return (pr["fmap"].to(dev),) if pr["kind"] == "attn" else ()


SEQ_CASES = [("lstm", 12), ("lstm", 70), ("attn", 12), ("attn", 68)]       # (the attention decoder takes V % 4 == 0 only: 68 for 70)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,V", SEQ_CASES)
@stops_on_fault
def test_teacher_forced_with_noise(E, dev, kind, V, dtype):
    """forward_tf with pretrain = 0: ONE gumbel_softmax_argmax_kernel launch over the B Tmax rows b Tmax + t, stream 0x7466; ragged
    lengths; V = 70 (LSTM decoder): a counter's lanes straddle rows."""
    B, T = 3, 4
    pr = seq_problem(kind, B, T, V, TF_LENGTHS)
    with det_mode(E, dtype == "bf16" and kind == "lstm"):
        eng = seq_engine(E, pr, dtype)
        params, feats, caps = [p.to(dev) for p in pr["params"]], pr["feats"].to(dev), pr["caps"].to(dev)

        def run(seed=0, noise=None):
            r = eng.forward_tf(params, feats, *maps_of(pr, dev), caps, list(TF_LENGTHS), 0.75, pretrain=False, noise_u=noise, seed=seed)
            torch.cuda.synchronize()
            return {"pred": r[0], "h_n c_n": r[1], "rest": r[2:]}

        assert max(TF_LENGTHS) == T
        make = lambda s: on(R.tf_u(s, B, T, V), dev)
        same_route(E, run, make(SEEDS[0]), SEEDS[0], f"teacher-forced {kind} V={V} {dtype}")
        twin(run, make, dev, f"teacher-forced {kind} V={V} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,V", SEQ_CASES)
@stops_on_fault
def test_scheduled_sampling(E, dev, kind, V, dtype):
    """forward_scheduled at sample_prob = 0.5.  First the coin alone (pick = argmax draws no noise): `replaced` is the host's
    coin < prob at the positions a caption reaches.  Then coin and noise together (V = 12: the vector form; V = 70: the scalar form),
    everything the call returns: pred, the final states, the alphas, `inputs`, `replaced`.  (Attention: V = 68, the vector form again.)"""
    B, T, p = 5, 4, 0.5
    pr = seq_problem(kind, B, T, V, SS_LENGTHS)
    eng = seq_engine(E, pr, dtype)
    params, feats, caps = [p_.to(dev) for p_ in pr["params"]], pr["feats"].to(dev), pr["caps"].to(dev)

    def runner(pick):
        def run(seed=0, noise=None):
            coin, u = noise if noise is not None else (None, None)
            r = eng.forward_scheduled(params, feats, *maps_of(pr, dev), caps, list(SS_LENGTHS), p, pick, coin, u, seed)
            torch.cuda.synchronize()
            head, (inputs, replaced) = r[:-3], r[-2:]                      # (pred, (h_n, c_n)[, alphas]), saved, inputs, replaced
            return {"head": head, "inputs": inputs, "replaced": replaced}
        return run

    reach = torch.arange(1, T)[None, :] < torch.tensor(SS_LENGTHS)[:, None]
    for s in SEEDS:
        coin = R.ss_coin(s, B, T - 1)
        got = runner("argmax")(seed=s)["replaced"].cpu()
        assert torch.equal(got.bool(), torch.from_numpy(coin < np.float32(p)) & reach), f"coins of seed {s:#x}"
    what = f"scheduled sampling {kind} V={V} {dtype}"
    same_route(E, runner("sample"), (on(R.ss_coin(SEEDS[0], B, T - 1), dev), on(R.ss_noise(SEEDS[0], B, T - 1, V), dev)), SEEDS[0], what)
    twin(runner("argmax"), lambda s: (on(R.ss_coin(s, B, T - 1), dev), None), dev, what + " (coin alone)")
    res = twin(runner("sample"), lambda s: (on(R.ss_coin(s, B, T - 1), dev), on(R.ss_noise(s, B, T - 1, V), dev)), dev, what)
    assert all(int(r["replaced"].sum()) >= 2 for r in res), "too few replaced positions to exercise the noise"


# ---------------------------------------------------------------------------------------------------------------- the sampler
STREAM_ID = 0xFEDCBA9876543210
V_STREAMED = 8 * 512 * 4 + 3                 # kSelQuads * kSelThreads * 4 register-resident entries, then a tail of 3


@pytest.mark.parametrize("opts", [(0, 1.0), (3, 1.0), (0, 0.5)], ids=["plain", "k3", "p05"])
@pytest.mark.parametrize("V", [2, 7, 70, V_STREAMED])
@pytest.mark.parametrize("rows", [1, 5])
@stops_on_fault
def test_sample_logits(E, dev, rows, V, opts):
    """gic_sample_logits: counter r ceil(V / 4) + q, lane e, the caller's stream_id with its high bits set.  ids, logp, kept."""
    top_k, top_p = min(opts[0], V), opts[1]
    logits = (3.0 * torch.randn(rows, V, generator=torch.Generator().manual_seed(rows + V))).to(dev)

    def run(seed=0, noise=None):
        r = E.sample_logits(logits, top_k, top_p, 0.9, noise_u=noise, seed=seed, stream_id=STREAM_ID)
        torch.cuda.synchronize()
        return {"ids": r[0], "logp": r[1], "kept": r[2]}

    what = f"sample_logits rows={rows} V={V} k={top_k} p={top_p}"
    for s in SEEDS:
        noise = on(R.sample_u(s, STREAM_ID, rows, V), dev)
        a = run(noise=noise)
        same_bits(run(noise=noise), a, what + ": two explicit launches")
        same_bits(run(seed=s), a, f"{what}, seed {s:#x}: device-drawn launch vs the host's uniforms")


@stops_on_fault
def test_sample_logits_seeds_differ(E, dev):
    """(One row of two entries can draw the same token under both seeds; 64 rows of 70 cannot.)"""
    logits = torch.zeros(64, 70, device=dev)
    a, b = (E.sample_logits(logits, seed=s, stream_id=STREAM_ID)[0] for s in SEEDS)
    want = [on(R.sample_u(s, STREAM_ID, 64, 70), dev) for s in SEEDS]
    assert not torch.equal(a, b)
    for ids, u in zip((a, b), want):
        assert torch.equal(ids, E.sample_logits(logits, noise_u=u)[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cons", [False, True], ids=["free", "constrained"])
@pytest.mark.parametrize("kind", ["lstm", "attn"])
@stops_on_fault
def test_sample_captions(E, dev, kind, cons, dtype):
    """sample_captions / constrained_sample_captions (the BAN instantiation of the selection kernel): stream t, six rows, V = 70 -- the
    sampler's own map, which is not the roll-out's at V % 4 != 0 (68 for the attention decoder).  ids, scores, lengths."""
    B, n, L, V = 2, 3, 4, 70 if kind == "lstm" else 68
    pr = seq_problem(kind, B, L + 1, V, (L + 1,) * B, scale=3.0)
    kw = dict(no_repeat_ngram=2, min_length=2, suppress_tokens=(5, 9)) if cons else {}
    with det_mode(E, dtype == "bf16" and kind == "lstm"):
        eng = seq_engine(E, pr, dtype)
        params, feats = [p.to(dev) for p in pr["params"]], pr["feats"].to(dev)

        nbytes = eng.sample_ws_bytes(B, L, n)

        def run(seed=0, noise=None):
            ws = torch.zeros(nbytes + 256, device=dev, dtype=torch.uint8)     # (zeroed: a route-only pass skips the products that fill it)
            off = (-ws.data_ptr()) % 256
            r = eng.sample_captions(params, feats, *maps_of(pr, dev), L, n, top_k=20, top_p=0.9, temperature=1.1, seed=seed, noise_u=noise,
                                    ws=ws[off:off + nbytes], **kw)
            torch.cuda.synchronize()
            return {"ids": r[0], "scores": r[1], "lengths": r[2]}

        what = f"sample_captions {kind} {'constrained ' if cons else ''}{dtype}"
        make = lambda s: on(R.sample_us(s, L, B * n, V), dev)
        if kind == "lstm":                     # (V = 70: separate products; the attention decoder's six rows run on the fused step kernels)
            same_route(E, run, make(SEEDS[0]), SEEDS[0], what)
        twin(run, make, dev, what)


# ---------------------------------------------------------------------------------------------------------------- highway dropout
DISC_KEYS = ("emb", "pooled", "argmax", "hpre", "keep", "ydrop", "feat")


@pytest.mark.parametrize("h", HIGHWAY, ids=[h.id for h in HIGHWAY])
@stops_on_fault
def test_highway_dropout(E, dev, h, monkeypatch):
    """highway_keep4 at its three callers -- gemm_kernel's scalar highway epilogue, tile8's wide one, disc_highway_redrop_kernel -- on
    the smallest shape of every highway route: rows off the 4-row quads and the 128-row tiles, F % 8 != 0.  N is F (not Fp) at all
    three.  The written `keep` against the host mask directly; the launch against the explicit-mask launch (hpre, keep, ydrop, feat,
    the logits) for gic_disc_fwd and gic_disc_fwd_redrop; the seed by value and through each of the four gic_step_scalars slots."""
    case = h.case()
    gen = torch.Generator().manual_seed(2024)
    P = DC.make_params(case, "rounding", gen)
    X = DC.make_inputs(case, gen, train=True, mask=False)
    F, MR = case.F, case.MR
    with det_mode(E, case.dtype == "bf16"):
        eng = disc_make_engine(E, case, monkeypatch)
        params, ids = [p.to(dev) for p in P], X["ids"].to(dev)
        scal = E.StepScalarsBuffer(dev)
        scal.set(1.0, SLOT_SEEDS)

        def fwd(seed=0, noise=None, slot=None):
            g = disc_alloc_state(case, dev, hpre_off=h.off // 4)
            st = disc_live(g)
            state = {k: st[k] for k in DISC_KEYS}
            eng.fwd(params, None, ids, True, noise, seed=seed, state=state, logits=st["logits"],
                    dev_scalars=scal if slot is not None else None, seed_slot=slot or 0)
            torch.cuda.synchronize()
            disc_assert_guards(case, g)
            return {**{k: state[k] for k in ("hpre", "keep", "ydrop", "feat")}, "logits": st["logits"]}, state

        def redrop(src, seed=0, noise=None, slot=None):
            g = disc_alloc_state(case, dev)
            st = disc_live(g)
            dst = {k: st[k] for k in ("keep", "ydrop", "feat")}
            eng.fwd_redrop(params, src, dst, True, noise, seed=seed, logits=st["logits"], dev_scalars=scal if slot is not None else None,
                           seed_slot=slot or 0)
            torch.cuda.synchronize()
            disc_assert_guards(case, g)
            return {**dst, "logits": st["logits"]}

        with E.route_only() as r:
            fwd(seed=SEEDS[0])
            line_dev = r.last()
        mask0 = on(R.highway_keep(SEEDS[0], MR, F, DC.DROP_P), dev)
        with E.route_only() as r:
            fwd(noise=mask0)
            line_exp = r.last()
        assert line_dev == line_exp and line_dev.split(" lds=")[0] == h.route, (line_dev, line_exp)

        seen = []
        for slot, s in enumerate(SLOT_SEEDS):
            what = f"{h.id}, seed {s:#x}"
            mask = on(R.highway_keep(s, MR, F, DC.DROP_P), dev)
            a, src = fwd(noise=mask)
            ra = redrop(src, noise=mask)
            assert torch.equal(a["keep"][:, :F], mask) and torch.equal(ra["keep"][:, :F], mask)
            if slot == 0:
                same_bits(fwd(noise=mask)[0], a, f"{what}: two explicit gic_disc_fwd launches")
                same_bits(redrop(src, noise=mask), ra, f"{what}: two explicit gic_disc_fwd_redrop launches")
            wrong = SLOT_SEEDS[(slot + 1) % 4]                      # the value seed of a launch that must read its slot instead
            runs = [("slot %d" % slot, dict(seed=wrong, slot=slot))] + ([("by value", dict(seed=s))] if s in SEEDS else [])
            for name, kw in runs:
                d, dsrc = fwd(**kw)
                assert torch.equal(d["keep"][:, :F], mask), f"{what}, {name}: the keep flags gic_disc_fwd wrote are not the host's"
                same_bits(d, a, f"{what}, {name}: gic_disc_fwd, device-drawn vs the host's mask")
                rd = redrop(dsrc, **kw)
                assert torch.equal(rd["keep"][:, :F], mask), f"{what}, {name}: the keep flags gic_disc_fwd_redrop wrote are not the host's"
                same_bits(rd, ra, f"{what}, {name}: gic_disc_fwd_redrop, device-drawn vs the host's mask")
            seen.append(a)
        assert all(differs(seen[0], x) for x in seen[1:])


# ---------------------------------------------------------------------------------------------------------------- the composed step
def _step_noise(inst, m, dev):
    """The next step's seeds in the order FusedAdvStep takes them (three dropout seeds: D(real), D(fake), D(gen); then the roll-out's)
    and what they draw: (noise_u [L, B, V], the three keep masks [B R, F])."""
    from gan_image_captioning_amd.generator import SEEDS as STREAM
    den = inst.fused.den
    s = [STREAM.next() for _ in range(4)]
    masks = [on(R.highway_keep(s[i], m["B"] * den.R, den.F, den.drop_p), dev) for i in range(3)]
    return on(R.rollout_us(s[3], m["L"], m["B"], m["V"]), dev), masks


def _step_result(inst, out):
    torch.cuda.synchronize()
    return {"losses": out["losses"].clone(), "ids": out["ids"].clone(), "probs": out["probs"].clone(), "logits": out["logits"].clone(),
            "gen grads": inst.gen_arena.grad.clone(), "disc grads": inst.disc_arena.grad.clone()}


def _golden_instructor(dtype, dev):
    g = Golden("cfg1")                  # B = 8, L = 10, V = 64, E = 32, H = 512
    m = dict(g.meta)
    m["B"] = int(g.t("caps").shape[0])
    inst, args = make_instructor(m, "fused", dtype={"f32": "fp32", "bf16": "bf16"}[dtype])
    load_params(inst, *initial_params(g))
    inst.gen.train(); inst.disc.train()
    inst.gen.decoder.temperature = 0.9
    return inst, m, g.t("caps").to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@stops_on_fault
def test_composed_step(E, dev, dtype, monkeypatch):
    """One free-running FusedAdvStep call at the golden cfg1 shapes (deterministic mode: D's weight gradients are f32 atomics
    otherwise) against the same call given the host's noise for the seeds the step took: losses, ids, probabilities, the three D
    logits and both gradient arenas."""
    from gan_image_captioning_amd.generator import SEEDS as STREAM
    monkeypatch.setenv("GIC_NO_STEP_GRAPH", "1")
    with det_mode(E, True):
        inst, m, caps = _golden_instructor(dtype, dev)
        for k in (5, 77):
            STREAM.reset(k)
            dev_run = _step_result(inst, inst.fused(None, caps, m["L"], True, opt_step=False))
            STREAM.reset(k)
            u, masks = _step_noise(inst, m, dev)
            exp = [_step_result(inst, inst.fused(None, caps, m["L"], True, u, masks, opt_step=False)) for _ in range(2)]
            same_bits(exp[0], exp[1], f"composed step {dtype}, SEEDS.reset({k}): two explicit steps")
            same_bits(dev_run, exp[0], f"composed step {dtype}, SEEDS.reset({k}): free-running vs the host's noise")
            if k == 5:                         # (after complete steps: the buffers a route-only pass reads hold a real step's values)
                same_route(E, lambda seed=0, noise=None: inst.fused(None, caps, m["L"], True, *(noise or ()), opt_step=False), (u, masks), 0,
                           f"composed step {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@stops_on_fault
def test_composed_step_through_the_replayed_graphs(E, dev, dtype, monkeypatch):
    """GIC_STEP_GRAPH=1: four training steps (eager, capture, two replays; fresh seeds each, read from gic_step_scalars) by one
    instructor, the same four steps with the host's noise by a second one from the same weights.  Every step equals its explicit twin,
    and so do the weights both end with: what a free-running step computes and what the oracle pins are the same computation.  bf16:
    the refresh of the compute-dtype weight images is part of every replay."""
    from gan_image_captioning_amd.generator import SEEDS as STREAM
    with det_mode(E, True):
        monkeypatch.setenv("GIC_STEP_GRAPH", "1")
        monkeypatch.delenv("GIC_NO_STEP_GRAPH", raising=False)
        graph, m, caps = _golden_instructor(dtype, dev)
        assert graph.fused.use_graph
        monkeypatch.setenv("GIC_NO_STEP_GRAPH", "1")
        twin_inst, _, _ = _golden_instructor(dtype, dev)
        assert not twin_inst.fused.use_graph
        for step in range(4):
            STREAM.reset(100 + 10 * step)
            got = _step_result(graph, graph.fused(None, caps, m["L"], True))
            STREAM.reset(100 + 10 * step)
            u, masks = _step_noise(twin_inst, m, dev)
            want = _step_result(twin_inst, twin_inst.fused(None, caps, m["L"], True, u, masks))
            same_bits(got, want, f"replayed step {step} {dtype}")
            same_bits({"gen": graph.gen_arena.flat, "disc": graph.disc_arena.flat}, {"gen": twin_inst.gen_arena.flat, "disc": twin_inst.disc_arena.flat},
                      f"weights after step {step} {dtype}")
        assert len(graph.fused._graphs) == 1 and len(next(iter(graph.fused._graphs.values()))["graphs"]) == 6, "the step was not captured"
