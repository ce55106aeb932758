"""The decode heads' workspace contract without a GPU (tests/decode_ws.py, tests/decode_ws_cases.py): the layout replica against the
eleven host-only ``gic_*_ws_bytes`` queries, the typed poison's legality, the case matrix (every f32 case decidable by the float64
oracle alone, every search ending as its termination says), and the checker against the failures this family can have -- pure-torch
fake heads that write into a band, leave an element of ids unwritten, modify an input, read ``count`` before writing it or return a
token past ``lengths`` that is not <PAD>."""
import ctypes as C
import re
import types

import pytest
import torch

from tests import decode_ws as W
from tests import decode_ws_cases as WC
from tests.decode_ws import Dims

# ---------------------------------------------------------------- 1. the replica against the queries
LSTM_GRID = [(3, 6, 68, 8, 16, 1), (3, 6, 68, 8, 16, 2), (3, 6, 50, 8, 16, 2), (1, 6, 68, 8, 16, 1), (65, 6, 68, 8, 16, 1)]
ATTN_GRID = [(3, 5, 52, 8, 16, 24, 9, 16), (1, 5, 52, 8, 16, 24, 9, 16)]
UPDATE = ("the workspace layout of csrc/decode.hip and its replica disagree: if the layout changed on purpose, update {fn} in "
          "tests/decode_ws.py (and the header comment of decode.hip); if not, the query is wrong")


def _engine(d: Dims, dt):
    from gan_image_captioning_amd import engine
    if d.attn:
        return engine.AttnDecoderEngine(d.V, d.E, d.H, d.C, d.P, d.A, dt)
    return engine.DecoderEngine(d.V, d.E, d.H, d.NL, dt)


def _dims(shape):
    return Dims(*shape) if len(shape) == 6 else Dims(*shape[:5], 1, *shape[5:])


def _fused_rows(eng, d):
    return 0 if d.attn else eng.fused_rollout_rows()


@pytest.mark.parametrize("dt", [W.F32, W.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("shape", LSTM_GRID + ATTN_GRID, ids=lambda s: "x".join(map(str, s)))
def test_replica_total_equals_every_query(shape, K, dt):
    d = _dims(shape)
    eng = _engine(d, dt)
    fused_rows = _fused_rows(eng, d)
    if not d.attn:
        assert fused_rows == (512 if d.V % 4 == 0 else 0), fused_rows          # V = 68 qualifies, V = 50 does not
    fused = W.is_fused(d, K, fused_rows)
    assert fused == (d.attn or (d.V == 68 and d.B * K <= 512))                   # (65, 8): the generic path by row count alone
    rows = lambda r: "\n" + W.region_table(r)          # noqa: E731
    r, total = W.decode_regions(d, K, dt, True, fused)
    assert total == eng.beam_ws_bytes(d.B, d.L, K), UPDATE.format(fn="decode_regions (beam)") + rows(r)
    r, total = W.decode_regions(d, K, dt, False, fused)
    assert total == eng.sample_ws_bytes(d.B, d.L, K), UPDATE.format(fn="decode_regions (sampler)") + rows(r)
    r, total = W.forced_regions(d, K, dt, fused)
    assert total == eng.forced_beam_ws_bytes(d.B, d.L, K), UPDATE.format(fn="forced_regions") + rows(r)
    for M in (1, 2, 4):
        r, total = W.ensemble_regions(d, K, dt, True, fused, M)
        assert total == eng.ensemble_beam_ws_bytes(d.B, d.L, M, K), UPDATE.format(fn=f"ensemble_regions (beam, M = {M})") + rows(r)
        r, total = W.ensemble_regions(d, K, dt, False, fused, M)
        assert total == eng.ensemble_sample_ws_bytes(d.B, d.L, M, K), UPDATE.format(fn=f"ensemble_regions (sampler, M = {M})") + rows(r)


@pytest.mark.parametrize("S", [0, 3, 16])
@pytest.mark.parametrize("rows,L", [(12, 6), (12, 5), (1, 6), (520, 6)])
def test_replica_total_equals_the_constraints_query(rows, L, S):
    from gan_image_captioning_amd import _lib as lib
    c = lib.DecodeConstraints()
    c.num_suppress = S
    out = C.c_uint64(0)
    lib.check(lib.load().gic_decode_constraints_ws_bytes(rows, L, C.byref(c), C.byref(out)), "gic_decode_constraints_ws_bytes")
    r, total = W.constraints_regions(rows, L, S)
    assert total == int(out.value), UPDATE.format(fn="constraints_regions") + "\n" + W.region_table(r)


def test_regions_are_aligned_disjoint_and_in_the_documented_order():
    d = Dims(3, 5, 52, 8, 16, 1, 24, 9, 16)
    r, total = W.forced_regions(d, 4, W.BF16, True)
    assert [x.name for x in r] == ["xh0", "c0", "fproj", "hp", "e", "ahist", "pm", "ps", "pv", "pi", "score", "fin", "len", "tok", "par",
                                   "htok", "hpar", "anc", "last", "done", "count", "hop_id", "hop_tgt", "hop_val", "init", "cws0.nban",
                                   "cws0.ban", "cws0.hist"]
    at = 0
    for x in r:
        assert x.offset % W.ALIGN == 0 and x.offset >= at, x
        at = x.offset + x.nbytes
    assert at <= total
    r, _ = W.ensemble_regions(Dims(3, 6, 50, 8, 16, 2), 4, W.F32, True, False, 2)
    assert [x.name for x in r] == ["xh0", "c0", "xh1", "c1", "gpre", "logits", "pm", "ps", "pv", "pi", "score", "fin", "len", "tok", "par",
                                   "htok", "hpar", "last", "done", "count", "slabs", "m1.xh0", "m1.c0", "m1.xh1", "m1.c1", "m1.gpre"]
    r, _ = W.decode_regions(Dims(3, 6, 68, 8, 16, 1), 4, W.F32, False, True)
    assert [x.name for x in r] == ["xh0", "c0", "logits", "score", "fin", "len", "tok", "par", "htok", "last", "done", "count"]


# ---------------------------------------------------------------- 2. the poison
def case_layouts(case, dt, fused_rows):
    """([regions, total] of the case's workspace, of its constraint workspace or None)."""
    d, K = WC.MODELS[case.model]
    h = WC.HEADS[case.head]
    fused = W.is_fused(d, K, fused_rows)
    if h.kind == "forced":
        main = W.forced_regions(d, K, dt, fused)
    elif h.kind.startswith("ens"):
        main = W.ensemble_regions(d, K, dt, h.kind == "ens-beam", fused, WC.M_ENS)
    else:
        main = W.decode_regions(d, K, dt, h.kind == "beam", fused)
    S = len(h.cons["suppress_tokens"])
    return main, (W.constraints_regions(d.B * K, d.L, S) if h.cons is not WC.C_OFF else None)


def case_poison(case, dt, fused_rows):
    """``poison(i, live)`` of the case for decode_ws.run_priors."""
    d, K = WC.MODELS[case.model]
    S = len(WC.HEADS[case.head].cons["suppress_tokens"])
    lay = case_layouts(case, dt, fused_rows)

    def poison(i, live):
        regions, total = lay[i]
        assert total == live.numel(), f"{case.id}: workspace request {i} holds {live.numel()} bytes, the replica's layout {total}"
        s = S if i == 1 else 0
        W.write_poison(live, regions, dt, W.poison_ints(d, K, WC.EOS, s), W.int_ranges(d, K, s, 2))
    return poison


@pytest.mark.parametrize("dt", [W.F32, W.BF16], ids=["f32", "bf16"])
def test_poison_is_typed_and_legal_in_every_case(dt):
    """Every integer region of every case receives a value inside its legal index range (write_poison asserts it), every float region
    NaN in its own type, and nothing else is written."""
    seen = set()
    for case in WC.CASES:
        if (case.model, case.head) in seen:
            continue
        seen.add((case.model, case.head))
        d, K = WC.MODELS[case.model]
        fused_rows = _fused_rows(_engine(d, dt), d)
        poison = case_poison(case, dt, fused_rows)
        for i, lay in enumerate(case_layouts(case, dt, fused_rows)):
            if lay is None:
                continue
            regions, total = lay
            live = torch.full((total,), 0x5A, dtype=torch.uint8)
            poison(i, live)
            S = len(WC.HEADS[case.head].cons["suppress_tokens"]) if i == 1 else 0
            ranges = W.int_ranges(d, K, S, 2)
            covered = torch.zeros(total, dtype=torch.bool)
            for r in regions:
                v = W.region_view(live, r, dt)
                covered[r.offset:r.offset + r.nbytes] = True
                if r.kind == "i32":
                    lo, hi = ranges[r.role]
                    assert int(v.min()) >= lo and int(v.max()) <= hi and int(v.min()) == int(v.max()), (case.id, r.name)
                else:
                    assert bool(torch.isnan(v).all()), (case.id, r.name)
            assert bool((live[~covered] == 0).all()), case.id
    ints = W.poison_ints(Dims(3, 6, 68, 8, 16, 1), 4, WC.EOS, 2)
    assert (ints["fin"], ints["done"], ints["count"], ints["len"], ints["tok"], ints["pi"], ints["nban"]) == (1, 1, 12, 6, WC.EOS, 67, 9)


# ---------------------------------------------------------------- 3. the case matrix
def test_matrix_holds_every_listed_combination():
    ids = {c.id for c in WC.CASES}
    assert len(ids) == len(WC.CASES)
    for model in ("lstm1", "lstm2", "generic", "attn"):
        for head in WC.HEADS:
            if head in WC.ATTN_ONLY and model != "attn":
                continue
            for term in ("ends", "runs"):
                assert f"{model}-{head}-{term}" in ids
    for model in ("lstm1-b1k1", "attn-b1k1", "rows520"):
        assert {f"{model}-{h}-{t}" for h in WC.SMALL for t in ("ends", "runs")} <= ids
    assert WC.MODELS["rows520"][0].B * WC.MODELS["rows520"][1] == 520 and WC.MODELS["lstm1"][0].B * WC.MODELS["lstm1"][1] == 12
    h = WC.HEADS
    assert h["diverse"].groups == 2 and h["diverse"].diversity == 1.0 and h["beam-lp0.7"].lp == 0.7
    assert h["cbeam"].cons == dict(no_repeat_ngram=2, min_length=3, suppress_tokens=(1, 3)) and h["forced-cons"].cons is WC.CONS
    assert {h["ens-beam"].mode, h["ens-sample"].mode} == {"prob", "logprob"}
    f = WC.force_words(WC.MODELS["lstm1"][0])
    assert tuple(f.shape) == (3, 2, 2) and int(f.max()) == 67 and not set(f.flatten().tolist()) & {0, 1, 2, 3}


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_oracle_decides_every_case(case):
    """The GPU test compares EVERY image (row) of a case with the oracle: the oracle alone decides each selection by >= 1e-4 (each
    draw and nucleus by > 1e-5), and the <E> bias ends the search as the case's termination says."""
    want = WC.oracle(case)
    assert WC.decided(case, want) == "", f"{case.id} (seed {WC.seed_of(case)})"


# ---------------------------------------------------------------- 4. the checker flags the failures this family can have
D, K = Dims(3, 6, 68, 8, 16, 1), 4
REGIONS, NBYTES = W.decode_regions(D, K, W.F32, True, True)
BY_NAME = {r.name: r for r in REGIONS}
CPU = torch.device("cpu")


def fake_head(ns, feats, shift, fault=None):
    """A pure-torch 'beam search' through the module's allocation helpers: a deterministic function of the features that initialises
    its state words first -- unless a fault is seeded."""
    ws = ns._aligned_ws(None, NBYTES, CPU)
    ids, scores, lengths = ns._decode_outputs(D.B, K, D.L, CPU)
    count = W.region_view(ws, BY_NAME["count"], W.F32)
    stale = int(count[0]) if fault == "reads_count" else 0          # the fault: the step loop's early exit reads count before init
    count.zero_()
    W.region_view(ws, BY_NAME["fin"], W.F32).zero_()
    if fault == "band":
        ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel()).fill_(0)
    if fault == "input":
        feats[0, 0] += 1.0
    base = int(feats.sum().abs() * 100) + shift
    for b in range(D.B):
        for k in range(K):
            n = 1 if stale >= D.B else D.L - (b + k) % 3           # the search "was over" at step 0
            for t in range(D.L):
                if fault == "unwritten" and (b, k, t) == (1, 2, 3):
                    continue
                ids[b, k, t] = WC.PAD if t >= n else WC.EOS if (t == n - 1 and n < D.L) else 4 + (base + b + 3 * k + t) % (D.V - 4)
            lengths[b, k] = n
            scores[b, k] = -0.5 * n - k
    if fault == "pad":
        ids[2, 2, D.L - 1] = 5                                      # lengths[2, 2] = 5 < L
    count.fill_(D.B)
    W.region_view(ws, BY_NAME["fin"], W.F32).fill_(1)


def _run_fake(fault):
    ns = types.SimpleNamespace(_aligned_ws=None, _decode_outputs=None, torch=torch)
    h = W.Harness(ns, CPU, W.OutSpec(D.V, D.L, WC.PAD))
    feats = h.put("features", torch.arange(D.B * D.E, dtype=torch.float32).reshape(D.B, D.E) / 7)
    other = torch.ones(D.B, D.E)

    def poison(i, live):
        W.write_poison(live, REGIONS, W.F32, W.poison_ints(D, K, WC.EOS, 0), W.int_ranges(D, K, 0, 2))
    return W.run_priors(h, "fake", lambda: fake_head(ns, feats, 0, fault), lambda: fake_head(ns, other, 11), poison)


def test_checker_passes_a_healthy_head():
    out = _run_fake(None)
    assert set(out) == {"ids", "scores", "lengths"} and int(out["lengths"].min()) == 4


@pytest.mark.parametrize("fault,msg", [
    ("band", "fake [on zeros]: a write outside the workspace: byte 0 above it holds 0x0"),
    ("unwritten", "fake [on zeros]: 1 elements of ids were never written, the first at [1, 2, 3]"),
    ("input", "fake [on zeros]: the call changed its input features"),
    ("reads_count", "fake: the run on a workspace holding finished twin differs from the run on zeros in ids"),
    ("pad", "fake [on zeros]: ids past a caption's length must be <PAD> (0): [5]"),
])
def test_checker_flags_the_fault(fault, msg):
    with pytest.raises(AssertionError, match=re.escape(msg)):
        _run_fake(fault)


def test_checker_flags_a_stale_count_under_poison_alone():
    """Without a twin search before it, the typed poison alone (count = rows) exposes the premature read."""
    ns = types.SimpleNamespace(_aligned_ws=None, _decode_outputs=None, torch=torch)
    h = W.Harness(ns, CPU, W.OutSpec(D.V, D.L, WC.PAD))
    feats = torch.ones(D.B, D.E)
    with h.call(lambda i, live: live.zero_()):
        fake_head(ns, feats, 0, "reads_count")
    first = h.check("fake")
    with h.call(lambda i, live: W.write_poison(live, REGIONS, W.F32, W.poison_ints(D, K, WC.EOS, 0), W.int_ranges(D, K, 0, 2))):
        fake_head(ns, feats, 0, "reads_count")
    with pytest.raises(AssertionError, match="holding typed poison differs from the run on zeros in ids"):
        W.same_bits("fake", W.POISON, h.check("fake"), first)


def test_banded_buffers_are_aligned_and_banded():
    b = W.Banded(1000, CPU, "x")
    assert b.live.data_ptr() % 256 == 0 and b.live.numel() == 1000 and b.lo >= W.BAND and b.breach() is None
    b.flat[b.lo - 1] = 0
    assert b.breach() == ("below", 1, 0)


def test_aligned_ws_keeps_a_fitting_caller_buffer():
    """The reuse that ``ws=`` documents: a caller's buffer that is large enough and 256-byte aligned is the one the head runs in;
    a short or misaligned one is replaced by a fresh aligned buffer of the size asked for."""
    from gan_image_captioning_amd import engine
    b = W.Banded(4096, CPU, "ws")
    assert engine._aligned_ws(b.live, 4096, CPU).data_ptr() == b.live.data_ptr()
    assert engine._aligned_ws(b.live, 1024, CPU).data_ptr() == b.live.data_ptr()
    for bad in (b.live[:1000], b.live[8:], None):
        got = engine._aligned_ws(bad, 4096, CPU)
        assert got.numel() == 4096 and got.data_ptr() % 256 == 0 and not (b.live.data_ptr() <= got.data_ptr() < b.live.data_ptr() + 4096)
