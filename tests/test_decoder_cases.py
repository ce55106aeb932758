"""The decoder case table (tests/decoder_cases.py) without a GPU: every case names the routes and kernels gic_decoder_sample_fwd /
_bwd select for it (a pure restatement of their conditions, so a changed threshold has to move the table deliberately), the table
reaches every route, kernel and chunk / pass count the decoder has, the references alone leave at most 1 % of a case's rows without
a clear argmax margin, the scattered tokens repeat, and the checker flags the failures this kernel family can have, each at the stage
it belongs to and nowhere upstream."""
import pytest
import torch

from tests import decoder_cases as D
from tests.decoder_cases import CASES, ORDER
from tests.gpu_util import SENTINEL, Guarded

BY = {c.id: c for c in CASES}


def test_ids_are_unique():
    assert len(BY) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_names_the_route_the_selection_takes(case):
    assert D.route_str(D.select(case)) == case.route


def test_plans_of_the_shapes_the_issue_names():
    assert D.lstm_plan("f32", 8, 512, True) == (2, 2, True) and D.lstm_plan("f32", 520, 8, True) == (2, 2, True)      # ldx = 520: 512 + 8
    assert D.lstm_plan("bf16", 8, 1024, True) == (2, 2, True) and D.lstm_plan("bf16", 520, 512, True) == (2, 2, True)  # ldx = 1032: 1024 + 8
    assert D.lstm_plan("bf16", 512, 512, False) == (1, 2, False)                                                       # two passes, one chunk
    assert D.lstm_plan("bf16", 512, 512, True) == (1, 1, True)                                                         # the bench shape
    assert D.lstm_plan("f32", 8, 16, True) == (1, 1, True)
    # the second pass starts past 4096 pieces: kc > 256 in f32, > 512 in bf16
    assert D.lstm_plan("f32", 128, 128, False)[1] == 1 and D.lstm_plan("f32", 128, 136, False)[1] == 2
    assert D.lstm_plan("bf16", 256, 256, False)[1] == 1 and D.lstm_plan("bf16", 256, 264, False)[1] == 2


def test_table_reaches_every_route_kernel_and_chunk_count():
    for dtype in ("f32", "bf16"):
        S = [D.select(c) for c in CASES if c.dtype == dtype]
        assert {s["fwd"] for s in S} == {"fused", "generic"} and {s["bwd"] for s in S} == {"fused", "generic"}
        assert {s["argmax"] for s in S} == {None, "reg1", "reg4", "scalar"}
        assert {s["softmax_bwd"] for s in S} == ({None, "vec8", "scalar"} if dtype == "f32" else {None, "vec5", "vec8", "scalar"})
        layers = [p for s in S if s["lstm"] for p in s["lstm"]]
        assert {p[0] for p in layers} >= {1, 2} and {p[1] for p in layers} == {1, 2} and {p[2] for p in layers} == {None, 1, 2}
        assert {p[3] for p in layers} == {True, False}
        assert {s["vocab"] for s in S if s["vocab"]} >= {1, 2}
    # the bench shape's gathering steps stay in one pass; its step 0 and the whole of layer 1 (ldx = 1024) take the second without a second chunk
    assert D.select(BY["e512-h512-nl2-bf16"])["lstm"] == [(1, 2, 1, True), (1, 2, None, False)]
    assert BY["v16452-f32"].nblk == 258 and BY["tails-f32"].V % 64 == 4 and BY["tails-f32"].B % 64 == 1 and BY["tails-f32"].ldx(0) == 24
    assert BY["h512-f32"].H // 4 == 128 and BY["tiny3-f32"].NL == 3
    for flag, n in (("pretrain", 2), ("states", 1), ("force", 2), ("det", 3)):
        for dtype in ("f32", "bf16"):
            assert sum(1 for c in CASES if getattr(c, flag) and c.dtype == dtype) == n, flag
    assert {c.part for c in CASES if c.pretrain} == {True, False} == {c.part for c in CASES if c.force}


def fill(case, P=None, X=None, mut=None, exact=False, near=None):
    """A correct result in storage precision (the references themselves, cast), optionally mutated."""
    if P is None:
        P, X = D.data(case)
    img = D.images(case, P)
    st, ws, grads = D.new_state(case), D.new_ws(case), D.new_grads(case, P)
    D.run_forward(case, P, img, X, st, None, mut=mut, exact=exact, near=near)
    D.run_backward(case, P, img, X, st, ws, grads, None, mut=mut)
    return P, X, img, st, ws, grads


def check(case, P, X, img, st, ws, grads, exact=False):
    rep = D.Report()
    D.check_images(case, P, img, rep)
    D.run_forward(case, P, img, X, st, rep, exact=exact)
    D.run_backward(case, P, img, X, st, ws, grads, rep, det=True)
    return rep


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_alone_has_clear_margins_and_repeated_tokens(case):
    """At most 1 % of a case's (step, caption) rows lack an fp64 margin of twice the bound between their two largest y; where more
    tokens are scattered into d_embed than the vocabulary has, some repeat."""
    near = []
    st = D.new_state(case)
    P, X = D.data(case)
    D.run_forward(case, P, D.images(case, P), X, st, None, near=near)
    unclear, rows = near[0]
    assert unclear <= 0.01 * rows, (unclear, rows)
    if case.B * (case.L - 1) > case.V or case.det:
        assert D.repeats(st["ids"], case.L) > 0


@pytest.mark.parametrize("cid", ["tiny3-f32", "tails-f32", "tails-bf16", "tails-generic-bf16", "forced-f32", "forced-generic-bf16", "states-bf16",
                                 "b516-f32", "b516-bf16", "pretrain-f32", "pretrain-generic-bf16", "v12-bf16", "h264-f32"])
def test_checker_passes_a_correct_result(cid):
    case = BY[cid]
    rep = check(case, *fill(case))
    assert not rep.failed, rep.failed
    want = set(ORDER) - ({"wout"} if case.dtype == "f32" else set())
    if D.select(case)["fwd"] != "fused":
        want -= {"part_m", "part_s", "key"}
    if case.pretrain:
        want -= {"dlogits"}
    if case.L < 2:
        want -= {"xrows"}
    assert want <= set(rep.ratio), want - set(rep.ratio)


def test_checker_passes_the_tie_regime_and_flags_a_later_index():
    for (dtype, part), case in D.TIES.items():
        for pair in D.TIE_PAIRS:
            gen = torch.Generator().manual_seed(D.SEED)
            P, X = D.tie_params(case, gen, pair), D.make_inputs(case, gen)
            good = fill(case, P, X, exact=True)
            assert (good[3]["ids"] == pair[0]).all()
            assert not check(case, *good, exact=True).failed
            rep = check(case, *fill(case, P, X, mut="tie_later", exact=True), exact=True)
            assert min(ORDER.index(s) for s in rep.failed) == ORDER.index("key" if part else "ids"), rep.failed


def _d_b_differs(P, X, img, st, ws, grads):
    grads[3][5] += 1e-3 * (1 + grads[3][5].abs())


@pytest.mark.parametrize("cid,mut,stage", [
    ("tails-f32", "row64_unwritten", "c"),                  # 1. row 64 of a B = 65 buffer left at its pre-fill
    ("tails-bf16", "k_tail_missing", "gates"),              # 2. the last 8 columns of K missing from a gate product
    ("tails-f32", "seam_swapped", "gates"),                 # 3. the pieces either side of the x|h seam exchanged
    ("tails-bf16", "h_up_ulp", "h copies"),                 # 4. h_up one bf16 ulp off h
    ("tails-bf16", "truncate", "h"),                        # 5. bf16 results truncated instead of rounded
    ("tails-f32", "quad_no_bias", "part_m"),                # 6. the one quad of the partial tile without its bias
    ("tails-bf16", "part_s_subtile", "part_s"),             # 7. part_s missing one 16-entry sub-tile
    ("tails-f32", "out_neighbour_scale", "out"),            # 8. a tile of out scaled with its neighbour's scale
    ("tails-bf16", "no_upper_term", "dgates"),              # 10. dgates without the upper layer's term
    ("tails-f32", "dc_no_f", "dgates"),                     # 11. the dc carry not multiplied by f
    ("tails-f32", "embed_once", "d_embed"),                 # 12. a repeated token counted once in d_embed
    ("tails-f32", _d_b_differs, "d_b_ih"),                  # 13. d_b_ih != d_b_hh
], ids=lambda v: v if isinstance(v, str) else (v.__name__ if callable(v) else ""))
def test_checker_flags_the_failures_this_family_can_have(cid, mut, stage):
    """Each mutation of a correct result is flagged at its own stage and at no stage upstream of it (9., the tie, is above)."""
    case = BY[cid]
    bufs = fill(case, mut=None if callable(mut) else mut)
    if callable(mut):
        mut(*bufs)
    rep = check(case, *bufs)
    assert stage in rep.failed, (rep.failed, rep.ratio)
    assert min(ORDER.index(s) for s in rep.failed) == ORDER.index(stage), rep.failed
    if mut == "quad_no_bias":
        assert {"part_s", "out"} <= set(rep.failed)
    if callable(mut):
        assert "d_b_ih == d_b_hh" in rep.failed


def test_a_touched_guard_row_is_noticed():
    """14. sentinel guard rows either side of a buffer, also behind a misaligned view."""
    for dtype in (torch.float32, torch.bfloat16, torch.uint8, torch.int64):
        for off in (0, 2):
            g = Guarded(5, 3, dtype, "cpu", 0, off=off)
            assert g.guards_intact() and g.live.shape == (5, 3) and float(g.flat[0]) == (0xA5 if dtype == torch.uint8 else SENTINEL)
            g.live.fill_(7)
            assert g.guards_intact()
            g.flat[g.lo + g.live.numel()] = 0
            assert not g.guards_intact()
            g = Guarded(5, 3, dtype, "cpu", 0, off=off)
            g.flat[g.lo - 1] = 0
            assert not g.guards_intact()
