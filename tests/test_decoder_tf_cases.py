"""The teacher-forced decoder case table (tests/decoder_tf_cases.py) without a GPU: every case names the routes the teacher-forced entry
points select for it (a restatement of their conditions) and what the library's own GEMM selection answers for its products (probed in
route-only mode and through gic_debug_wgrad_fold), so a changed threshold has to move the table deliberately; the table reaches every
route the path has; the checker passes the references themselves in every mode and flags the failures this path can have, each at
the stage it belongs to and at no stage upstream; and the scheduled-sampling problems have no near ties by construction."""
import pytest
import torch

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine
from tests import decoder_tf_cases as F
from tests import sched_sample_cases as SC
from tests.decoder_tf_cases import CASES, ORDER, RUNS, Mode

BY = {c.id: c for c in CASES}
PTR = 0x7F0000010000          # a fake, 16-byte aligned, non-null device pointer: never dereferenced
DT = {"f32": L.F32, "bf16": L.BF16}


def test_ids_are_unique():
    assert len(BY) == len(CASES) and len({F.run_id(r) for r in RUNS}) == len(RUNS)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_names_the_route_the_selection_takes(case):
    assert F.route_str(F.select(case)) == case.route


def gate_splits(case, l):
    """splits= of the route line of layer l's per-step gate product as gic_decoder_forward_tf issues it (no_split unset)."""
    c = case
    with engine.route_only() as r:
        assert L.load().gic_gemm(PTR, PTR, PTR, c.B, 4 * c.H, c.ldx(l), c.ldx(l), c.ldx(l), 4 * c.H, 1, 1, DT[c.dtype], L.F32, PTR, 0, 1.0, None) == 0
        line = r.last()
    return int(line.split(" splits=")[1].split()[0])


def projection_tile(case):
    """The tile height of the vocabulary product over all B * Tmax rows, from its route line gemm<in,out,a_kc,b_kc,BM,BN,...>."""
    c = case
    with engine.route_only() as r:
        assert L.load().gic_gemm(PTR, PTR, PTR, c.B * c.Tmax, c.V, c.H, c.H, c.H, c.V, 1, 1, DT[c.dtype], L.F32, PTR, 0, 1.0, None) == 0
        line = r.last()
    assert line.startswith("gemm<"), line
    return int(line.split(",")[4])


def probe(case):
    """The GEMM selection's answers for a case (deterministic mode off): the gate products' split count per layer, whether the merged
    dW_ih | dW_hh product of a layer folds its bias sums (the fold's tile divides din), whether dW_out folds db_out, the projection's tile."""
    c, lib = case, L.load()
    rows = c.B * c.Tmax
    fold = lambda M, N: lib.gic_debug_wgrad_fold(PTR, PTR, M, N, rows, M, N, 0, 0, DT[c.dtype], L.F32)
    wg = []
    for l in range(c.NL):
        tn = fold(4 * c.H, c.ldx(l))
        wg.append("folded" if tn and c.din(l) % tn == 0 else "unfolded")
    return (f"gate={','.join(str(gate_splits(c, l)) for l in range(c.NL))} wgrad={','.join(wg)} "
            f"out={'folded' if fold(c.V, c.H) else 'unfolded'} proj={projection_tile(c)}")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_names_what_the_gemm_selection_answers(case):
    engine.set_deterministic(False)
    assert probe(case) == case.gemm


def test_table_reaches_every_route_of_the_path():
    for dtype in ("f32", "bf16"):
        S = [F.select(c) for c in CASES if c.dtype == dtype]
        assert {s["bwd"] for s in S} == {"fused", "generic"} and {s["ss_logits"] for s in S} == {"fused", "gemm"}
        assert {s["softmax_bwd"] for s in S} == {"scalar", "vec8" if dtype == "f32" else "vec5"}
        assert {s["scatter"] for s in S} == {"none", "rows", "scalar"}
        assert {s["drop"] for c, s in zip([c for c in CASES if c.dtype == dtype], S) if any(m.drop for cc, m in RUNS if cc is c)} >= {"vec/vec"}
    assert {c.gemm.split()[2] for c in CASES} == {"out=folded", "out=unfolded"}
    assert any("wgrad=folded" in c.gemm for c in CASES) and any("wgrad=unfolded" in c.gemm for c in CASES)
    assert BY["tf-splitk-bf16"].gemm.startswith("gate=4 ")                     # splits K in the plain call
    assert BY["tf-short-f32"].Tmax < BY["tf-short-f32"].T and BY["tf-short-f32"].Lc != BY["tf-short-f32"].Tmax - 1
    assert BY["tf-len1-f32"].Tmax == 1 < BY["tf-len1-f32"].T and BY["tf-nocaps-f32"].Lc == 0
    assert BY["tf-rows-f32"].B * BY["tf-rows-f32"].Tmax == 360 and set(BY["tf-rows-f32"].lengths) == set(range(1, 10))
    assert {c.gemm.split()[3] for c in CASES} == {"proj=64", "proj=128"}
    assert BY["tf-tiles-f32"].nblk == 16 and 1 in BY["tf-base-f32"].lengths and BY["tf-base-f32"].NL == 2
    # the modes laid over the table
    modes = lambda name: {m.id for c, m in RUNS if c.id == name + "-f32"}
    for c in CASES:
        assert {"pretrain", "adv"} <= {m.id for cc, m in RUNS if cc is c}
    ss = {f"ss{p:g}-{k}" for p in (0.5, 1.0) for k in ("sample", "argmax")}
    for name in ("tf-base", "tf-generic", "tf-tiles", "tf-splitk", "tf-nocaps"):
        assert ss <= modes(name), name
    for name in ("tf-base", "tf-generic"):
        assert {"adv-drop", "pretrain-drop-philox", "ss0.5-sample-drop", "ss1-argmax-drop-philox"} <= modes(name), name
    assert "adv-philox" in modes("tf-base") and "adv-det" in modes("tf-base") and "adv-det" in modes("tf-odd")
    P, X = F.data(BY["tf-base-f32"])
    assert int(X["caps"].min()) == -3 and int(X["caps"].max()) == 64 + 5 and X["lengths"][1] == 7


def fill(case, mode, mut=None, gaps=None):
    """A correct result in storage precision (the references themselves, cast), optionally mutated."""
    P, X = F.data(case, mode)
    img = F.images(case, P)
    st, ws, grads = F.new_state(case), F.new_ws(case), F.new_grads(case, P)
    F.run_forward(case, mode, P, img, X, st, None, mut=mut, gaps=gaps)
    F.run_backward(case, mode, P, img, X, st, ws, grads, None, mut=mut)
    return P, img, X, st, ws, grads


def check(case, mode, P, img, X, st, ws, grads):
    rep = F.Report()
    F.run_forward(case, mode, P, img, X, st, rep)
    F.run_backward(case, mode, P, img, X, st, ws, grads, rep)
    return rep


@pytest.mark.parametrize("run", RUNS, ids=[F.run_id(r) for r in RUNS])
def test_checker_passes_a_correct_result(run):
    """Every case in every mode: the references, cast to storage precision, pass every stage the mode has.  Scheduled sampling: in the
    f32 reference chain every replaced position's top-2 score gap is at least MIN_GAP (tests/test_sched_sample_api.py's condition), so
    the inputs hold no near tie by construction; a seed that fails is replaced."""
    case, mode = run
    gaps = []
    bufs = fill(case, mode, gaps=gaps)
    rep = check(case, mode, *bufs)
    assert not rep.failed, rep.failed
    pretrain = mode.pretrain or mode.ss is not None
    want = set(ORDER) - {"logits" if not pretrain else "y"} - ({"dlogits"} if pretrain else set())
    if not mode.ss:
        want -= {"replaced", "pick", "inputs", "ss tail"}
    elif case.Tmax < 2:
        want -= {"replaced", "pick", "inputs"} | ({"ss tail"} if case.Lc == 0 else set())
    elif case.Lc == case.Tmax - 1:
        want -= {"ss tail"}
    if not mode.drop:
        want -= {"hdrop"}
    if case.NL == 1:
        want -= {"h copies"}
    if not mode.det:
        want -= {"d_b_ih == d_b_hh"}
    assert want <= set(rep.ratio), want - set(rep.ratio)
    if mode.ss and case.dtype == "f32" and case.Tmax > 1:
        print(f"{F.run_id(run)}: replaced {len(gaps)}, min top-2 gap {min(gaps, default=float('inf')):.3e}")
        assert min(gaps, default=1.0) >= SC.MIN_GAP
        if mode.ss[0] == 1.0:
            assert gaps
        st = bufs[3]
        assert mode.ss[0] < 1.0 or (st["replaced"][:, :case.Tmax - 1] == (torch.arange(1, case.Tmax)[None, :] < bufs[2]["lengths"][:, None]).int()).all()


def test_padded_steps_exist_where_the_table_says_so():
    for c in CASES:
        X = F.data(c)[1]
        assert bool(F.padded_pairs(c, X).any()) == (min(c.lengths) < c.Tmax)


def _wgrad_over_T_slots(case, P, img, X, st, ws, grads):
    """9. one more slot's rows in a weight gradient: the stale d_gates of the last step against slot Tmax's x rows."""
    grads[1] += ws["dgates"][0][case.Tmax - 1].float().t() @ st["xh"][0][case.Tmax][:, :case.E].float()


def _d_b_ih_misses_a_row(case, P, img, X, st, ws, grads):
    """10. the bias gradient without the row (t = 0, b = 0)."""
    grads[3] -= ws["dgates"][0][0][0].float()


ADV, PRE = Mode(False), Mode(True)
MUTATIONS = [
    ("tf-base-f32", PRE, "pad_advance", "pad state"),                          # 1. a padded row's (h, c) advanced instead of held
    ("tf-base-bf16", PRE, "pad_hout", "hout"),                                 # 2. a non-zero hout row past its length
    ("tf-base-f32", ADV, "pad_gates", "pad gates"),                            # 3. non-zero gates at a padded step
    ("tf-short-bf16", PRE, "hn_slot_T", "h_n"),                                # 4. h_n taken from slot T instead of slot Tmax
    ("tf-short-f32", PRE, "hout_stride_T", "hout"),                            # 5. hout written with row stride T * H instead of Tmax * H
    ("tf-base-f32", ADV, "u_tbv", "y"),                                        # 6. u indexed [Tmax, B, V]
    ("tf-base-bf16", ADV, "dhout_unmasked", "dhout"),                          # 7. dhout not zeroed past the lengths
    ("tf-short-f32", PRE, "ids_stride_tm1", "d_embed"),                        # 8. d_embed scattered with ids_stride = Tmax - 1
    ("tf-short-f32", ADV, _wgrad_over_T_slots, "d_w_ih"),                      # 9. a weight gradient summed over T instead of Tmax slots
    ("tf-base-bf16", PRE, _d_b_ih_misses_a_row, "d_b_ih"),                     # 10. d_b_ih missing one row
    ("tf-base-bf16", Mode(True, (1.0, "sample")), "pick_second", "pick"),      # 11. a pick that is the second-best candidate
    ("tf-base-f32", Mode(True, (0.5, "argmax")), "replaced_past", "replaced"),  # 12. `replaced` set at a position past its length
    ("tf-base-f32", Mode(True, (1.0, "argmax")), "xrow_teacher", "xrows"),     # 13. a replaced position's x row still the teacher's embedding
    ("tf-base-bf16", Mode(False, drop=F.DROP_P), "hdrop_scaled", "hdrop"),     # 14. hdrop scaled at a dropped element
]


@pytest.mark.parametrize("cid,mode,mut,stage", MUTATIONS, ids=[f"{i + 1}-{m if isinstance(m, str) else m.__name__.strip('_')}" for i, (_, _, m, _) in enumerate(MUTATIONS)])
def test_checker_flags_the_failures_this_path_can_have(cid, mode, mut, stage):
    """Each mutation of a correct result is flagged at its own stage and at no stage upstream of it."""
    case = BY[cid]
    bufs = fill(case, mode, mut=None if callable(mut) else mut)
    if callable(mut):
        mut(case, *bufs)
    rep = check(case, mode, *bufs)
    assert stage in rep.failed, (rep.failed, rep.ratio)
    assert min(ORDER.index(s) for s in rep.failed) == ORDER.index(stage), rep.failed


def test_deterministic_mode_holds_the_two_bias_gradients_to_the_same_bits():
    case, mode = BY["tf-base-f32"], Mode(False, det=True)
    bufs = fill(case, mode)
    bufs[5][3][2] += 1e-6 * (1 + bufs[5][3][2].abs())
    rep = check(case, mode, *bufs)
    assert "d_b_ih == d_b_hh" in rep.failed
