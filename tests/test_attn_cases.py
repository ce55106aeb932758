"""The attention-decoder case table (tests/attn_cases.py) without a GPU: the restated launch geometry reaches every edge the table
names (so a changed tile constant makes the table fail instead of silently testing nothing), the roll-out workspace layout restated
from csrc/attn_rollout.hip's header has the library's size, the references alone lie within their own bounds for every case and dtype
(the clean fill), and the checker flags the failures this kernel family can have, each at the stage it belongs to and nowhere upstream,
in every case where it applies and in both dtypes."""
import ctypes as C

import pytest
import torch

from tests import attn_cases as A
from tests.attn_cases import CASES, FAMILY, ORDER

BY = {c.id: c for c in CASES}
G = {c.id: A.geometry(c) for c in CASES}


def test_ids_are_unique_and_every_case_has_both_dtypes():
    assert len(BY) == len(CASES) == 36
    assert all(f"{c.name}-f32" in BY and f"{c.name}-bf16" in BY for c in CASES)


def test_dims_are_ones_the_library_takes():
    for c in CASES:
        assert c.V % 4 == 0 and c.E % 8 == 0 and c.H % 8 == 0 and c.C % 8 == 0 and c.A % 8 == 0 and c.P <= A.MAX_P and c.A <= A.MAX_A
        if c.family == "tf":
            assert len(c.lengths) == c.B and 1 <= min(c.lengths) and max(c.lengths) <= c.L


def test_geometry_reaches_every_edge_the_table_names():
    g = G.__getitem__
    # attn_dalpha's last block is partial
    assert g("base-f32")["dalpha_blocks"] == (7, 3) and g("steps-f32")["dalpha_blocks"][1] == 1
    # attn_bwd column blocks and attn_fwd width passes, partial last
    assert g("wide-A-f32")["bwd_blocks"] == (3, 8) and g("wide-A-bf16")["bwd_blocks"] == (2, 8)
    assert g("wide-A-f32")["width_passes"] == (3, 8) and g("wide-A-bf16")["width_passes"] == (2, 8)
    assert g("base-f32")["bwd_blocks"] == (1, 16)
    # the LDS ceilings
    for dt in ("f32", "bf16"):
        assert BY[f"max-A-{dt}"].A == A.MAX_A and BY[f"max-P-{dt}"].P == A.MAX_P
        assert BY[f"tf-max-A-{dt}"].A == A.MAX_A and BY[f"tf-max-P-{dt}"].P == A.MAX_P
        assert g(f"max-A-{dt}")["lds_fwd"] == (2048 + 3) * 4 and g(f"max-P-{dt}")["lds_fwd"] == (8 + 1024) * 4
        assert g(f"max-A-{dt}")["bwd_blocks"] == ((8, 256) if dt == "f32" else (4, 512))
        assert g(f"max-P-{dt}")["softmax_passes"] == 4 and g(f"max-P-{dt}")["lds_bwd"] == (1024 + 8 * (256 if dt == "f32" else 512)) * 4
        # the second softmax pass and the tails of the 16-position energy pass, the 8-position z pass, the 16-position backward pass
        m = g(f"many-P-{dt}")
        assert m["softmax_passes"] == 2 and m["fwd_pos"] == (19, 12) and m["z_pos"] == (38, 4) and m["bwd_pos"] == (19, 12)
        assert BY[f"one-pos-{dt}"].P == 1
        # roll-out tiles
        assert g(f"r-tiles-{dt}")["rows_tile"] == 32 and g(f"r-tiles-{dt}")["rows_tiles"] == (2, 8)
        assert g(f"r-tall-{dt}")["rows_tile"] == 16 and g(f"r-tall-{dt}")["rows_tiles"] == (2, 4) and g(f"r-tall-{dt}")["rows_lds"] == 87808
        assert A.rows_lds(32, 1024) > 64 * 1024 >= A.rows_lds(32, 70)
        rc = g(f"r-chunks-{dt}")
        assert rc["rows_pos"] == 2 and rc["rows_width"] == (3, 8) and rc["rows_chan"] == ((3, 8) if dt == "f32" else (2, 8)) and rc["rows_tiles"] == (1, 5)
        # the packed step kernels: P = 70 is no multiple of the 8-position group and exceeds a wave; the last ctx workgroup is partial
        tc = g(f"tf-chunks-{dt}")
        assert tc["energy_blocks"] == (9, 6) and BY[f"tf-chunks-{dt}"].P > 64 and tc["ctx_blocks"] == ((3, 8) if dt == "f32" else (2, 8))
    # z channel passes with 8 live channels in the last; the attn_dalpha lane loop and the dz re-zero loop run more than once; K chunks
    assert g("wide-C-f32")["z_chan"] == (3, 8) and g("wide-C-bf16")["z_chan"] == (2, 8)
    for dt in ("f32", "bf16"):
        assert g(f"wide-C-{dt}")["dalpha_lanes"] > 1 and g(f"wide-C-{dt}")["dz_zero"] == 3 and g(f"wide-C-{dt}")["lstm_chunks"] > 1
        assert g(f"base-{dt}")["dalpha_lanes"] == 1 and g(f"base-{dt}")["lstm_chunks"] == 1
    # several width passes of the energy kernel: A = 264 is two passes of 256 columns in f32 and one of 512 in bf16 (tf-max-A has four)
    assert g("tf-chunks-f32")["width_passes"] == (2, 8) and g("tf-chunks-bf16")["width_passes"] == (1, 264) and g("tf-max-A-bf16")["width_passes"][0] == 4
    # the 64 KB request of attn_step_energy at k = 8 (tests/test_gpu_attn_beam.py)
    assert g("tf-max-A-f32")["lds_energy"](8) == 64 * 1024
    # steps: accumulation over 6 steps; tf-short: Tmax < T; lengths of every kind
    assert BY["steps-f32"].L == 6 and BY["tf-short-f32"].steps == 5 < BY["tf-short-f32"].L and BY["tf-base-f32"].steps == BY["tf-base-f32"].L
    assert min(BY["tf-base-f32"].lengths) == 1


def test_saturated_case_is_saturated():
    for dt in ("f32", "bf16"):
        case = BY[f"saturated-{dt}"]
        P, X = A.data(case)
        img, st = A.images(case, P), A.new_state(case)
        A.fill_forward(case, P, img, X, st)
        x = st["fproj"].double() + st["hproj"][1].double()[:, None, :]
        al, bound, e, _ = A.attention(st["fproj"].double(), st["hproj"][1].double(), P[10].double())
        assert float((e.max(1).values - e.min(1).values).max()) > 104 and float(x.abs().max()) > 10
        assert int(((al == 0) & (bound == 0)).sum()) > 0 and bool((st["alpha"][1][al == 0] == 0).all())
        assert int((torch.tanh(x).float().abs() == 1).sum()) > 0


def _lib():
    from gan_image_captioning_amd import _lib as L
    return L, L.load()


@pytest.mark.parametrize("case", FAMILY["rollout"], ids=[c.id for c in FAMILY["rollout"]])
def test_rollout_layout_has_the_librarys_size(case):
    L, lib = _lib()
    out = C.c_uint64(0)
    dims = L.AttnDims(case.B, case.L, case.V, case.E, case.H, case.C, case.P, case.A, L.F32 if case.dtype == "f32" else L.BF16)
    L.check(lib.gic_attn_rollout_ws_bytes(C.byref(dims), case.rows, C.byref(out)), "gic_attn_rollout_ws_bytes")
    lay, total = A.rollout_layout(case)
    assert total == int(out.value)
    assert all(o % 256 == 0 for o, _ in lay.values()) and list(lay) == ["xh", "c", "gpre", "hp", "rowkey", "logits"]


def test_rollout_layout_with_the_fused_vocabulary_product():
    """V >= 128 in bf16: from gumbelmax_from rows on a step needs no logits, the scratch holds one row less than that."""
    L, lib = _lib()
    case = A.Case("big-V", "rollout", 4, 3, 256, 8, 16, 24, 9, 16, "bf16", N=40)
    assert A.gumbelmax_from(case) == 128 * 79 + 1 and A.gumbelmax_from(case._replace(dtype="f32")) == 0
    for c in (case, case._replace(N=2000)):
        out = C.c_uint64(0)
        L.check(lib.gic_attn_rollout_ws_bytes(C.byref(L.AttnDims(c.B, c.L, c.V, c.E, c.H, c.C, c.P, c.A, L.BF16)), c.rows, C.byref(out)), "ws_bytes")
        assert A.rollout_layout(c)[1] == int(out.value)


# ---------------------------------------------------------------------------------------------------------------- checker self-test
def fill(case, mut=None, post=None, backward=True):
    P, X = A.data(case)
    img = A.images(case, P)
    st = A.new_state(case)
    A.fill_forward(case, P, img, X, st, mut)
    ws = grads = roll = None
    if case.family == "rollout":
        roll = A.new_rollout_ws(case)
        A.run_rollout(case, P, img, X, st, roll, None, mut)
    elif backward:
        ws, grads = A.new_ws(case), A.new_grads(case, P)
        A.run_backward(case, P, img, X, st, ws, grads, None, mut)
    if post is not None:
        post(case, st, ws)
    return P, X, img, st, ws, grads, roll


def check(case, P, X, img, st, ws, grads, roll):
    rep = A.Report()
    A.check_images(case, P, img, rep)
    A.run_forward(case, P, img, X, st, rep)
    if roll is not None:
        A.run_rollout(case, P, img, X, st, roll, rep)
    elif ws is not None:
        A.run_backward(case, P, img, X, st, ws, grads, rep)
    return rep


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_references_lie_within_their_bounds(case):
    """Filling the buffers from the references in storage precision leaves the Report clean, and every stage was compared."""
    rep = check(case, *fill(case))
    assert not rep.failed, rep.failed
    want = set(ORDER) - {"past length", "alphas out", "h_n c_n", "untouched", "rollout z", "rollout joined", "dfproj_act"}
    if case.family == "rollout":
        want = {s for s in want if ORDER.index(s) <= ORDER.index("h copies")} | {"rollout z", "rollout joined"}
    if case.family != "train":
        want |= {"alphas out", "h_n c_n"}
    if case.family == "tf":
        want |= ({"past length"} if min(case.lengths) < case.steps else set()) | ({"untouched"} if case.steps < case.L else set())
    if case.dtype == "bf16" and case.family != "rollout":
        want |= {"dfproj_act"}
    assert want <= set(rep.ratio), want - set(rep.ratio)


def _dalpha_stale(case, st, ws):
    ws["dalpha"].view(-1)[-(case.B * case.P % 4):] = 7.0


def _dz_nonzero(case, st, ws):
    ws["dz"][-1, -1] = 2.0 ** -100


def _dh_extra_nonzero(case, st, ws):
    ws["dh_extra"][0, 0] = -0.0                            # all-zero BITS are asked for


smooth = lambda c: c.P > 1 and not c.sat                   # the attention gradients are exactly zero at P = 1 and vanish when saturated
MUTATIONS = [
    # (mutation, the stage that must flag it, the cases it applies to, needs the backward)
    ("alpha_first256", "alpha", lambda c: c.P > 256, False),
    ("alpha_scaled", "alpha", lambda c: True, False),
    ("z_last8_stale", "z", lambda c: True, False),
    ("z_tail_dropped", "z", lambda c: c.P % 8 != 0, False),
    ("z_neighbour_alpha", "z", lambda c: c.B > 1 and c.P > 1 and not c.sat, False),
    ("hproj_from_h_t", "hproj", lambda c: True, False),
    ("past_alpha", "past length", lambda c: c.family == "tf" and min(c.lengths) < c.steps, False),
    ("past_z", "past length", lambda c: c.family == "tf" and min(c.lengths) < c.steps, False),
    ("dalpha_no_add", "dalpha", lambda c: c.family == "tf", True),
    (_dalpha_stale, "dalpha", lambda c: c.family != "rollout" and c.B * c.P % 4 != 0, True),
    ("dhproj_last_block_zero", "dhproj", lambda c: c.family != "rollout" and smooth(c) and c.A % (256 if c.dtype == "f32" else 512) != 0, True),
    ("dhproj_pos_dropped", "dhproj", lambda c: c.family != "rollout" and smooth(c) and c.P >= 4, True),
    ("dfproj_step_missing", "dfproj", lambda c: c.family != "rollout" and smooth(c), True),
    ("dfproj_last_pass", "dfproj", lambda c: c.family != "rollout" and smooth(c), True),
    ("dwa_overwritten", "dwa_rows", lambda c: c.family != "rollout" and smooth(c), True),
    ("dgates_no_extra", "dgates", lambda c: c.family != "rollout" and smooth(c), True),
    (_dz_nonzero, "dz zero", lambda c: c.family != "rollout", True),
    (_dh_extra_nonzero, "dh_extra zero", lambda c: c.family != "rollout", True),
    ("roll_tail_stale", "rollout z", lambda c: c.family == "rollout", False),
    ("roll_chan_first_group", "rollout z", lambda c: c.family == "rollout" and c.C > 128, False),
    ("roll_joined_bits", "rollout joined", lambda c: c.family == "rollout", False),
]
_name = lambda m: m if isinstance(m, str) else m.__name__.lstrip("_")
MATRIX = [(m, stage, c, bwd) for m, stage, applies, bwd in MUTATIONS for c in CASES if applies(c)]


def test_every_mutation_applies_somewhere_in_both_dtypes():
    for m, *_ in MUTATIONS:
        assert {c.dtype for mm, _, c, _ in MATRIX if mm is m} == {"f32", "bf16"}, _name(m)


@pytest.mark.parametrize("mut,stage,case,bwd", MATRIX, ids=[f"{_name(m)}-{c.id}" for m, _, c, _ in MATRIX])
def test_checker_flags_the_failures_this_family_can_have(mut, stage, case, bwd):
    """Each mutation of a correct result is flagged at its own stage and at no stage upstream of it."""
    bufs = fill(case, None if callable(mut) else mut, mut if callable(mut) else None, backward=bwd)
    rep = check(case, *bufs)
    assert stage in rep.failed, (rep.failed, rep.ratio.get(stage))
    assert min(ORDER.index(s) for s in rep.failed) == ORDER.index(stage), rep.failed


def test_teacher_forced_entry_points_take_a_caller_owned_state():
    import inspect

    from gan_image_captioning_amd import engine
    for name in ("forward_tf", "forward_scheduled", "sample_fwd"):
        p = inspect.signature(getattr(engine.AttnDecoderEngine, name)).parameters
        assert "state" in p and p["state"].default is None, name
