"""The discriminator case table (tests/disc_cases.py) without a GPU: every case names the convolution kernels select_disc_fwd /
select_disc_bwd (csrc/disc.hip) take for it -- by a Python restatement of their conditions AND by the library's own plan
(gic_debug_disc_plan), which must agree in both modes of gic_set_deterministic, so a threshold that moves in either has to move the table
deliberately and the table's coverage of every variant is the library's --, every highway route the scan reaches is pinned on one small shape, the integer regime of every case really has ties and zeros, and the checker flags the
failures this kernel family can have, each at the stage it belongs to."""
import ctypes

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine
from tests import disc_cases as D
from tests.disc_cases import CASES, HIGHWAY

P = 0x7F0000010000          # a fake, aligned, non-null device pointer
DT = {"f32": L.F32, "bf16": L.BF16}
EXACT_SEED, ROUND_SEED = 101, 202


def test_ids_are_unique():
    ids = [c.id for c in CASES] + [h.id for h in HIGHWAY]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_names_the_kernels_the_selection_takes(case):
    assert D.select(case) == (case.fwd, case.bwd_x, case.bwd_w)


def dims_of(case):
    d = L.DiscDims()
    d.B, d.L, d.V, d.De, d.R, d.nconv = case.B, case.L, case.V, case.De, case.R, len(case.fs)
    for k, (f, n) in enumerate(zip(case.fs, case.nf)):
        d.fsize[k], d.nfilt[k] = f, n
    d.F, d.Fp, d.dtype, d.drop_p = case.F, case.Fp, DT[case.dtype], D.DROP_P
    return d


def library_plan(d, flags):
    """gic_debug_disc_plan's lines (host-only; no pointer is involved)."""
    out = ctypes.create_string_buffer(2048)
    status = L.load().gic_debug_disc_plan(ctypes.byref(d), flags, out, len(out))
    assert status == 0, L.load().gic_last_error()
    return out.value.decode().splitlines()


FWD_KERNEL = {"bf16": "disc_conv_pool_fwd_bf16_kernel<{t}>", "mfma": "disc_conv_pool_fwd_mfma_kernel<{t}>",
              "scalar8": "disc_conv_pool_fwd_kernel<{t},8>", "scalar32": "disc_conv_pool_fwd_kernel<{t},32>"}
BWD_W_KERNEL = {"lds": "disc_conv_pool_bwd_w_lds_kernel<{t},8>", "w8": "disc_conv_pool_bwd_w_kernel<{t},8>", "w32": "disc_conv_pool_bwd_w_kernel<{t},32>"}
BWD_X_KERNEL = {"small1": ("disc_conv_pool_bwd_x_small_kernel<{t},32,8>", " rpb=1"), "small4": ("disc_conv_pool_bwd_x_small_kernel<{t},32,8>", " rpb=4"),
                "general": ("disc_conv_pool_bwd_x_kernel<{t}>", "")}


def kernel_and_extras(line):
    """'kernel<..> grid=.. block=.. lds=.. extras' -> (kernel, ' extras')."""
    head, _, tail = line.partition(" lds=")
    return head.split(" grid=")[0], tail.partition(" ")[1] + tail.partition(" ")[2]


@pytest.mark.parametrize("det", [False, True], ids=["", "det"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_library_plan_is_the_restated_selection(case, det):
    """The library's own selection (gic_debug_disc_plan = make_ctx + select_disc_fwd + select_disc_bwd) names exactly the kernels, rows
    per block, disc_out_bwd blocks, weight-gradient block rows and fold launches that D.select / D.det_plan restate, in both modes of
    gic_set_deterministic: neither side can drift alone, and test_table_reaches_every_kernel_and_edge speaks for the library."""
    t = case.dtype
    fwd, bwd_x, bwd_w = D.select(case)
    engine.set_deterministic(det)
    try:
        if case.forward_only:
            lines = library_plan(dims_of(case), L.DISC_PLAN_NO_ARGMAX)
            assert kernel_and_extras(lines[0]) == (FWD_KERNEL[fwd].format(t=t), "")
            return
        lines = library_plan(dims_of(case), L.DISC_PLAN_GRADS | L.DISC_PLAN_TRAIN)
        no_grads = library_plan(dims_of(case), L.DISC_PLAN_TRAIN | L.DISC_PLAN_HW_UNALIGNED)
    finally:
        engine.set_deterministic(False)
    out_blocks, out_fold, rows_y, w_fold = D.det_plan(case, det)
    xk, xe = BWD_X_KERNEL[bwd_x]
    want = [(FWD_KERNEL[fwd], ""), ("disc_out_bwd_kernel<{t}>", f" blocks={out_blocks} part={int(out_fold)}")]
    want += [("disc_out_fold_kernel", "")] * out_fold
    want += [("disc_highway_bwd_vec_kernel<{t}>", ""), (BWD_W_KERNEL[bwd_w], f" rows_y={rows_y} part={int(w_fold)}")]
    want += [("disc_wgrad_fold_kernel", "")] * w_fold
    want += [(xk, xe)]
    assert [kernel_and_extras(l) for l in lines] == [(k.format(t=t), e) for k, e in want]
    # the generator's path (no parameter gradients: no weight gradient, nothing folded in either mode), `dh` off its alignment
    assert [kernel_and_extras(l) for l in no_grads] == [(k.format(t=t), e) for k, e in
                                                       [(FWD_KERNEL[fwd], ""), ("disc_out_bwd_kernel<{t}>", " blocks=256 part=0"),
                                                        ("disc_highway_bwd_kernel<{t}>", ""), (xk, xe)]]


def test_table_reaches_every_kernel_and_edge():
    got = {(c.dtype,) + D.select(c) for c in CASES}
    for dtype in ("f32", "bf16"):
        assert {g[1] for g in got if g[0] == dtype} >= {"mfma", "scalar8", "scalar32"}
        assert {g[2] for g in got if g[0] == dtype} >= {"small1", "small4", "general"}
        assert {g[3] for g in got if g[0] == dtype} >= {"lds", "w8", "w32"}
    assert ("bf16", "bf16", None, None) in got and ("bf16", "mfma", None, None) in got
    by = {c.id: c for c in CASES}
    assert by["r24-L11-f32"].MR % 16 == 8 and by["fo-r24-L11-bf16"].MR % 32 == 8                # partial workgroups
    assert by["r10-b205-f32"].MR >= 2048 and by["r10-b205-f32"].MR % 4                          # rpb = 4, MR % 4 != 0
    assert by["r24-L8-f32"].L == max(by["r24-L8-f32"].fs)                                       # one window
    assert sum(-(-n // 16) for n in by["r24-L11-f32"].nf) > 8                                   # the tile & 7 round robin wraps
    assert by["fp8-f32"].Fp == by["fp8-f32"].F
    # deterministic mode: the caps bite down to one block row / one block
    assert D.det_plan(by["det-cap5-f32"]) == (3, True, 1, False)
    assert D.det_plan(by["det-cap3-f32"]) == (1, False, 1, False)
    assert D.det_plan(by["r24-L11-f32"])[1] and D.det_plan(by["r24-L11-f32"])[3]
    assert D.det_plan(by["s4-L12-f32"])[3] and D.det_plan(by["s2-L16-f32"])[3] and not D.det_plan(by["r5-L255-f32"])[3]


def disc_fwd(rows, F, Fp, dtype, train=1, **state):
    """gic_disc_fwd in route-only mode (as tests/test_route.py::disc_fwd): it selects its highway product (M = rows, N = F, K = Fp) and
    launches nothing.  One caption of `rows` representations; `state` replaces buffers of the saved state."""
    d, prm, sh, st = L.DiscDims(), L.DiscParams(), L.DiscShadow(), L.DiscState()
    d.B, d.L, d.V, d.De, d.R, d.nconv = 1, 3, 50, rows, rows, 1
    d.fsize[0], d.nfilt[0] = 2, F
    d.F, d.Fp, d.dtype, d.drop_p = F, Fp, DT[dtype], D.DROP_P
    for s in (prm, sh, st):
        for name, ctype in s._fields_:
            setattr(s, name, P if ctype is L.c_void_p else ctype(P))
    for name, ptr in state.items():
        setattr(st, name, ptr)
    return d, prm, sh, st, None, 0, P, train, None, 1, P, None, 0, None


@pytest.mark.parametrize("h", HIGHWAY, ids=[h.id for h in HIGHWAY])
def test_highway_shape_takes_the_route_it_names(h):
    assert h.rows % 4 and h.rows % 128, "rows off the Philox quads and the tiles"
    assert h.F % 8 or not h.route.startswith("tile8"), "live and dead columns in one 8-column patch"
    for train in (1, 0):
        with engine.route_only() as r:
            status = L.load().gic_disc_fwd(*disc_fwd(h.rows, h.F, h.Fp, h.dtype, train, hpre=P + h.off))
            line = r.last()
        assert status == 0 and line.split(" lds=")[0] == h.route, line


def test_every_highway_route_of_the_scan_has_a_shape():
    lib = L.load()
    reached = {}
    with engine.route_only() as r:
        for dtype in ("f32", "bf16"):
            for off in (0, 8):
                for F, Fp in D.HIGHWAY_SCAN_F:
                    for rows in D.HIGHWAY_SCAN_ROWS:
                        assert lib.gic_disc_fwd(*disc_fwd(rows, F, Fp, dtype, hpre=P + off)) == 0
                        reached.setdefault(r.last().split(" grid=")[0], (rows, F, Fp, dtype, off))
    pinned = {h.route.split(" grid=")[0] for h in HIGHWAY}
    missing = {k: v for k, v in reached.items() if k not in pinned}
    assert not missing, f"highway routes without a shape (first shape that reaches each): {missing}"
    assert len(reached) >= 12
    assert {k.split("<")[0] for k in reached} == {"gemm", "tile8"}


@pytest.mark.parametrize("case", [c for c in CASES if c.exact], ids=[c.id for c in CASES if c.exact])
def test_integer_regime_has_ties_and_zeros(case):
    g = torch.Generator().manual_seed(EXACT_SEED)
    Pm = D.make_params(case, "exact", g)
    X = D.make_inputs(case, g, train=False)
    tied, zero = D.tie_counts(case, Pm, X["ids"])
    assert tied >= 100 and zero >= 100, (tied, zero)
    mag = max(int(f * case.s * 6 + 3) for f in case.fs)
    assert mag <= 256, "every pre-activation is an integer exact in bf16"


# ---------------------------------------------------------------------------------------------------------------- the checker can fail
def filled(case, regime, mut=None, soft=False, accumulate=False):
    """A correct result in storage precision (the references themselves, cast), optionally mutated, and what the checker says of it."""
    g = torch.Generator().manual_seed(EXACT_SEED if regime == "exact" else ROUND_SEED)
    Pm = D.make_params(case, regime, g)
    X = D.make_inputs(case, g, soft=soft, train=not case.forward_only)
    img = D.images(case, Pm)
    st, ws = D.new_state(case), D.new_ws(case)
    exact = regime == "exact"
    D.run_forward(case, Pm, img, X, st, None, exact=exact, mut=mut)
    rep = D.Report()
    D.run_forward(case, Pm, img, X, st, rep, exact=exact)
    if not exact and not case.forward_only:
        G0 = [torch.randn(p.shape, generator=g) for p in Pm] if accumulate else None
        grads = [None] * len(Pm)
        D.run_backward(case, Pm, img, X, st, ws, grads, G0, None, None, mut=mut)
        D.run_backward(case, Pm, img, X, st, ws, grads, G0, ws.get("d_inp"), rep)
    return rep


BY = {c.id: c for c in CASES}


@pytest.mark.parametrize("cid,soft,acc", [("r24-L11-f32", False, False), ("r24-L11-bf16", True, True), ("s2-L16-bf16", False, True),
                                          ("s4-L12-f32", True, False), ("r5-L255-bf16", False, False), ("fo-r24-L64-bf16", False, False),
                                          ("fp8-bf16", True, False)])
def test_checker_passes_a_correct_result(cid, soft, acc):
    rep = filled(BY[cid], "rounding", soft=soft, accumulate=acc)
    assert not rep.failed, rep.failed
    assert {"emb", "pooled", "ydrop", "feat", "logits"} <= set(rep.ratio)
    if not BY[cid].forward_only:
        assert {"argmax", "hpre", "keep", "dfeat", "dydrop", "dh", "dpooled", "demb", "emb_w", "hw_w", "hw_b", "f2o_w", "f2o_b", "o2l_w", "o2l_b",
                "conv_w.0", "conv_b.0"} <= set(rep.ratio)
    if BY[cid].exact:
        assert not filled(BY[cid], "exact").failed


@pytest.mark.parametrize("cid,regime,mut,stage,allowed", [
    ("r24-L11-f32", "rounding", "drop_last_t", "pooled", {"pooled", "argmax"}),
    ("r24-L11-bf16", "rounding", "drop_last_t", "pooled", {"pooled", "argmax"}),
    ("fo-r24-L11-bf16", "rounding", "drop_last_t", "pooled", {"pooled"}),
    ("r24-L11-f32", "exact", "drop_last_t", "pooled", {"pooled", "argmax"}),
    ("r24-L11-bf16", "rounding", "no_taps_4_7", "pooled", {"pooled", "argmax"}),
    ("r24-L11-f32", "exact", "no_taps_4_7", "pooled", {"pooled", "argmax"}),
    ("r24-L11-f32", "exact", "argmax_ge", "argmax", {"argmax"}),
    ("r5-L255-bf16", "exact", "argmax_ge", "argmax", {"argmax"}),
    ("r24-L11-bf16", "rounding", "partial_group_unwritten", "pooled", {"pooled", "argmax"}),
    ("r24-L11-f32", "rounding", "tile_to_neighbour", "pooled", {"pooled", "argmax"}),
    ("r24-L11-bf16", "rounding", "keep_quad_shift", "keep", {"keep"}),
    ("r24-L11-f32", "rounding", "wgrad_block_row_omitted", "conv_w.3", {f"conv_{p}.{k}" for p in "wb" for k in range(5)}),
    ("s4-L12-bf16", "rounding", "wgrad_block_row_omitted", "conv_w.1", {"conv_w.0", "conv_w.1", "conv_b.0", "conv_b.1"}),
], ids=lambda v: v if isinstance(v, str) else "")
def test_checker_flags_the_failures_this_family_can_have(cid, regime, mut, stage, allowed):
    """The last time step dropped from the max, taps 4..7 of the wide filters zeroed, >= for > in the argmax, the rows of the last
    partial group left unwritten, a filter tile written to its neighbour's columns, a 4-row quad of `keep` shifted by a row, one block
    row's partial omitted from a weight gradient: each flagged at its own stage and (the rest of the result follows from the mutated
    buffers) nowhere else."""
    rep = filled(BY[cid], regime, mut=mut)
    assert stage in rep.failed, (rep.failed, rep.ratio)
    assert set(rep.failed) <= allowed, rep.failed
