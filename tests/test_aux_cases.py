"""tests/aux_cases.py without a GPU: (a) every fp64 reference agrees with torch's own operator on the case inputs, (b) a plain f32
emulation of every kernel passes the checker on every case (the bounds are not too tight), (c) the checker flags seeded faults, each at
its kernel, (d) the case ids are unique and the table reaches every routing branch of the kernels (the launch conditions of cast2d,
colsum, bn_stats and clip_adam restated in Python)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_step as O
from tests import aux_cases as A

F64 = torch.float64
# (a): err / bound of an fp64 evaluation by torch's operator.  The bounds are of the order of 2^-24 of the value, fp64 rounds at 2^-53; a
# cancelling expression (BatchNorm of a constant column, scaled by 1 / sqrt(eps)) amplifies that by a few hundred.
EXACT = 1e-4


def ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------------------------------------------------------- (d) tables
@pytest.mark.parametrize("table", [A.ADAM_CASES, A.GAN_CASES, A.ROLLOUT_CASES, A.XENT_CASES, A.CAST_CASES, A.COLSUM_CASES, A.EMB_CASES,
                                   A.STATS_CASES, A.BN1D_CASES], ids=["adam", "gan", "rollout", "xent", "cast", "colsum", "emb", "stats", "bn1d"])
def test_case_ids_are_unique(table):
    assert len(set(ids(table))) == len(table)


def test_adam_table_reaches_every_branch():
    routes = {c.id: A.adam_route(c) for c in A.ADAM_CASES}
    R = list(routes.values())
    assert any(not r["al"] and r["n4"] == 0 and r["tail"] > 2048 for r in R)                    # the unaligned fallback, more than one block
    assert any(r["al"] and r["n4"] > 0 and 0 < r["tail"] < 4 for r in R)                        # 16-byte body and a scalar tail
    assert any(r["al"] and r["n4"] > 0 and r["tail"] == 0 for r in R)
    assert any(r["n4"] == 0 and r["al"] for r in R)                                             # n < 4
    assert sum(r["vec_wraps"] for r in R) >= 2 and any(r["capped"] and r["vec_wraps"] for r in R)
    assert any(r["sq_vec_blocks"] > 0 and r["sq_scalar_blocks"] == 1 for r in R)                # whole blocks and a partial last one
    assert any(r["sq_vec_blocks"] == 0 and r["sq_scalar_blocks"] > 1 for r in R)                # a misaligned g: every block scalar
    only_g = A.adam_route(A.AdamCase(12291, off=(0, 1, 0, 0)))
    assert not only_g["al"] and only_g["sq_vec_blocks"] == 0
    assert A.adam_route(A.AdamCase(2 * 2 ** 20 + 5))["blocks"] == 1025 and A.adam_route(A.AdamCase(2 * 2 ** 20 + 5))["vec_wraps"]
    assert A.adam_route(A.AdamCase(2048 * 2048 + 4096 + 3)) == {"sq_vec_blocks": 1025, "sq_scalar_blocks": 1, "al": True, "n4": 1049600, "tail": 3,
                                                                  "blocks": 2048, "capped": True, "vec_wraps": True, "tail_wraps": False}
    assert {c.regime for c in A.ADAM_CASES} == {"clip", "noclip", "zero_g", "inf"} and {c.t for c in A.ADAM_CASES} >= {1, 2, 3, 10000}
    assert [A.adam_partials(n) for n in (1, 4096, 4097)] == [1, 1, 2]


def test_cast_table_reaches_every_branch():
    for c in A.CAST_CASES:
        assert A.cast_route(c)[0] == c.route, c.id
    assert {(c.src, c.dst, c.route) for c in A.CAST_CASES} == {("f32", "f32", "scalar"), ("f32", "bf16", "scalar"), ("f32", "bf16", "vec"),
                                                               ("bf16", "f32", "scalar"), ("bf16", "bf16", "scalar")}
    assert A.cast_route(A.CAST_BASE)[0] == "vec" and all(A.cast_route(c)[0] == "scalar" for c in A.CAST_BROKEN)
    assert A.cast_route(A.CAST_BIG) == ("vec", 2048, True, True)
    assert A.cast_route(A.CastCase("f32", "bf16", 1, 8, 8, 8, route="vec")) == ("vec", 1, False, True)
    for pair in {(c.src, c.dst, c.route) for c in A.CAST_CASES}:
        mine = [c for c in A.CAST_CASES if (c.src, c.dst, c.route) == pair]
        assert any(c.lds > c.cols and c.ldd > c.cols for c in mine) and any(c.lds == c.cols == c.ldd for c in mine), pair


def test_colsum_table_reaches_every_branch():
    plans = {c.id: A.colsum_plan(c) for c in A.COLSUM_CASES}
    for d, vn in (("f32", 4), ("bf16", 8)):
        assert plans[A.ColsumCase(d, 65, 64, 64).id][0] == "vec"
        for broken in (A.ColsumCase(d, 65, 63, 64), A.ColsumCase(d, 65, 64, 64 + vn // 2), A.ColsumCase(d, 65, 64, 64, off=1)):
            assert plans[broken.id][0] == "scalar", broken.id
        mine = [c for c in A.COLSUM_CASES if c.dtype == d]
        for kernel in ("vec", "scalar"):
            k = [c for c in mine if c.route == kernel]
            assert {(c.acc, c.det) for c in k} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (d, kernel)
            assert any(c.rows < 8 for c in k) and any(c.lda > c.cols for c in k) and any(plans[c.id][3] > 2 for c in k), (d, kernel)
        assert any(c.route == "vec" and c.rows % (32 * plans[c.id][3]) for c in mine)                   # rows past the end re-read row r
    assert A.colsum_plan(A.ColsumCase("f32", 2100, 904, 904)) == ("vec", 8, 8, 33)
    assert A.colsum_plan(A.ColsumCase("f32", 2100, 904, 904, det=1))[3] == 2 and A.colsum_plan(A.ColsumCase("f32", 2100, 904, 904, acc=1, det=1))[3] == 1


def test_stats_table_reaches_every_branch():
    plans = [A.stats_parts(c.rows, c.C) for c in A.STATS_CASES]
    assert any(256 % CG and P > 1 for CG, RL, gx, R, P in plans) and {CG for CG, *_ in plans} >= {1, 3, 9, 25, 32}
    assert any(gx > 1 and P > 1 for CG, RL, gx, R, P in plans)
    assert A.stats_parts(4099, 24) == (3, 85, 1, 64, 65) and A.stats_parts(4099, 200) == (25, 10, 1, 64, 65)
    assert A.stats_parts(257, 2048) == (32, 8, 8, 52, 5) and A.stats_parts(1, 8) == (1, 256, 1, 1, 1)
    for CG, RL, gx, R, P in plans:
        assert (RL - 1) * CG + CG - 1 < 256 and P <= 256


def test_embedding_table_reaches_every_branch():
    runs = set()
    for c in A.EMB_CASES:
        if c.pattern == "runs" and c.n <= A.K_SCATTER_MAX_N:
            idc = A.emb_clamped(c, A.emb_inputs(c))
            runs |= set(torch.bincount(idc).tolist())
            assert int(A.emb_inputs(c)["ids"].min()) < 0 and int(A.emb_inputs(c)["ids"].max()) == 2 ** 40
    assert runs >= {63, 64, 65, 1100}
    assert {c.E for c in A.EMB_CASES} >= {1, 63, 64, 65, 200} and {c.n for c in A.EMB_CASES} >= {1, 2, 3, 1000, 8191, 8192, 8193}
    assert {(c.zero_first, c.det) for c in A.EMB_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    corner = [c for c in A.EMB_CASES if c.pattern == "corner" and c.det][0]
    ids_ = A.emb_inputs(corner)["ids"]
    assert (int(ids_[-1]) << 13 | (corner.n - 1)) == 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- (a) references
@pytest.mark.parametrize("case", [c for c in A.ADAM_CASES if c.n <= 12291], ids=ids([c for c in A.ADAM_CASES if c.n <= 12291]))
def test_adam_reference_is_clip_grad_norm_then_torch_adam(case):
    inp = A.adam_inputs(case)
    h = A.ADAM_HYPER
    p = torch.nn.Parameter(inp["p"].double())
    p.grad = inp["g"].double().clone()
    opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"])
    opt.state[p] = {"step": torch.tensor(float(case.t - 1)), "exp_avg": inp["m"].double().clone(), "exp_avg_sq": inp["v"].double().clone()}
    norm = torch.nn.utils.clip_grad_norm_([p], h["clip"])
    opt.step()
    st = opt.state[p]
    out = {"norm": norm.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "p": p.detach(), "step": int(st["step"])}
    ratios = A.adam_check(case, inp, out, f32_scalars=False)
    assert max(ratios.values()) < EXACT
    if case.regime == "inf":
        assert int(torch.isnan(out["p"]).sum()) == 1 and bool(torch.isnan(out["p"][case.n // 3]))
    if case.regime == "noclip":                                 # coef saturates at exactly 1: plain Adam
        assert A.adam_coef(float(norm)) == 1.0


def _torch_losses(t, r, f, g):
    """(g_loss, d_loss) from torch's own operators (the oracle's softplus is clamp + log1p, whose autograd at a logit of exactly 0 is
    the clamp's one-sided derivative; binary_cross_entropy_with_logits has the smooth one)."""
    bce = lambda x, one: F.binary_cross_entropy_with_logits(x, torch.ones_like(x) if one else torch.zeros_like(x))
    if t in ("standard", "JS", "KL"):
        d = bce(r, True) + bce(f, False)
        return {"standard": bce(g, True), "JS": -bce(g, False), "KL": (-g).mean()}[t], d
    if t == "hinge":
        return -g.mean(), torch.relu(1 - r).mean() + torch.relu(1 + f).mean()
    if t == "tv":
        return (-torch.tanh(g)).mean(), (torch.tanh(f) - torch.tanh(r)).mean()
    return bce(f - r, True), bce(r - f, True)


@pytest.mark.parametrize("case", A.GAN_CASES, ids=ids(A.GAN_CASES))
def test_gan_reference_is_the_oracles_get_losses(case):
    inp = A.gan_inputs(case)
    x = {k: v.double().requires_grad_() for k, v in inp.items()}
    o_g, o_d = O.get_losses(x["d_real"], x["d_fake"], x["g_out"], case.type)
    g_loss, d_loss = _torch_losses(case.type, x["d_real"], x["d_fake"], x["g_out"])
    torch.testing.assert_close(torch.stack([g_loss, d_loss]), torch.stack([o_g, o_d]), rtol=1e-12, atol=1e-12)
    out = {"losses": torch.stack([o_g, o_d]).detach()}
    zero = torch.zeros(case.n, dtype=F64)
    gr = torch.autograd.grad(d_loss, [x["d_real"], x["d_fake"]], allow_unused=True)
    gg = torch.autograd.grad(g_loss, [x["g_out"], x["d_real"], x["d_fake"]], allow_unused=True)
    for name, t in zip(A.GRAD_NAMES, list(gr) + list(gg)):
        out[name] = zero if t is None else t
    assert A.gan_check(case, inp, out)["gan_losses"] < EXACT


@pytest.mark.parametrize("case", A.XENT_CASES, ids=ids(A.XENT_CASES))
def test_xent_reference_is_cross_entropy(case):
    inp = A.xent_inputs(case)
    x = inp["logits"].double().requires_grad_()
    tgt = inp["targets"]
    bad = (tgt < 0) | (tgt >= case.V)
    w = inp["w"].double() if inp["w"] is not None else torch.ones(case.rows, dtype=F64)
    rows = F.cross_entropy(x, tgt.clamp(0, case.V - 1), reduction="none") * w
    dl, = torch.autograd.grad(rows.sum() / case.rows, x)
    rows = torch.where(bad, torch.full_like(rows, float("nan")), rows).detach()
    out = {"loss": rows.sum() / case.rows, "row_loss": rows, "dlogits": dl}
    if case.dtype == "bf16":
        out["dlogits"] = dl                                    # (fp64: inside the bf16 allowance as well)
    assert max(A.xent_check(case, inp, out).values()) < EXACT
    if case.bad is None and not case.weighted:
        assert abs(float(out["loss"]) - float(F.cross_entropy(x.detach(), tgt))) < 1e-12


@pytest.mark.parametrize("case", A.BN1D_CASES, ids=ids(A.BN1D_CASES))
def test_bn1d_reference_is_batch_norm(case):
    inp = A.bn1d_inputs(case)
    x, g, b = (inp[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    rm, rv = inp["rm0"].double().clone(), inp["rv0"].double().clone()
    mom, eps = A.f32(case.momentum), A.f32(A.BN_EPS)
    if case.training and case.B == 1:                           # torch refuses one value per channel: xhat = 0, var = 0, unbiased factor 1
        y = (x - x) * g + b
        rm, rv = (1 - mom) * rm + mom * x.detach()[0], (1 - mom) * rv
    else:
        y = F.batch_norm(x, rm, rv, g, b, bool(case.training), mom, eps)
    dx, dg, db = torch.autograd.grad(y, [x, g, b], inp["dy"].double())
    xd = x.detach()
    mean, var = (xd.mean(0), xd.var(0, unbiased=False)) if case.training else (inp["rm0"].double(), inp["rv0"].double())
    invstd = (var + eps) ** -0.5
    out = {"y": y.detach(), "xhat": (y.detach() - b.detach()) / g.detach(), "invstd": invstd, "rm": rm, "rv": rv}
    if not case.training:
        out["rm"], out["rv"] = inp["rm0"], inp["rv0"]
    out["xhat"] = (xd - mean) * invstd                         # (y - beta) / gamma cancels: the definition instead, y checks it
    assert A.bn1d_check_fwd(case, inp, out)["bn1d_fwd"] < EXACT
    assert A.bn1d_check_bwd(case, inp, out, {"dx": dx, "dgamma": dg, "dbeta": db})["bn1d_bwd"] < EXACT


@pytest.mark.parametrize("case", [c for c in A.EMB_CASES if not c.det], ids=ids([c for c in A.EMB_CASES if not c.det]))
def test_scatter_reference_is_index_add(case):
    inp = A.emb_inputs(case)
    ref, mag, cnt = A.emb_scatter_reference(case, inp)
    want = torch.zeros(case.V, case.E, dtype=F64) if case.zero_first else inp["dw0"].double()
    want.index_add_(0, A.emb_clamped(case, inp), inp["dout"].double())
    torch.testing.assert_close(ref, want, rtol=1e-13, atol=1e-13)
    assert int(cnt.sum()) == case.n
    emb = F.embedding(A.emb_clamped(case, inp), inp["weight"])
    assert A.emb_check_fwd(case, inp, {"out": emb}) == {"embedding_fwd": 0.0}


def test_bf16_reference_is_torchs_conversion():
    x = torch.cat([A.cast_values(33, 100).reshape(-1), A.cast_values(7, 24).reshape(-1)])
    mine, theirs = A.bf16_rne(x), x.bfloat16()
    A.same_bits("cast2d", "rne", "bf16", mine, theirs, nan_free=True)
    assert bool(torch.isnan(mine[torch.isnan(x)]).all())
    sp = torch.tensor(A.SPECIALS, dtype=torch.float32).bfloat16().float().tolist()
    assert sp[5] == 1.0 and sp[6] == 1.0 + 2.0 ** -6 and sp[9] == 1.0 + 2.0 ** -7 and sp[10] == 1.0          # ties to even, and their neighbours
    assert sp[11] == float("inf") and sp[13] == 3.3895313892515355e38 and sp[14] == float("inf") and sp[2] > 0 and sp[3] == 0.0


@pytest.mark.parametrize("case", A.COLSUM_CASES[:8] + A.STATS_CASES[:6], ids=lambda c: c.id)
def test_sum_references_are_torch_sums(case):
    if isinstance(case, A.ColsumCase):
        inp = A.colsum_inputs(case)
        a = inp["A"][:, :case.cols].double()
        got = torch.stack([a[:, c].sum() for c in range(case.cols)]) + (inp["out0"].double() if case.acc else 0)
        assert max(A.colsum_check(case, inp, {"out": got}).values()) < EXACT
    else:
        y = A.stats_inputs(case)["y"].double()
        got = torch.cat([torch.einsum("rc->c", y), torch.einsum("rc,rc->c", y, y)])
        assert A.stats_check(case, A.stats_inputs(case), {"stats": got})["bn_stats"] < EXACT


# ---------------------------------------------------------------------------------------------------------------- (b) emulations
def _emulate(case):
    """(ratios of the f32 emulation under the checker)"""
    if isinstance(case, A.AdamCase):
        inp = A.adam_inputs(case)
        return A.adam_check(case, inp, A.adam_emulate(case, inp))
    if isinstance(case, A.GanCase):
        inp = A.gan_inputs(case)
        out = A.gan_emulate(case, inp)
        bare = A.gan_emulate(case, inp, want_grads=False)
        assert torch.equal(out["losses"], bare["losses"])
        return A.merge(A.gan_check(case, inp, out), A.gan_check(case, inp, bare))
    if isinstance(case, A.RolloutCase):
        inp = A.rollout_inputs(case)
        return A.rollout_check(case, inp, A.rollout_emulate(case, inp))
    if isinstance(case, A.XentCase):
        inp = A.xent_inputs(case)
        return A.xent_check(case, inp, A.xent_emulate(case, inp))
    if isinstance(case, A.CastCase):
        inp = A.cast_inputs(case)
        return A.cast_check(case, inp, A.cast_emulate(case, inp))
    if isinstance(case, A.ColsumCase):
        inp = A.colsum_inputs(case)
        return A.colsum_check(case, inp, A.colsum_emulate(case, inp))
    if isinstance(case, A.EmbCase):
        inp = A.emb_inputs(case)
        out = A.emb_emulate(case, inp)
        return A.merge(A.emb_check_fwd(case, inp, out), A.emb_check_bwd(case, inp, out))
    if isinstance(case, A.StatsCase):
        inp = A.stats_inputs(case)
        return A.stats_check(case, inp, A.stats_emulate(case, inp))
    inp = A.bn1d_inputs(case)
    out = A.bn1d_emulate(case, inp)
    return A.merge(A.bn1d_check_fwd(case, inp, out), A.bn1d_check_bwd(case, inp, out, out))


ALL = (A.ADAM_CASES + A.GAN_CASES + A.ROLLOUT_CASES + A.XENT_CASES + A.CAST_CASES + A.COLSUM_CASES + A.EMB_CASES + A.STATS_CASES + A.BN1D_CASES)


@pytest.mark.parametrize("case", ALL, ids=[type(c).__name__[:-4] + "-" + c.id for c in ALL])
def test_f32_emulation_is_within_the_bounds(case):
    ratios = _emulate(case)
    assert ratios and all(0 <= r <= 1 for r in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------- (c) seeded faults
def flagged(kernel, fn):
    with pytest.raises(A.Mismatch) as e:
        fn()
    assert e.value.kernel == kernel, (e.value.kernel, str(e.value))
    assert e.value.case and e.value.index >= 0 and "got" in str(e.value) and "bound" in str(e.value)
    return e.value


@pytest.mark.parametrize("fault,case", [("seam_piece", A.AdamCase(4097)), ("seam_piece", A.AdamCase(12291)), ("coef_twice", A.AdamCase(12291)),
                                        ("coef_twice", A.AdamCase(4097, t=10000)), ("t_minus_1", A.AdamCase(4097, t=2)),
                                        ("t_minus_1", A.AdamCase(4097, t=3))], ids=lambda x: x if isinstance(x, str) else x.id)
def test_checker_flags_adam_faults(fault, case):
    assert case in A.ADAM_CASES
    inp = A.adam_inputs(case)
    e = flagged("clip_adam", lambda: A.adam_check(case, inp, A.adam_emulate(case, inp, fault)))
    if fault == "seam_piece":
        assert e.index == A.adam_route(case)["n4"] * 4 - 4


def test_checker_flags_a_wrong_norm_and_step():
    case = A.AdamCase(12291)
    inp = A.adam_inputs(case)
    out = A.adam_emulate(case, inp)
    out["norm"] = out["norm"] * (1 + 2.0 ** -17)
    flagged("sqnorm_partial", lambda: A.adam_check(case, inp, out))
    out = A.adam_emulate(case, inp)
    out["step"] = case.t + 1
    with pytest.raises(AssertionError, match="step_count"):
        A.adam_check(case, inp, out)
    out = A.adam_emulate(case, inp)
    out["p"][int(torch.nonzero(inp["pad"])[0])] = -0.0                  # the padding leaves +0
    flagged("clip_adam", lambda: A.adam_check(case, inp, out))


def test_checker_flags_a_loss_mean_over_the_padded_count():
    for t in A.LOSS_TYPES:
        case = A.GanCase(t, 9001)
        inp = A.gan_inputs(case)
        e = flagged("gan_losses", lambda: A.gan_check(case, inp, A.gan_emulate(case, inp, "padded_mean")))
        assert e.what in ("g_loss", "d_loss")


def test_checker_flags_swapped_rollout_indices():
    case = A.RolloutCase(2, 4, 3, 5)
    inp = A.rollout_inputs(case)
    flagged("rollout_rewards", lambda: A.rollout_check(case, inp, A.rollout_emulate(case, inp, "swap_n_r")))


def test_checker_flags_a_colsum_without_its_last_row_group():
    for case in (A.ColsumCase("f32", 2100, 904, 904), A.ColsumCase("bf16", 65, 63, 64), A.ColsumCase("f32", 9, 63, 71)):
        case = case._replace(route=A.colsum_plan(case)[0])
        assert case in A.COLSUM_CASES
        inp = A.colsum_inputs(case)
        flagged("colsum_vec" if case.route == "vec" else "colsum", lambda: A.colsum_check(case, inp, A.colsum_emulate(case, inp, "drop_last_group")))


def test_checker_flags_a_cast_without_its_odd_last_piece():
    for case in (A.CAST_BIG, A.CastCase("f32", "bf16", 1, 8, 8, 8, route="vec"), A.CastCase("f32", "bf16", 7, 24, 32, 32, route="vec")):
        assert case in A.CAST_CASES
        inp = A.cast_inputs(case)
        e = flagged("cast2d", lambda: A.cast_check(case, inp, A.cast_emulate(case, inp, "skip_odd_piece")))
        assert e.index == (case.rows - 1) * case.cols + case.cols - 8
    case = A.CastCase("f32", "bf16", 7, 24, 32, 32, route="vec")
    out = A.cast_emulate(case, A.cast_inputs(case))
    out["dst"][3, 25] = 0.0                                             # a write into the padding
    flagged("cast2d", lambda: A.cast_check(case, A.cast_inputs(case), out))


def test_checker_flags_a_descending_scatter_run():
    for case in [c for c in A.EMB_CASES if c.det and c.n >= 1000 and c.pattern != "corner"]:
        inp = A.emb_inputs(case)
        out = A.emb_emulate(case, inp, "descending")
        flagged("det_scatter", lambda: A.emb_check_bwd(case, inp, out))


def test_checker_flags_bn_stats_read_from_the_first_row_lane():
    for case in (A.StatsCase("f32", 24, 4099), A.StatsCase("bf16", 200, 65), A.StatsCase("f32", 2048, 257)):
        assert case in A.STATS_CASES
        inp = A.stats_inputs(case)
        flagged("bn_stats", lambda: A.stats_check(case, inp, A.stats_emulate(case, inp, "red_g")))


def test_checker_flags_nan_and_reports_the_first_index():
    ref = torch.arange(6, dtype=F64)
    got = ref.float()
    got[4] = float("nan")
    e = flagged("k", lambda: A.check("k", "c", "w", got, ref, 1.0))
    assert (e.index, e.what) == (4, "w")
    ref2 = ref.clone()
    ref2[2] = float("nan")
    assert flagged("k", lambda: A.check("k", "c", "w", ref.float(), ref2, 1.0)).index == 2
    ref2[2] = float("inf")
    got = ref.float()
    got[2] = 3e38
    assert flagged("k", lambda: A.check("k", "c", "w", got, ref2, 1.0)).index == 2
    assert A.check("k", "c", "w", ref.float() + 0.25, ref, 0.5) == pytest.approx(0.5)
    assert flagged("k", lambda: A.check("k", "c", "w", ref.float(), ref, float("nan"))).index == 0
    assert A.check("k", "c", "w", ref.float(), ref, 0.0) == 0.0


def test_xent_checker_needs_nan_on_a_bad_target_only():
    case = A.XentCase("f32", 5, 257, True, -1)
    inp = A.xent_inputs(case)
    out = A.xent_emulate(case, inp)
    assert bool(torch.isnan(out["row_loss"][2])) and bool(torch.isnan(out["loss"]))
    out["row_loss"][2] = 0.0
    flagged("xent_rows", lambda: A.xent_check(case, inp, out))
    out = A.xent_emulate(case, inp)
    out["loss"] = torch.tensor(0.0)
    flagged("mean", lambda: A.xent_check(case, inp, out))
    good = A.XentCase("bf16", 5, 1000, True)
    out = A.xent_emulate(good, A.xent_inputs(good))
    out["dlogits"] = (out["dlogits"].float() * (1 + 2.0 ** -6)).bfloat16()
    flagged("xent_rows", lambda: A.xent_check(good, A.xent_inputs(good), out))
