"""The inference-mode trunk's convolution routes and the inputs of its GPU walk, pinned without a GPU.

Route-only mode (tests/test_route.py): gic_conv2d with a null statistics pointer validates and selects over fake, aligned pointers and
launches nothing.  Pinned here: every layer of every walk of tests/trunk_eval_cases.py and every isolated case takes its recorded
variant; the walks and cases together reach every variant that any layer of the scan grid reaches; no eval route is one of the kernels
that exist under the BatchNorm-sum epilogue only; and the running statistics the GPU walk is given leave every tensor of an eval pass
finite and alive (CPU oracle, the small walks)."""
import pytest
import torch

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine
from tests import trunk_eval_cases as T

P = 0x7F0000010000          # a fake, aligned, non-null device pointer
DT = {"bf16": L.BF16, "f32": L.F32}


def route(l, N, dtype):
    with engine.route_only() as r:
        status = L.load().gic_conv2d(*T.conv_args(l, N, DT[dtype], P, P, P))
        line = r.last()
    assert status == 0, (l, N, dtype, line)
    return line


@pytest.mark.parametrize("walk", T.EVAL_WALKS, ids=[w.id for w in T.EVAL_WALKS])
def test_every_layer_of_a_walk_takes_its_recorded_route(walk):
    dtype, det = T.MODES[walk.mode]
    want = walk.key_of()
    layers = T.trunk_layers(walk.arch, walk.S)
    assert sorted(want) == sorted(l.name for l in layers) and sum(len(v.split()) for v in walk.routes.values()) == len(layers)
    engine.set_deterministic(det)
    try:
        got = {l.name: T.route_key(route(l, walk.N, dtype)) for l in layers}
    finally:
        engine.set_deterministic(False)
    moved = {n: (want[n], got[n]) for n in want if want[n] != got[n]}
    assert not moved, moved


def test_trunk_layers_restate_the_plan():
    """The layer table the routes are probed with is the geometry TrunkPlan launches (its buffers are shaped on the meta device)."""
    from gan_image_captioning_amd.encoder_engine import TrunkPlan
    from gan_image_captioning_amd.trunk import ResNetTrunk
    for arch, S, N in (("resnet18", 96, 2), ("resnet50", 200, 3), ("resnet50", 64, 3)):
        plan = TrunkPlan(ResNetTrunk(arch), L.BF16)
        plan._running_table = lambda b, dev: None
        b = plan._buffers(N, S, torch.device("meta"))
        layers = {l.name: l for l in T.trunk_layers(arch, S)}
        assert [s.name for s in plan.steps] == [l.name for l in T.trunk_layers(arch, S)]
        assert tuple(b["xin"].shape) == (N, S + 6, S + 6, 4) and layers["0"].out_hw() == tuple(b["y0"].shape[1:3])
        for blk, e in zip(plan.blocks, b["blocks"]):
            for s, buf in ((blk["c1"], "y1"), (blk["c2"], "y2"), (blk["c3"], "y3"), (blk["ds"], "yd")):
                if s is None:
                    continue
                l = layers[s.name]
                assert (l.cin, l.cout, l.k, l.kw, l.stride, l.pad) == (s.cin, s.cout, s.k, s.k, s.stride, s.pad), s.name
                reads_out_map = buf == "y3" or (buf == "y2" and blk["kind"] == "basic")         # (as _run_trunk passes H)
                assert l.out_hw() == tuple(e[buf].shape[1:3]) and l.H == l.W == (e["hout"] if reads_out_map else e["hin"]), s.name


@pytest.mark.parametrize("case", T.PLAIN_CONVS, ids=[c.id for c in T.PLAIN_CONVS])
def test_every_plain_convolution_takes_its_recorded_route(case):
    assert T.route_key(route(case, case.N, case.dtype)) == case.key


def scan():
    """variant key -> (rows, K, cout) of the smallest shape of the grid that reaches it"""
    best = {}
    for dtype in ("bf16", "f32"):
        for arch in T.SCAN_ARCHS:
            for S in T.SCAN_S:
                for l in T.trunk_layers(arch, S):
                    ho, wo = l.out_hw()
                    for N in T.SCAN_N:
                        key = T.route_key(route(l, N, dtype))
                        rank = (N * ho * wo, l.k * l.kw * l.cin, l.cout)
                        if key not in best or rank < best[key]:
                            best[key] = rank
    return best


def test_the_tables_reach_every_variant_the_scan_reaches():
    best = scan()
    per_key = {c.key: c for c in T.PLAIN_CONVS[:len(best)]}
    assert set(per_key) == set(best), (set(best) - set(per_key), set(per_key) - set(best))
    # ... each with the smallest shape that reaches it
    for key, rank in best.items():
        c = per_key[key]
        assert (c.rows(), c.k * c.kw * c.cin, c.cout) == rank, (key, c, rank)
    covered = {c.key for c in T.PLAIN_CONVS} | {k for w in T.EVAL_WALKS for k in w.routes}
    assert covered == set(best), covered ^ set(best)


def test_no_eval_route_is_a_statistics_epilogue_kernel():
    keys = set(scan()) | {c.key for c in T.PLAIN_CONVS} | {k for w in T.EVAL_WALKS for k in w.routes}
    for key in keys:
        name = key.split("<")[0]
        assert name not in T.BNSTATS_ONLY and name in ("tile8", "gemm"), key
        f = key[key.index("<") + 1:-1].split(",")
        if name == "tile8":        # <TO, BN, EPI, CONV, NS, ABN, ARES, AMAXK>
            assert f[2] == "0" and f[3] == "true" and f[5] == f[6] == "false", key
        else:                      # <TI, TO, AKC, BKC, BM, BN, VEC, EPI, CONV, PIPE>
            assert f[7] == "0" and f[8] == "true" and f[0] == f[1], key
    # the same shapes WITH a statistics pointer do take them (the premise of the finding): the stem, a 3x3 / stride 1, a wide shallow 1x1
    for l, N in ((T.Layer("stem", 230, 230, 4, 64, 7, 8, 2, 0), 64), (T.Layer("3x3", 56, 56, 64, 64, 3, 3, 1, 1), 64), (T.Layer("1x1", 56, 56, 64, 64, 1, 1, 1, 0), 64)):
        a = list(T.conv_args(l, N, L.BF16, P, P, P))
        a[3], a[4] = P, 8
        with engine.route_only() as r:
            assert L.load().gic_conv2d(*a) == 0
            assert r.last().split("<")[0].split(" ")[0] in T.BNSTATS_ONLY, r.last()
        assert T.route_key(route(l, N, "bf16")).startswith("tile8<bf16,"), l


SMALL = [w for w in T.EVAL_WALKS if w.mode != "det"]          # (under a second each on the CPU; the det walk has the bf16 walk's inputs)


@pytest.mark.parametrize("walk", SMALL, ids=[w.id for w in SMALL])
def test_the_walks_running_statistics_leave_the_eval_pass_alive(walk):
    """What the GPU walk's inputs must meet (it asserts the same of the tensors the GPU stored): with the perturbed running statistics,
    the var = 0 / 1e-6 channels and a zero gamma in every layer, every formed tensor of the eval pass is finite and has at least 10 %
    non-zero elements -- and the forced channels are there."""
    formed, feat, table = T.cpu_eval_pass(walk.arch, walk.S, walk.N, emulate_bf16=walk.mode != "fp32")
    assert len(formed) == 1 + sum(2 if l.name.endswith("conv1") else (1 if l.name.endswith("conv2") and walk.arch == "resnet50" else 0)
                                  for l in T.trunk_layers(walk.arch, walk.S))
    for name, t in formed.items():
        assert torch.isfinite(t).all(), name
        assert float((t != 0).float().mean()) >= 0.10, (name, float((t != 0).float().mean()))
    assert torch.isfinite(feat).all()
    for name, (rm, rv, ga) in table.items():
        assert int((rv == 0).sum()) == 2 and int((rv == 1e-6).sum()) == 2 and int((ga == 0).sum()) >= 1 and bool((ga < 0).any()), name
        assert torch.isfinite(rm).all() and bool((rv >= 0).all())
