"""The GEMM case table (tests/gemm_cases.py) against the selection, without a GPU: every case takes the variant it names, the table
reaches every variant the scan grid reaches, and K = 0 selects (it used to divide by zero on the host).  Route-only mode as in
tests/test_route.py: the pointers are fake, 16-byte aligned and never dereferenced.

The same for the second table (WGRAD_CASES: the weight-gradient form and the caller-only flags, through gic_debug_gemm_desc): every row's
route and status, the table's coverage of its own scan grid, and the checker of tests/test_gpu_gemm_wgrad.py against a plain numpy
emulation of the form: the sound emulation passes at every case, each seeded fault fails at the case named for it."""
import pytest

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine
from tests import gemm_cases as G
from tests.gemm_cases import CASES, DTYPE_PAIRS, LAYOUTS, SCAN_K, SCAN_M, SCAN_N, WGRAD_CASES, desc_args, gemm_args, route_key

P = 0x7F0000010000          # a fake, aligned, non-null device pointer
DT = {"f32": L.F32, "bf16": L.BF16}


def route(case):
    engine.set_deterministic(case.det)
    try:
        with engine.route_only() as r:
            status = L.load().gic_gemm(*gemm_args(case, P, P, P, P, DT))
            line = r.last()
    finally:
        engine.set_deterministic(False)
    return status, line


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_takes_the_variant_it_names(case):
    status, line = route(case)
    assert status == 0, line
    assert route_key(line) == case.key, line


def test_ids_are_unique():
    ids = [c.id for c in CASES + WGRAD_CASES]
    assert len(set(ids)) == len(ids)


def test_table_covers_every_variant_the_scan_grid_reaches():
    """Every (variant key, overwrite | accumulate) pair selected anywhere on the grid (tight leading dimensions, bias present) has a
    case: a new instantiation in the dispatch fails here until the table (and so the GPU matrix) has one for it."""
    lib = L.load()
    gemm, last = lib.gic_gemm, lib.gic_debug_last_route
    found = {}
    with engine.route_only():
        for lay, (a_kc, b_kc) in LAYOUTS.items():
            for i_dt, o_dt in DTYPE_PAIRS:
                for M in SCAN_M:
                    for N in SCAN_N:
                        for K in SCAN_K:
                            for acc in (0, 1):
                                status = gemm(P, P, P, M, N, K, K if a_kc else M, K if b_kc else N, N, a_kc, b_kc, DT[i_dt], DT[o_dt], P, acc, 1.0, None)
                                assert status == 0, (M, N, K, lay, i_dt, o_dt, acc)
                                found.setdefault((last(), acc), (M, N, K, lay, i_dt, o_dt))
    reached = {}
    for (line, acc), shape in found.items():
        reached.setdefault((route_key(line.decode()), acc), shape)
    covered = {(c.key, c.accumulate) for c in CASES if not c.det}
    missing = {k: v for k, v in reached.items() if k not in covered}
    assert not missing, f"{len(missing)} of {len(reached)} variants without a case (first shape that reaches each): {missing}"
    assert len(reached) >= 132


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("i_dt,o_dt", [("f32", "f32"), ("bf16", "f32")])
def test_k_zero_selects(i_dt, o_dt, acc):
    """K = 0 is the empty sum, C = bias (+ C): one split of no K tiles through the 4-wave kernel."""
    with engine.route_only() as r:
        status = L.load().gic_gemm(P, P, P, 64, 64, 0, 8, 8, 64, 1, 1, DT[i_dt], DT[o_dt], P, acc, 1.0, None)
        line = r.last()
    assert status == 0
    assert line.startswith(f"gemm<{i_dt},{o_dt},true,true,64,64,") and " splits=1 " in line and " zero=0" in line, line


# ------------------------------------------------------------------------------------------ the second table
def wroute(case):
    """(status, route line) of a WGRAD_CASES row over fake pointers; a misaligned operand sits one element (2 bytes) off."""
    engine.set_deterministic(case.det)
    try:
        with engine.route_only() as r:
            status = L.load().gic_debug_gemm_desc(*desc_args(case, P + 2 * (case.misalign == "A"), P + 2 * (case.misalign == "B"), P, P, DT, P, P, P))
            line = r.last()
    finally:
        engine.set_deterministic(False)
    return status, line


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.id for c in WGRAD_CASES])
def test_descriptor_case_takes_the_route_and_status_it_names(case):
    status, line = wroute(case)
    assert status == case.status, line
    assert route_key(line) == case.key, line
    assert case.form == (" a_sum=" in line)
    if case.form:
        assert line.endswith(f" a_sum={case.sums} n_split={case.n_split if case.c2 else 0}"), line


def test_descriptor_table_holds_what_the_issue_names():
    """Both tile widths of the form in both split states, its zero fill and its atomics onto a live C, bf16 output, every extras
    combination, and the flags' routes: c_zeroed turns ("split", "zero") into ("split", "nozero"), no_split into "nosplit"."""
    forms = {(c.key[0].split(",")[4], c.key[1], c.key[2]) for c in WGRAD_CASES if c.form}
    assert forms >= {(t, "nosplit", "nozero") for t in ("64", "128")} | {(t, "split", z) for t in ("64", "128") for z in ("zero", "nozero")}
    assert {(c.sums, c.c2) for c in WGRAD_CASES if c.form} >= set(G.WSCAN_EXTRAS)
    assert any(c.form and c.out_dtype == "bf16" and c.c2 and c.sums for c in WGRAD_CASES)
    plain = {(c.M, c.N, c.K, c.layout): c.key for c in CASES if c.ldc_pad == 0 and not c.accumulate and not c.det and c.bias}
    for layout in ("NN", "TN"):
        cz = [c for c in WGRAD_CASES if c.c_zeroed and not c.wgrad and c.layout == layout and c.ldc_pad == 0]
        ns = [c for c in WGRAD_CASES if c.no_split and not c.wgrad and c.layout == layout and not c.accumulate]
        assert cz and ns
        for c in cz:
            assert plain[(c.M, c.N, c.K, layout)][1:] == ("split", "zero") and c.key == (plain[(c.M, c.N, c.K, layout)][0], "split", "nozero")
        assert any(plain.get((c.M, c.N, c.K, layout), ("",))[1:] == ("split", "zero") and c.key[1:] == ("nosplit", "nozero") for c in ns)
    assert {c.status for c in WGRAD_CASES} == {0, G.UNSUPPORTED}


def test_descriptor_table_covers_every_variant_its_scan_grid_reaches():
    """Every (variant key, overwrite | accumulate) pair the selection takes anywhere on WSCAN_GRID with the extras set (TN, bf16 operands,
    lda / ldb rounded up to whole chunks, n_split = the tile width where there is a second matrix) has a case."""
    lib = L.load()
    desc, last, fold = lib.gic_debug_gemm_desc, lib.gic_debug_last_route, lib.gic_debug_wgrad_fold
    up = lambda v: (v + 7) // 8 * 8
    reached = {}
    with engine.route_only():
        for M in G.WSCAN_M:
            for N in G.WSCAN_N:
                for K in G.WSCAN_K:
                    for o_dt in ("bf16", "f32"):
                        tile = fold(P, P, M, N, K, up(M), up(N), 0, 0, L.BF16, DT[o_dt])
                        assert tile in (64, 128)
                        for sums, c2 in G.WSCAN_EXTRAS:
                            if c2 and N <= tile:
                                continue
                            for acc in (0, 1):
                                status = desc(P, P, P, M, N, K, up(M), up(N), N, 0, 0, L.BF16, DT[o_dt], P, acc, 1.0, 0, 0, 1, P if sums else None,
                                              P if sums > 1 else None, P if c2 else None, N - tile, tile if c2 else 0, None)
                                assert status == 0, (M, N, K, o_dt, sums, c2, acc)
                                key = route_key(last().decode())
                                assert len(key) == 4, (M, N, K, o_dt, sums, c2, acc, key)
                                reached.setdefault((key, acc), (M, N, K, o_dt, sums, c2))
    covered = {(c.key, c.accumulate) for c in WGRAD_CASES if not c.det}
    missing = {k: v for k, v in reached.items() if k not in covered}
    assert not missing, f"{len(missing)} of {len(reached)} variants without a case (first shape that reaches each): {missing}"
    assert len(reached) >= 60


def _emulated(case, regime, fault=None):
    from tests.test_gpu_gemm_wgrad import make_host
    host = make_host(case, regime)
    return host, G.emulate_wgrad(case, host, wroute(case)[1], fault)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.id for c in WGRAD_CASES])
def test_emulation_passes_the_checker(case):
    for regime in ("exact", "rounding"):
        host, after = _emulated(case, regime)
        ratios = G.check_wgrad(case, regime, host, after)
        assert all(r <= 1.0 for r in ratios.values())
        assert (regime == "rounding" and not case.status) == ("C" in ratios) and (regime == "rounding" and case.form and case.sums > 0) == ("a_sum" in ratios)


@pytest.mark.parametrize("regime", ["exact", "rounding"])
@pytest.mark.parametrize("fault", G.FAULTS)
def test_checker_flags_the_faults_this_form_can_have(fault, regime):
    case = {c.id: c for c in WGRAD_CASES}[G.FAULT_CASES[fault]]
    host, after = _emulated(case, regime)
    G.check_wgrad(case, regime, host, after)                          # the sound emulation passes this very case
    host, after = _emulated(case, regime, fault)
    with pytest.raises(G.Mismatch) as e:
        G.check_wgrad(case, regime, host, after)
    assert e.value.what.split(":")[0] in {"k_past_K": ("a_sum",), "split_missing": ("a_sum",), "sum2_unwritten": ("a_sum2",), "c2_tile_to_C": ("C",),
                                          "c2_not_zeroed": ("C | C2",), "tail_row": ("a_sum",)}[fault], str(e.value)


def test_checker_flags_a_fall_back_that_writes_the_sums():
    """A route without the suffix owns neither a_sum nor C2: a single changed word is a contract violation, whatever its value."""
    case = next(c for c in WGRAD_CASES if not c.form and c.sums == 2 and not c.status and c.accumulate)
    host, after = _emulated(case, "rounding")
    after["s1"][G.SUM_GUARD + 3] += 1.0
    with pytest.raises(G.Mismatch):
        G.check_wgrad(case, "rounding", host, after)
    case = next(c for c in WGRAD_CASES if c.status and c.c2)
    host, after = _emulated(case, "exact")
    after["C2"][1, 0] = 0.0
    with pytest.raises(G.Mismatch):
        G.check_wgrad(case, "exact", host, after)
