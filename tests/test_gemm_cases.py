"""The GEMM case table (tests/gemm_cases.py) against the selection, without a GPU: every case takes the variant it names, the table
reaches every variant the scan grid reaches, and K = 0 selects (it used to divide by zero on the host).  Route-only mode as in
tests/test_route.py: the pointers are fake, 16-byte aligned and never dereferenced."""
import pytest

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine
from tests.gemm_cases import CASES, DTYPE_PAIRS, LAYOUTS, SCAN_K, SCAN_M, SCAN_N, gemm_args, route_key

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
    ids = [c.id for c in CASES]
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
