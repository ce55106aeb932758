"""Where the weight-gradient products fold their bias sums (csrc/gemm.h: GemmDesc.a_sum, wgrad_folds_a_sum / wgrad_tile_n), without a GPU.

gic_debug_wgrad_fold is the host predicate the library's own call sites consult (decoder.hip, disc.hip): the tile width of the 4-wave
kernel that folds the column sums of A into the product, or 0 where the product runs as ever and the column-sum pass stays.  The route
line of a descriptor without the new fields (everything gic_gemm can express) must not have moved: the strings below are rows of
tests/test_route.py's table."""
import pytest

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine

P = 0x7F0000010000          # a fake, 16-byte aligned, non-null device pointer: never dereferenced
BF16, F32 = L.BF16, L.F32


def fold(M, N, K, a_kc=0, b_kc=0, in_dt=BF16, out_dt=F32, A=P, B=P, lda=None, ldb=None):
    up = lambda v: (v + 7) // 8 * 8
    lda = lda if lda is not None else up(K if a_kc else M)
    ldb = ldb if ldb is not None else up(K if b_kc else N)
    return L.load().gic_debug_wgrad_fold(A, B, M, N, K, lda, ldb, a_kc, b_kc, in_dt, out_dt)


@pytest.fixture(autouse=True)
def _mode_off():
    engine.set_deterministic(False)
    yield
    engine.set_deterministic(False)


def test_the_train_steps_weight_gradients_fold():
    """cfg2's products: dW_out (128 x 128 tiles), dW_ih | dW_hh merged over xh (N = E + H), the highway's dW (split-K), and the tests' small ones."""
    assert fold(10000, 512, 1280) == 128
    assert fold(2048, 1024, 1280) == 64 and 512 % 64 == 0          # din = 512 is on a tile boundary: one launch for both matrices
    assert fold(900, 900, 8192, lda=904, ldb=904) == 64
    assert fold(160, 104, 15) == 64 and fold(160, 104, 540) == 64
    assert fold(160, 104, 15, in_dt=F32) == 0 and fold(10000, 512, 1280, in_dt=F32) == 0      # the f32 parity mode keeps its launches


def test_deterministic_mode_keeps_the_column_sum_pass():
    engine.set_deterministic(True)
    assert fold(10000, 512, 1280) == 0 and fold(2048, 1024, 1280) == 0 and fold(160, 104, 15) == 0
    engine.set_deterministic(False)
    assert fold(10000, 512, 1280) == 128


@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (1, 0), (0, 1)])
def test_k_contiguous_operands_do_not_fold(a_kc, b_kc):
    assert fold(2048, 512, 1280, a_kc, b_kc) == 0


def test_tile8_eligible_shapes_do_not_fold():
    """What the 8-wave kernel takes (wide, deep, k-contiguous, bf16): its A never passes through registers."""
    for M, N, K in ((4096, 960, 960), (8192, 960, 960)):
        with engine.route_only() as r:
            assert L.load().gic_gemm(P, P, P, M, N, K, K, K, N, 1, 1, BF16, F32, None, 1, 1.0, None) == 0
            assert r.last().startswith("tile8<")
        assert fold(M, N, K, 1, 1) == 0


def test_unaligned_operands_do_not_fold():
    assert fold(2048, 512, 1280, A=P + 2) == 0                     # A off its 16-byte alignment: the scalar path
    assert fold(2048, 512, 1280, B=P + 8) == 0
    assert fold(2048, 512, 1280, lda=2052) == 0                    # a leading dimension that is no whole 16-byte chunk
    assert fold(2048, 512, 1280, ldb=516) == 0
    assert fold(2048, 512, 1280, lda=2056) == 64                   # (8 bf16 elements per chunk)


@pytest.mark.parametrize("shape,expected", [
    ((64, 10000, 1280, 0, 0, BF16, F32, 1), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=157x3 block=256 lds=0 splits=3"),
    ((900, 900, 8192, 0, 0, BF16, F32, 1), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=225x3 block=256 lds=0 splits=3"),
    ((2048, 512, 1280, 0, 0, BF16, F32, 0), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=256x1 block=256 lds=0 splits=1"),
    ((10000, 512, 1280, 0, 0, BF16, F32, 0), "gemm<bf16,f32,false,false,128,128,true,0,false,false> grid=316x1 block=256 lds=0 splits=1"),
])
def test_route_line_without_the_new_fields_is_unchanged(shape, expected):
    M, N, K, a_kc, b_kc, in_dt, out_dt, acc = shape
    up = lambda v: (v + 7) // 8 * 8
    with engine.route_only() as r:
        assert L.load().gic_gemm(P, P, P, M, N, K, up(K if a_kc else M), up(K if b_kc else N), up(N), a_kc, b_kc, in_dt, out_dt, None, acc, 1.0, None) == 0
        line = r.last()
    assert line.startswith(expected + " per="), line
    assert "a_sum" not in line and "n_split" not in line
