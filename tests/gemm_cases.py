"""The plain GEMM kernel variants `gic_gemm` selects, one small case per variant: the table behind tests/test_gemm_cases.py (which
pins every case's route and the table's coverage without a GPU) and tests/test_gpu_gemm_matrix.py (which runs every case on the
GPU against an fp64 product).  Nothing here touches the GPU.

A case is (M, N, K, layout, in_dtype, out_dtype, accumulate, lda_pad, ldb_pad, ldc_pad, bias, alpha, key):
  layout   NT: A [M, K], B [N, K] (both k-contiguous); NN: A [M, K], B [K, N]; TN: A [K, M], B [K, N]
  *_pad    elements added to the tight leading dimension (K, M or N of the operand's contiguous axis; N for C)
  bias     whether a bias vector is passed
  key      the variant the selection must take: (the route line up to " grid=", "split" | "nosplit", "zero" | "nozero"), the last two
           from the line's splits= (> 1) and zero= (> 0) fields; a tile8 line has neither and reads as ("nosplit", "nozero")
  det      the case runs under engine.set_deterministic(True)

PER_KEY holds, for every (key, overwrite | accumulate) pair that `gic_gemm` selects anywhere on SCAN_GRID (tight leading dimensions,
bias present), the smallest shape of that grid that reaches it.  EDGES adds what the grid does not vary: K tails and C rows with live
neighbours, m- / n-contiguous tails, missing bias, rows off the tile8 grid and the deterministic mode.  A change of the selection's
thresholds has to move this table deliberately: the route test fails for every case that slid onto another kernel, the coverage test
for every variant the grid reaches that no case here does."""
from typing import NamedTuple, Tuple

SCAN_M = (5, 33, 64, 100, 128, 130, 200, 256, 520, 1000, 1024, 2048, 4096, 4224, 8192, 8200, 16512, 33024, 65792)
SCAN_N = (3, 64, 70, 72, 128, 136, 257, 264, 384, 520, 900, 904, 1000, 1024, 1152, 2048)
SCAN_K = (7, 24, 50, 64, 128, 256, 264, 320, 512, 520, 904, 1024, 2048, 4096)
LAYOUTS = {"NT": (1, 1), "NN": (1, 0), "TN": (0, 0)}              # layout -> (a_kc, b_kc)
DTYPE_PAIRS = (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"))


class Case(NamedTuple):
    M: int
    N: int
    K: int
    layout: str
    in_dtype: str
    out_dtype: str
    accumulate: int
    lda_pad: int
    ldb_pad: int
    ldc_pad: int
    bias: bool
    alpha: float
    key: Tuple[str, str, str]
    det: bool = False

    @property
    def id(self):
        pads = f"-ld+{self.lda_pad}+{self.ldb_pad}+{self.ldc_pad}" if self.lda_pad or self.ldb_pad or self.ldc_pad else ""
        return (f"{self.M}x{self.N}x{self.K}-{self.layout}-{self.in_dtype}>{self.out_dtype}-{'acc' if self.accumulate else 'ovw'}{pads}"
                f"{'' if self.bias else '-nobias'}-a{self.alpha:g}{'-det' if self.det else ''}")

    def leading_dims(self):
        a_kc, b_kc = LAYOUTS[self.layout]
        return (self.K if a_kc else self.M) + self.lda_pad, (self.K if b_kc else self.N) + self.ldb_pad, self.N + self.ldc_pad


def route_key(line):
    """The variant key of a route line (engine.route_only.last())."""
    head = line.split(" grid=")[0]
    splits = int(line.split(" splits=")[1].split()[0]) if " splits=" in line else 1
    zero = int(line.split(" zero=")[1].split()[0]) if " zero=" in line else 0
    return head, "split" if splits > 1 else "nosplit", "zero" if zero > 0 else "nozero"


def gemm_args(case, A, B, C, bias, dtypes):
    """The argument tuple of gic_gemm for `case` over the pointers given (`bias` is ignored where the case has none); `dtypes` maps
    "f32" / "bf16" to the library's dtype codes."""
    a_kc, b_kc = LAYOUTS[case.layout]
    lda, ldb, ldc = case.leading_dims()
    return (A, B, C, case.M, case.N, case.K, lda, ldb, ldc, a_kc, b_kc, dtypes[case.in_dtype], dtypes[case.out_dtype],
            bias if case.bias else None, case.accumulate, case.alpha, None)


# one case per (variant key, overwrite | accumulate) of the scan grid, ordered by shape so that neighbours share a reference product;
# alpha cycles through 1, 0.5 and -2
PER_KEY = [
    Case(5, 3, 7, "NN", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NN", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NN", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NN", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NN", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NN", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "f32", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "NT", "f32", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "f32", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<f32,f32,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 7, "TN", "f32", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<f32,f32,false,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "f32", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 24, "NT", "f32", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 3, 256, "NT", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(5, 3, 256, "NT", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(5, 3, 512, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(5, 3, 512, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(5, 3, 512, "NN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,64,64,false,0,false,false>", "split", "zero")),
    Case(5, 3, 512, "NN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,64,64,false,0,false,false>", "split", "nozero")),
    Case(5, 3, 512, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "split", "zero")),
    Case(5, 3, 512, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "split", "nozero")),
    Case(5, 3, 512, "TN", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "split", "zero")),
    Case(5, 3, 512, "TN", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "split", "nozero")),
    Case(5, 64, 24, "NN", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 24, "NN", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 24, "NN", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 24, "NN", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 24, "NN", "f32", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 24, "NN", "f32", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(5, 64, 512, "NN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,64,64,true,0,false,false>", "split", "zero")),
    Case(5, 64, 512, "NN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,64,64,true,0,false,false>", "split", "nozero")),
    Case(64, 64, 7, "TN", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 7, "TN", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 7, "TN", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 7, "TN", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 7, "TN", "f32", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<f32,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 7, "TN", "f32", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<f32,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 512, "TN", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "zero")),
    Case(64, 64, 512, "TN", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "nozero")),
    Case(2048, 3, 512, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(2048, 3, 512, "NT", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(2048, 3, 2048, "NT", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "split", "zero")),
    Case(2048, 3, 2048, "NT", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "split", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("tile8<bf16,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("tile8<bf16,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("tile8<f32,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("tile8<f32,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(8192, 72, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("tile8<bf16,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(8192, 72, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("tile8<bf16,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(8192, 72, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("tile8<f32,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(8192, 72, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("tile8<f32,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,bf16,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "f32", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NN", "f32", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "f32", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<f32,f32,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "NT", "f32", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<f32,f32,true,true,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 7, "TN", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,false,false,128,128,false,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 24, "NT", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,true,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 257, 256, "NT", "f32", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 256, "NT", "f32", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<f32,f32,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 512, "NT", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 512, "NT", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,bf16,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 512, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 512, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,true>", "nosplit", "nozero")),
    Case(8192, 257, 1024, "TN", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,128,128,false,0,false,false>", "split", "zero")),
    Case(8192, 257, 1024, "TN", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,128,128,false,0,false,false>", "split", "nozero")),
    Case(8192, 257, 2048, "NN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,false,0,false,false>", "split", "zero")),
    Case(8192, 257, 2048, "NN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,false,0,false,false>", "split", "nozero")),
    Case(8192, 257, 2048, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,true>", "split", "zero")),
    Case(8192, 257, 2048, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,true>", "split", "nozero")),
    Case(8192, 264, 7, "TN", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 7, "TN", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 7, "TN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 7, "TN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 7, "TN", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 7, "TN", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,bf16,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "f32", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 24, "NN", "f32", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<f32,f32,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8192, 264, 1024, "TN", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,128,128,true,0,false,false>", "split", "zero")),
    Case(8192, 264, 1024, "TN", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,false,false,128,128,true,0,false,false>", "split", "nozero")),
    Case(8192, 264, 2048, "NN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,true,0,false,false>", "split", "zero")),
    Case(8192, 264, 2048, "NN", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,true,false,128,128,true,0,false,false>", "split", "nozero")),
    Case(8200, 257, 4096, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,false>", "split", "zero")),
    Case(8200, 257, 4096, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,true,true,128,128,true,0,false,false>", "split", "nozero")),
    Case(16512, 72, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("tile8<bf16,64,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 72, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("tile8<bf16,64,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 72, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("tile8<f32,64,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 72, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("tile8<f32,64,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 136, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 1.0, ("tile8<bf16,128,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 136, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 1.0, ("tile8<bf16,128,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 136, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("tile8<f32,128,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(16512, 136, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, 0.5, ("tile8<f32,128,0,false,2,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 72, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, -2.0, ("tile8<bf16,64,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 72, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("tile8<bf16,64,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 72, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("tile8<f32,64,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 72, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("tile8<f32,64,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 136, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, True, 0.5, ("tile8<bf16,128,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 136, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, 0.5, ("tile8<bf16,128,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 136, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("tile8<f32,128,0,false,1,false,false,1024>", "nosplit", "nozero")),
    Case(33024, 136, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, -2.0, ("tile8<f32,128,0,false,1,false,false,1024>", "nosplit", "nozero")),
]

EDGES = [
    # K tail with live neighbours: NT, lda = ldb = K + 56 (scalar loads: K = 50, lda = ldb = 57)
    Case(130, 70, 72, "NT", "f32", "f32", 0, 56, 56, 0, True, 1.0, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(130, 70, 72, "NT", "bf16", "f32", 1, 56, 56, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(33, 70, 200, "NT", "f32", "f32", 1, 56, 56, 0, True, -2.0, ("gemm<f32,f32,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(100, 70, 904, "NT", "bf16", "bf16", 0, 56, 56, 0, True, 1.0, ("gemm<bf16,bf16,true,true,64,64,true,0,false,true>", "nosplit", "nozero")),
    Case(100, 70, 904, "NT", "bf16", "f32", 0, 56, 56, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "split", "zero")),
    Case(4096, 520, 904, "NT", "bf16", "f32", 0, 56, 56, 0, True, 1.0, ("tile8<f32,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4096, 520, 904, "NT", "bf16", "bf16", 1, 56, 56, 0, True, 0.5, ("tile8<bf16,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(33, 70, 50, "NT", "f32", "f32", 0, 7, 7, 0, True, 1.0, ("gemm<f32,f32,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(33, 70, 50, "NT", "bf16", "bf16", 1, 7, 7, 0, True, -2.0, ("gemm<bf16,bf16,true,true,64,64,false,0,false,false>", "nosplit", "nozero")),
    # padded C: ldc = N + 8 keeps the staged 16-byte stores, ldc = N + 3 drops to the direct epilogue of the same kernel
    Case(130, 72, 64, "NT", "f32", "f32", 0, 0, 0, 8, True, 1.0, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(130, 72, 64, "NT", "f32", "f32", 0, 0, 0, 3, True, 1.0, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(130, 72, 64, "NT", "bf16", "bf16", 0, 0, 0, 8, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(130, 72, 64, "NT", "bf16", "bf16", 0, 0, 0, 3, True, 0.5, ("gemm<bf16,bf16,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 512, "TN", "bf16", "f32", 0, 0, 0, 8, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "zero")),
    Case(64, 64, 512, "TN", "bf16", "f32", 0, 0, 0, 3, True, -2.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "zero")),
    Case(5, 3, 512, "NT", "bf16", "f32", 1, 0, 0, 3, True, 1.0, ("gemm<bf16,f32,true,true,64,64,true,0,false,false>", "split", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "f32", 0, 0, 0, 8, True, -2.0, ("tile8<f32,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4096, 520, 256, "NT", "bf16", "bf16", 1, 0, 0, 8, True, 1.0, ("tile8<bf16,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    # M- and N-contiguous tails: M and N off the 8 grid, lda / ldb rounded up to 8 (the tail chunk reads the row padding)
    Case(130, 70, 64, "TN", "bf16", "f32", 0, 6, 2, 0, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(130, 70, 64, "TN", "f32", "f32", 1, 6, 2, 0, True, 0.5, ("gemm<f32,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(33, 70, 64, "NN", "bf16", "bf16", 0, 0, 2, 0, True, 1.0, ("gemm<bf16,bf16,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(33, 70, 64, "NN", "f32", "f32", 0, 0, 2, 0, True, -2.0, ("gemm<f32,f32,true,false,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(8195, 261, 24, "TN", "bf16", "bf16", 1, 5, 3, 0, True, 1.0, ("gemm<bf16,bf16,false,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    Case(8195, 261, 24, "NN", "bf16", "f32", 0, 0, 3, 0, True, 0.5, ("gemm<bf16,f32,true,false,128,128,true,0,false,false>", "nosplit", "nozero")),
    # no bias, on a staged, a direct, a split and a tile8 route
    Case(130, 72, 64, "NT", "f32", "f32", 0, 0, 0, 0, False, 0.5, ("gemm<f32,f32,true,true,64,64,true,0,false,false>", "nosplit", "nozero")),
    Case(33, 70, 50, "NN", "bf16", "f32", 1, 0, 0, 0, False, -2.0, ("gemm<bf16,f32,true,false,64,64,false,0,false,false>", "nosplit", "nozero")),
    Case(64, 64, 512, "TN", "bf16", "f32", 0, 0, 0, 0, False, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "zero")),
    Case(8232, 72, 256, "NT", "bf16", "bf16", 0, 0, 0, 0, False, 0.5, ("tile8<bf16,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    # tile8 with M off the 128 grid, one per BN
    Case(8232, 72, 256, "NT", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("tile8<f32,64,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4136, 520, 256, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("tile8<f32,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    Case(4136, 520, 256, "NT", "bf16", "bf16", 1, 0, 0, 0, True, -2.0, ("tile8<bf16,128,0,false,4,false,false,1024>", "nosplit", "nozero")),
    # the train step's split-K products, and again in deterministic mode (two splits onto a zeroed C at the most, none onto a live C)
    Case(64, 64, 512, "TN", "bf16", "f32", 0, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "split", "zero"), det=True),
    Case(64, 64, 512, "TN", "bf16", "f32", 1, 0, 0, 0, True, 1.0, ("gemm<bf16,f32,false,false,64,64,true,0,false,false>", "nosplit", "nozero"), det=True),
    Case(1280, 64, 10000, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "split", "zero")),
    Case(1280, 64, 10000, "NT", "bf16", "f32", 0, 0, 0, 0, True, 0.5, ("gemm<bf16,f32,true,true,64,64,true,0,false,true>", "split", "zero"), det=True),
    Case(100, 900, 4096, "TN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "split", "zero")),
    Case(100, 900, 4096, "TN", "bf16", "f32", 0, 0, 0, 0, True, -2.0, ("gemm<bf16,f32,false,false,64,64,false,0,false,false>", "split", "zero"), det=True),
]

CASES = PER_KEY + EDGES
