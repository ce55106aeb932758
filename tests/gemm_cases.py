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
for every variant the grid reaches that no case here does.

WGRAD_CASES is the second table: descriptors `gic_gemm` cannot express, run through gic_debug_gemm_desc (gicap.h) by
tests/test_gpu_gemm_wgrad.py.  They carry the fields only the library's own call sites set:
  c_zeroed, no_split   GemmDesc's flags of the same names
  wgrad                the descriptor says that the weight-gradient extras follow (gemm.h)
  sums                 0: no a_sum; 1: a_sum; 2: a_sum and a_sum2
  c2, n_split, ldc2_pad   a second output matrix for the columns from n_split on, ldc2 = N - n_split + ldc2_pad
  status               what gemm() must answer (0 or GIC_STATUS_UNSUPPORTED = -2: nothing may be written)
  misalign             "A" | "B": that operand starts one element off its 16-byte alignment
A key of four components is a route line that ends in " a_sum=<0|1|2> n_split=<n>": the product ran in the weight-gradient form
(EPI_WGRAD, gemm.hip); a key of three is a line without it: a_sum / a_sum2 / C2 must not be touched.  WGRAD_PER_KEY holds the smallest
shape of WSCAN_GRID (TN, bf16 operands, lda / ldb rounded up to whole 16-byte chunks, every combination of WSCAN_EXTRAS, n_split = the
tile width) per (key, overwrite | accumulate); WGRAD_EDGES adds the train step's shapes, the tails, the caller-only flags, the
fall-backs and the refusals.  emulate_wgrad / FAULTS / check_wgrad below are the form's epilogue in plain numpy, what it can get wrong,
and the checker both the GPU test and the self-test without a GPU (tests/test_gemm_cases.py) hold an output to."""
from typing import NamedTuple, Tuple

import numpy as np
import torch

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
    key: Tuple[str, ...]
    det: bool = False
    # what only gic_debug_gemm_desc reaches (module docstring)
    c_zeroed: bool = False
    no_split: bool = False
    wgrad: bool = False
    sums: int = 0
    c2: bool = False
    n_split: int = 0
    ldc2_pad: int = 0
    status: int = 0
    misalign: str = ""

    @property
    def id(self):
        pads = f"-ld+{self.lda_pad}+{self.ldb_pad}+{self.ldc_pad}" if self.lda_pad or self.ldb_pad or self.ldc_pad else ""
        extras = (("-cz" if self.c_zeroed else "") + ("-nosplit" if self.no_split else "") + ("-wg" if self.wgrad else "")
                  + (f"-s{self.sums}" if self.sums else "") + (f"-c2@{self.n_split}+{self.ldc2_pad}" if self.c2 else "")
                  + (f"-mis{self.misalign}" if self.misalign else "") + (f"-st{self.status}" if self.status else ""))
        return (f"{self.M}x{self.N}x{self.K}-{self.layout}-{self.in_dtype}>{self.out_dtype}-{'acc' if self.accumulate else 'ovw'}{pads}"
                f"{'' if self.bias else '-nobias'}-a{self.alpha:g}{'-det' if self.det else ''}{extras}")

    @property
    def ldc2(self):
        return max(self.N - self.n_split, 1) + self.ldc2_pad

    @property
    def form(self):
        """The case runs in the weight-gradient form (its key has the route line's a_sum= / n_split= suffix)."""
        return len(self.key) == 4

    def leading_dims(self):
        a_kc, b_kc = LAYOUTS[self.layout]
        return (self.K if a_kc else self.M) + self.lda_pad, (self.K if b_kc else self.N) + self.ldb_pad, self.N + self.ldc_pad


def route_key(line):
    """The variant key of a route line (engine.route_only.last()); a line of the weight-gradient form has a fourth component, its
    "a_sum=<0|1|2> n_split=<n>" suffix."""
    head = line.split(" grid=")[0]
    splits = int(line.split(" splits=")[1].split()[0]) if " splits=" in line else 1
    zero = int(line.split(" zero=")[1].split()[0]) if " zero=" in line else 0
    key = head, "split" if splits > 1 else "nosplit", "zero" if zero > 0 else "nozero"
    return key + (line[line.index(" a_sum=") + 1:],) if " a_sum=" in line else key


def gemm_args(case, A, B, C, bias, dtypes):
    """The argument tuple of gic_gemm for `case` over the pointers given (`bias` is ignored where the case has none); `dtypes` maps
    "f32" / "bf16" to the library's dtype codes."""
    a_kc, b_kc = LAYOUTS[case.layout]
    lda, ldb, ldc = case.leading_dims()
    return (A, B, C, case.M, case.N, case.K, lda, ldb, ldc, a_kc, b_kc, dtypes[case.in_dtype], dtypes[case.out_dtype],
            bias if case.bias else None, case.accumulate, case.alpha, None)


def desc_args(case, A, B, C, bias, dtypes, a_sum, a_sum2, C2):
    """The argument tuple of gic_debug_gemm_desc for `case` over the pointers given (a_sum / a_sum2 / C2 are ignored where the case has
    none)."""
    return gemm_args(case, A, B, C, bias, dtypes)[:-1] + (
        int(case.c_zeroed), int(case.no_split), int(case.wgrad), a_sum if case.sums >= 1 else None, a_sum2 if case.sums >= 2 else None,
        C2 if case.c2 else None, case.ldc2, case.n_split, None)


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


# ------------------------------------------------------------------------------------------ the descriptors gic_gemm cannot express
WSCAN_M = (5, 64, 100, 128, 160, 900, 1024, 2048, 3072, 4096)
WSCAN_N = (64, 104, 128, 256, 904, 1024)
WSCAN_K = (7, 15, 64, 200, 540, 1024, 2048, 8192)
WSCAN_EXTRAS = ((1, False), (2, False), (0, True), (1, True), (2, True))          # (sums, c2)
UNSUPPORTED = -2                                                                   # GIC_STATUS_UNSUPPORTED
REFUSED = ("unsupported", "nosplit", "nozero")                                     # route_key("unsupported")


def _wkey(layout, in_dtype, out_dtype, tile, vec, split, zero, suffix=None):
    b = lambda v: "true" if v else "false"
    a_kc, b_kc = LAYOUTS[layout]
    key = (f"gemm<{in_dtype},{out_dtype},{b(a_kc)},{b(b_kc)},{tile},{tile},{b(vec)},0,false,false>", split, zero)
    return key if suffix is None else key + (suffix,)


def _w(M, N, K, out_dtype, acc, alpha, tile, split, zero, sums=0, n_split=0, form=True, layout="TN", in_dtype="bf16", vec=True, wgrad=True, **kw):
    """A row of the second table: the key is spelled by its parts (tile width, split, zero fill and, with `form`, the a_sum= / n_split=
    suffix); m- / n-contiguous leading dimensions are rounded up to 8 elements unless given; a second output matrix where n_split > 0."""
    a_kc, b_kc = LAYOUTS[layout]
    c2 = kw.pop("c2", n_split > 0)
    lda_pad, ldb_pad = kw.pop("lda_pad", 0 if a_kc else -M % 8), kw.pop("ldb_pad", 0 if b_kc else -N % 8)
    key = _wkey(layout, in_dtype, out_dtype, tile, vec, split, zero, f"a_sum={sums} n_split={n_split if c2 else 0}" if form else None)
    if kw.get("status", 0):
        key = REFUSED
    return Case(M, N, K, layout, in_dtype, out_dtype, acc, lda_pad, ldb_pad, kw.pop("ldc_pad", 0), kw.pop("bias", True), alpha, key,
                wgrad=wgrad, sums=sums, c2=c2, n_split=n_split, **kw)


# one case per (variant key, overwrite | accumulate) of WSCAN_GRID x WSCAN_EXTRAS, in scan order; alpha cycles through 1, 0.5 and -2
WGRAD_PER_KEY = [
    _w(5, 64, 7, "bf16", 0, 1.0, 64, "nosplit", "nozero", sums=1),
    _w(5, 64, 7, "bf16", 1, 1.0, 64, "nosplit", "nozero", sums=1),
    _w(5, 64, 7, "bf16", 0, 0.5, 64, "nosplit", "nozero", sums=2),
    _w(5, 64, 7, "bf16", 1, 0.5, 64, "nosplit", "nozero", sums=2),
    _w(5, 64, 7, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=1),
    _w(5, 64, 7, "f32", 1, -2.0, 64, "nosplit", "nozero", sums=1),
    _w(5, 64, 7, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2),
    _w(5, 64, 7, "f32", 1, 1.0, 64, "nosplit", "nozero", sums=2),
    _w(5, 64, 540, "f32", 0, 0.5, 64, "split", "zero", sums=1),
    _w(5, 64, 540, "f32", 1, 0.5, 64, "split", "nozero", sums=1),
    _w(5, 64, 540, "f32", 0, -2.0, 64, "split", "zero", sums=2),
    _w(5, 64, 540, "f32", 1, -2.0, 64, "split", "nozero", sums=2),
    _w(5, 104, 7, "bf16", 0, 1.0, 64, "nosplit", "nozero", sums=0, n_split=64),
    _w(5, 104, 7, "bf16", 1, 1.0, 64, "nosplit", "nozero", sums=0, n_split=64),
    _w(5, 104, 7, "bf16", 0, 0.5, 64, "nosplit", "nozero", sums=1, n_split=64),
    _w(5, 104, 7, "bf16", 1, 0.5, 64, "nosplit", "nozero", sums=1, n_split=64),
    _w(5, 104, 7, "bf16", 0, -2.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    _w(5, 104, 7, "bf16", 1, -2.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    _w(5, 104, 7, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=0, n_split=64),
    _w(5, 104, 7, "f32", 1, 1.0, 64, "nosplit", "nozero", sums=0, n_split=64),
    _w(5, 104, 7, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=1, n_split=64),
    _w(5, 104, 7, "f32", 1, 0.5, 64, "nosplit", "nozero", sums=1, n_split=64),
    _w(5, 104, 7, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    _w(5, 104, 7, "f32", 1, -2.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    _w(5, 104, 540, "f32", 0, 1.0, 64, "split", "zero", sums=0, n_split=64),
    _w(5, 104, 540, "f32", 1, 1.0, 64, "split", "nozero", sums=0, n_split=64),
    _w(5, 104, 540, "f32", 0, 0.5, 64, "split", "zero", sums=1, n_split=64),
    _w(5, 104, 540, "f32", 1, 0.5, 64, "split", "nozero", sums=1, n_split=64),
    _w(5, 104, 540, "f32", 0, -2.0, 64, "split", "zero", sums=2, n_split=64),
    _w(5, 104, 540, "f32", 1, -2.0, 64, "split", "nozero", sums=2, n_split=64),
    # the 128 x 128 tile: at least 192 of them (24 x 8; N = 904 leaves the last column tile 8 wide), split from 16 K tiles on
    _w(3072, 904, 7, "bf16", 0, 1.0, 128, "nosplit", "nozero", sums=1),
    _w(3072, 904, 7, "bf16", 1, 1.0, 128, "nosplit", "nozero", sums=1),
    _w(3072, 904, 7, "bf16", 0, 0.5, 128, "nosplit", "nozero", sums=2),
    _w(3072, 904, 7, "bf16", 1, 0.5, 128, "nosplit", "nozero", sums=2),
    _w(3072, 904, 7, "bf16", 0, -2.0, 128, "nosplit", "nozero", sums=0, n_split=128),
    _w(3072, 904, 7, "bf16", 1, -2.0, 128, "nosplit", "nozero", sums=0, n_split=128),
    _w(3072, 904, 7, "bf16", 0, 1.0, 128, "nosplit", "nozero", sums=1, n_split=128),
    _w(3072, 904, 7, "bf16", 1, 1.0, 128, "nosplit", "nozero", sums=1, n_split=128),
    _w(3072, 904, 7, "bf16", 0, 0.5, 128, "nosplit", "nozero", sums=2, n_split=128),
    _w(3072, 904, 7, "bf16", 1, 0.5, 128, "nosplit", "nozero", sums=2, n_split=128),
    _w(3072, 904, 7, "f32", 0, -2.0, 128, "nosplit", "nozero", sums=1),
    _w(3072, 904, 7, "f32", 1, -2.0, 128, "nosplit", "nozero", sums=1),
    _w(3072, 904, 7, "f32", 0, 1.0, 128, "nosplit", "nozero", sums=2),
    _w(3072, 904, 7, "f32", 1, 1.0, 128, "nosplit", "nozero", sums=2),
    _w(3072, 904, 7, "f32", 0, 0.5, 128, "nosplit", "nozero", sums=0, n_split=128),
    _w(3072, 904, 7, "f32", 1, 0.5, 128, "nosplit", "nozero", sums=0, n_split=128),
    _w(3072, 904, 7, "f32", 0, -2.0, 128, "nosplit", "nozero", sums=1, n_split=128),
    _w(3072, 904, 7, "f32", 1, -2.0, 128, "nosplit", "nozero", sums=1, n_split=128),
    _w(3072, 904, 7, "f32", 0, 1.0, 128, "nosplit", "nozero", sums=2, n_split=128),
    _w(3072, 904, 7, "f32", 1, 1.0, 128, "nosplit", "nozero", sums=2, n_split=128),
    _w(3072, 904, 1024, "f32", 0, 0.5, 128, "split", "zero", sums=1),
    _w(3072, 904, 1024, "f32", 1, 0.5, 128, "split", "nozero", sums=1),
    _w(3072, 904, 1024, "f32", 0, -2.0, 128, "split", "zero", sums=2),
    _w(3072, 904, 1024, "f32", 1, -2.0, 128, "split", "nozero", sums=2),
    _w(3072, 904, 1024, "f32", 0, 1.0, 128, "split", "zero", sums=0, n_split=128),
    _w(3072, 904, 1024, "f32", 1, 1.0, 128, "split", "nozero", sums=0, n_split=128),
    _w(3072, 904, 1024, "f32", 0, 0.5, 128, "split", "zero", sums=1, n_split=128),
    _w(3072, 904, 1024, "f32", 1, 0.5, 128, "split", "nozero", sums=1, n_split=128),
    _w(3072, 904, 1024, "f32", 0, -2.0, 128, "split", "zero", sums=2, n_split=128),
    _w(3072, 904, 1024, "f32", 1, -2.0, 128, "split", "nozero", sums=2, n_split=128),
]

WGRAD_EDGES = [
    # the decoder tests' dW_ih | dW_hh: one ragged K tile; nine K tiles split three ways over the zero fill, and onto a live C
    _w(160, 104, 15, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    _w(160, 104, 540, "f32", 0, 0.5, 64, "split", "zero", sums=2, n_split=64),
    _w(160, 104, 540, "f32", 1, -2.0, 64, "split", "nozero", sums=2, n_split=64),
    # K = 0 in the form: the sums are the empty sum too
    _w(160, 104, 0, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2, n_split=64),
    # tails: M = 132 (lda = 136) and N = 140 (ldb = 144) off the 8 grid, K = 200 over four K tiles, N - n_split = 12 columns of C2 with
    # ldc2 = 16 (C2 staged like C), and ldc2 = 15 (C2's tile takes the direct epilogue, C's the staged one); the same onto a bf16 C
    _w(132, 140, 200, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2, n_split=128, ldc2_pad=4),
    _w(132, 140, 200, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=1, n_split=128, ldc2_pad=3),
    _w(132, 140, 200, "f32", 1, -2.0, 64, "nosplit", "nozero", sums=2, n_split=128, ldc2_pad=3, ldc_pad=3),
    _w(132, 136, 200, "bf16", 0, 1.0, 64, "nosplit", "nozero", sums=2, n_split=128, ldc2_pad=5),
    _w(131, 141, 200, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=1, n_split=64, ldc2_pad=3),
    # the highway's dW: 900 x 900 with lda = ldb = 904 (225 tiles of 64 x 64); N - n_split = 4 columns with ldc2 = 7; and at K = 4096
    # split three ways onto a live gradient (the tiles <= 320 && nk >= 64 branch: its column sums are atomics onto a live hw_b)
    _w(900, 900, 200, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=1, n_split=896, ldc2_pad=3),
    _w(900, 900, 4096, "f32", 1, 1.0, 64, "split", "nozero", sums=1),
    # no_split: that shape, and the skinny products of PER_KEY that split by default, with and without the extras
    _w(900, 900, 4096, "f32", 1, 1.0, 64, "nosplit", "nozero", sums=1, no_split=True),
    _w(900, 900, 4096, "f32", 1, 0.5, 64, "nosplit", "nozero", form=False, wgrad=False, no_split=True),
    _w(5, 64, 512, "f32", 0, -2.0, 64, "nosplit", "nozero", form=False, wgrad=False, no_split=True, layout="NN"),
    _w(64, 64, 512, "f32", 0, 1.0, 64, "nosplit", "nozero", form=False, wgrad=False, no_split=True),
    _w(64, 64, 512, "f32", 1, 1.0, 64, "nosplit", "nozero", form=False, wgrad=False, no_split=True),
    _w(64, 64, 512, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=2, no_split=True),
    # c_zeroed: the same two products add their splits onto the caller's zero C, without the zero fill
    _w(5, 64, 512, "f32", 0, -2.0, 64, "split", "nozero", form=False, wgrad=False, c_zeroed=True, layout="NN"),
    _w(64, 64, 512, "f32", 0, 1.0, 64, "split", "nozero", form=False, wgrad=False, c_zeroed=True),
    _w(64, 64, 512, "f32", 0, 1.0, 64, "split", "nozero", form=False, wgrad=False, c_zeroed=True, ldc_pad=3),
    # fall-backs: a_sum / a_sum2 alone where the form is not taken: status 0, the plain route line, the sums untouched.  f32 operands,
    # a k-contiguous A, A / B off their alignment, lda / ldb no whole chunks, c_zeroed (split and not), the deterministic mode (split
    # in two over the zero fill, and not), and a descriptor that does not say `wgrad`
    _w(160, 104, 15, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2, form=False, in_dtype="f32"),
    _w(160, 104, 15, "f32", 1, 0.5, 64, "nosplit", "nozero", sums=2, form=False, layout="NN", vec=False),
    _w(160, 104, 15, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=2, form=False, vec=False, misalign="A"),
    _w(160, 104, 15, "f32", 1, 1.0, 64, "nosplit", "nozero", sums=2, form=False, vec=False, misalign="B"),
    _w(160, 104, 15, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=2, form=False, vec=False, lda_pad=4),
    _w(160, 104, 15, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=1, form=False, vec=False, ldb_pad=4),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "nosplit", "nozero", sums=2, form=False, c_zeroed=True),
    _w(64, 64, 512, "f32", 0, 0.5, 64, "split", "nozero", sums=2, form=False, c_zeroed=True),
    _w(160, 104, 15, "f32", 0, -2.0, 64, "nosplit", "nozero", sums=2, form=False, det=True),
    _w(64, 64, 512, "f32", 0, 1.0, 64, "split", "zero", sums=2, form=False, det=True),
    _w(160, 104, 15, "f32", 0, 0.5, 64, "nosplit", "nozero", sums=2, n_split=64, form=False, wgrad=False),
    # refusals: a second output matrix that the selection cannot honour.  n_split off the tile boundary (64 under the 128 tile too),
    # at 0 and at N; then each of the conditions above
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=32, status=UNSUPPORTED),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=0, c2=True, status=UNSUPPORTED),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=104, status=UNSUPPORTED),
    _w(3072, 904, 7, "f32", 0, 1.0, 128, "", "", sums=1, n_split=64, status=UNSUPPORTED),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", sums=2, n_split=64, status=UNSUPPORTED, in_dtype="f32"),
    _w(160, 104, 15, "f32", 1, 1.0, 64, "", "", n_split=64, status=UNSUPPORTED, layout="NN"),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=64, status=UNSUPPORTED, misalign="A"),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=64, status=UNSUPPORTED, misalign="B"),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=64, status=UNSUPPORTED, lda_pad=4),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", n_split=64, status=UNSUPPORTED, ldb_pad=4),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", sums=1, n_split=64, status=UNSUPPORTED, c_zeroed=True),
    _w(160, 104, 15, "f32", 0, 1.0, 64, "", "", sums=2, n_split=64, status=UNSUPPORTED, det=True),
]

WGRAD_CASES = WGRAD_PER_KEY + WGRAD_EDGES


# ------------------------------------------------------------------------------------------ the form's epilogue in plain numpy
# What a run works on, `host` (tests/test_gpu_gemm_wgrad.py make_host builds it; CPU tensors):
#   A, B          the operands as the kernel addresses them, padding and the k rows past K included
#   C, C2         [M + 2, ld] with a guard row on either side; s1, s2: [SUM_GUARD + M + SUM_GUARD] (a_sum, a_sum2); None where absent
#   ref           fp64: A [M, K], B [N, K], bias [N] | None, C0 [M, N], s0 [M], P = A B^T, absP = |A| |B|^T | None
# and what it leaves, `after`: C, C2, s1, s2 again.
SUM_GUARD = 8
U_F32, U_BF16 = 2.0 ** -24, 2.0 ** -8
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
FAULTS = ("k_past_K", "split_missing", "sum2_unwritten", "c2_tile_to_C", "c2_not_zeroed", "tail_row")


class Mismatch(AssertionError):
    def __init__(self, case, regime, what, index, detail):
        self.case, self.regime, self.what, self.index = case, regime, what, index
        super().__init__(f"{case.id} {regime}: {what}: first at {index}: {detail}")


def plan_of(line):
    """(tile width, splits, K tiles per split, zero fill) of a 4-wave route line."""
    tile = int(line.split("<")[1].split(">")[0].split(",")[4])
    return tile, int(line.split(" splits=")[1].split()[0]), int(line.split(" per=")[1].split()[0]), int(line.split(" zero=")[1].split()[0]) > 0


def emulate_wgrad(case, host, line, fault=None):
    """What the launch `line` plans leaves in C, C2, a_sum and a_sum2, in f32 numpy: per split s the K tiles [s per, (s + 1) per) clipped
    to K; the column tiles from n_split on go to C2; the workgroups of the first column tile own a_sum, each the rows of its row tile;
    a split launch starts from a zero fill of all four (overwrite), from the live values (accumulate) or from the caller's zero C
    (c_zeroed) and adds split by split, an unsplit one stores or adds once.  A product outside the form is the plain product and
    leaves the sums and C2 alone; a refused one leaves everything.  `fault`: one of FAULTS."""
    after = {k: (None if host[k] is None else host[k].clone()) for k in ("C", "C2", "s1", "s2")}
    if case.status:
        return after
    M, N, K = case.M, case.N, case.K
    tile, splits, per, zero = plan_of(line)
    form = " a_sum=" in line
    bk = 64 if case.in_dtype == "bf16" else 32
    A, B = host["ref"]["A"].numpy().astype(np.float32), host["ref"]["B"].numpy().astype(np.float32)
    bias = host["ref"]["bias"].numpy().astype(np.float32) if case.bias else np.zeros(N, np.float32)
    two = form and case.c2
    ns = case.n_split if two else N
    live = np.concatenate([after["C"][1:M + 1, :ns].float().numpy()] + ([after["C2"][1:M + 1, :N - ns].float().numpy()] if two else []), axis=1)
    sums = [after[k][SUM_GUARD:SUM_GUARD + M].numpy().copy() for k in ("s1", "s2")[:case.sums]] if form else []
    if fault == "sum2_unwritten":
        sums = sums[:1]
    if zero:
        live[:, :ns] = 0.0
        if fault != "c2_not_zeroed":
            live[:, ns:] = 0.0
        for s in sums:
            s[:] = 0.0
    alpha = np.float32(case.alpha)
    for s in range(splits):
        k0, k1 = min(K, s * per * bk), min(K, (s + 1) * per * bk)
        v = alpha * (A[:, k0:k1] @ B[:, k0:k1].T) + (bias if s == 0 else np.float32(0.0))
        if splits > 1:
            live += v
        else:
            live = v + live if case.accumulate else v
        if not sums or (fault == "split_missing" and s == splits - 1 and splits > 1):
            continue
        t = A[:, k0:k1].sum(1, dtype=np.float32)
        st = host["A"].float().numpy()                   # [k rows, lda]: the k rows past K and the row padding behind M are in it
        if fault == "k_past_K" and s == splits - 1:      # the last K tile is staged whole
            t = t + st[K:(s + 1) * per * bk, :M].sum(0, dtype=np.float32)
        if fault == "tail_row" and M % 8:                # the tail chunk's first padding row lands in the last row's slot
            t[M - 1] += st[k0:k1, M].sum(dtype=np.float32)
        for dst in sums:
            if splits > 1:
                dst += t
            else:
                dst[:] = t + dst if case.accumulate else t
    out_td = after["C"].dtype
    after["C"][1:M + 1, :ns] = torch.from_numpy(live[:, :ns]).to(out_td)
    if two and fault == "c2_tile_to_C":                  # the first tile past n_split keeps C's base pointer
        w = min(tile, N - ns)
        after["C"][1:M + 1, ns:ns + w] = torch.from_numpy(live[:, ns:ns + w]).to(out_td)
        after["C2"][1:M + 1, w:N - ns] = torch.from_numpy(live[:, ns + w:]).to(out_td)
    elif two:
        after["C2"][1:M + 1, :N - ns] = torch.from_numpy(live[:, ns:]).to(out_td)
    for k, s in zip(("s1", "s2"), sums):
        after[k][SUM_GUARD:SUM_GUARD + M] = torch.from_numpy(s)
    return after


def _first(mask):
    return tuple(int(i) for i in torch.nonzero(mask)[0])


def _same_bits(case, regime, what, before, got, live=None):
    """Every element outside `live` (a boolean mask, None: no element is live) keeps its bits, NaN included."""
    changed = before.view(BITS[before.dtype]) != got.view(BITS[got.dtype])
    if live is not None:
        changed = changed & ~live
    if bool(changed.any()):
        i = _first(changed)
        raise Mismatch(case, regime, f"{what}: {int(changed.sum())} elements outside the live part changed", i, f"{before[i].item()!r} -> {got[i].item()!r}")


def _held(case, regime, what, got, ref, bound):
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    over = err > bound
    if bool(over.any()):
        i = _first(over)
        raise Mismatch(case, regime, f"{what}: {int(over.sum())} of {over.numel()} elements beyond the bound", i,
                       f"got {got[i].item()!r}, ref {ref[i].item()!r}, bound {bound[i].item()!r}")
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def _bit_equal(case, regime, what, got, want):
    differ = got.view(BITS[got.dtype]) != want.view(BITS[want.dtype])
    if bool(differ.any()):
        i = _first(differ)
        raise Mismatch(case, regime, f"{what}: {int(differ.sum())} of {differ.numel()} elements are not bit-identical to the reference", i,
                       f"got {got[i].item()!r}, want {want[i].item()!r}")


def check_wgrad(case, regime, host, after):
    """Hold what a run left to the contract (tests/test_gpu_gemm_wgrad.py's docstring): guards, padding and whatever the route does not
    own keep their bits; C | C2 and the sums are bit-identical to the fp64 reference in the exact regime and within the derived bounds
    in the rounding regime.  Raises Mismatch naming the first element; returns err / bound maxima {"C": .., "a_sum": ..} (rounding)."""
    M, N, K, ref = case.M, case.N, case.K, host["ref"]
    two = case.form and case.c2 and not case.status
    ns = case.n_split if two else N
    wrote_sums = case.form and not case.status

    def rows(buf, cols):
        m = torch.zeros(buf.shape, dtype=torch.bool)
        m[1:M + 1, :cols] = True
        return m

    _same_bits(case, regime, "C", host["C"], after["C"], None if case.status else rows(host["C"], ns))
    if host["C2"] is not None:
        _same_bits(case, regime, "C2", host["C2"], after["C2"], rows(host["C2"], N - ns) if two else None)
    for k, name in (("s1", "a_sum"), ("s2", "a_sum2")):
        if host[k] is not None:
            m = torch.zeros(host[k].shape, dtype=torch.bool)
            m[SUM_GUARD:SUM_GUARD + M] = True
            _same_bits(case, regime, name, host[k], after[k], m if wrote_sums else None)
    if case.status:
        return {}
    got = torch.cat([after["C"][1:M + 1, :ns]] + ([after["C2"][1:M + 1, :N - ns]] if two else []), dim=1)
    out_td = got.dtype
    bias = ref["bias"] if case.bias else torch.zeros(N, dtype=torch.float64)
    C0 = ref["C0"] if case.accumulate else torch.zeros(M, N, dtype=torch.float64)
    want = case.alpha * ref["P"] + bias + C0
    s_want = ref["A"].sum(1) + (ref["s0"] if case.accumulate else 0.0)
    s_got = [after[k][SUM_GUARD:SUM_GUARD + M] for k in ("s1", "s2")[:case.sums]] if wrote_sums else []
    ratios = {}
    if regime == "exact":
        assert 9 * K * abs(case.alpha) < 2 ** 24
        if out_td == torch.bfloat16 and case.accumulate:
            _held(case, regime, "C | C2", got, want, U_BF16 * want.abs())
        else:
            _bit_equal(case, regime, "C | C2", got, want.float().to(out_td))
        for name, s in zip(("a_sum", "a_sum2"), s_got):
            _bit_equal(case, regime, name, s, s_want.float())
        if len(s_got) == 2:
            _bit_equal(case, regime, "a_sum2 against a_sum", s_got[1], s_got[0])
        return ratios
    bound = (K + 4) * U_F32 * (abs(case.alpha) * ref["absP"] + bias.abs() + C0.abs())
    if out_td == torch.bfloat16:
        bound = bound + (2 * U_BF16 * (want.abs() + C0.abs()) if case.accumulate else U_BF16 * want.abs())
    ratios["C"] = _held(case, regime, "C | C2", got, want, bound)
    s_bound = (K + 4) * U_F32 * (ref["A"].abs().sum(1) + (ref["s0"].abs() if case.accumulate else 0.0))
    for name, s in zip(("a_sum", "a_sum2"), s_got):
        ratios["a_sum"] = max(ratios.get("a_sum", 0.0), _held(case, regime, name, s, s_want, s_bound))
    return ratios


# the case (of WGRAD_CASES, by id) on which each seeded fault must fail the checker
FAULT_CASES = {
    "k_past_K": "160x104x15-TN-bf16>f32-ovw-a1-wg-s2-c2@64+0",
    "split_missing": "160x104x540-TN-bf16>f32-ovw-a0.5-wg-s2-c2@64+0",
    "sum2_unwritten": "160x104x15-TN-bf16>f32-ovw-a1-wg-s2-c2@64+0",
    "c2_tile_to_C": "160x104x15-TN-bf16>f32-ovw-a1-wg-s2-c2@64+0",
    "c2_not_zeroed": "160x104x540-TN-bf16>f32-ovw-a0.5-wg-s2-c2@64+0",
    "tail_row": "132x140x200-TN-bf16>f32-ovw-ld+4+4+0-a1-wg-s2-c2@128+4",
}
