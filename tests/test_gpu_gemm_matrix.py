"""Every plain GEMM kernel variant `gic_gemm` selects (tests/gemm_cases.py), element by element against an fp64 product on the CPU.

Each case asserts its route with the real pointers before it launches, and then runs two data regimes:

  exact     A, B, bias and C0 are integers in [-3, 3] and alpha is +-2^j, so every partial sum is an integer multiple of |alpha| below
            2^24 in magnitude (9 * 10000 * 2 < 2^24): the f32 result is exact under any summation order, split-K atomics and both
            MFMA paths included.  f32 output and bf16 overwrite must be bit-identical to the cast reference; bf16 accumulate must
            lie within 2^-8 |ref|.  Nothing is fitted: a dropped, duplicated or misplaced K element, tile, split or zero fill changes
            an integer.
  rounding  Gaussian operands rounded to the input dtype before the reference is formed.  Per element, the worst-case bound of an
            f32 dot product in any order (Higham, gamma_K ~ K u):
                |got - ref| <= (K + 4) 2^-24 (|alpha| (|A| |B|^T) + |bias| + |C0|) + r
            r = 0 (f32 output), 2^-8 |ref| (bf16 overwrite), 2 * 2^-8 (|ref| + |C0|) (bf16 accumulate).  Derived, not measured: it is
            there to catch lost precision (a bf16 accumulator, f32 operands truncated to bf16) and bites at K <= 512.

Buffers: A, B and C carry their padded leading dimensions.  Padding the contract says is never read holds NaN, and so does the m- / n-
contiguous row padding that a tail chunk reads but that feeds only rows never stored (gemm.hip, gemm()); in the rounding regime the
padding behind a K tail holds ordinary numbers instead (the decoder's XH[:, Din:] operands).  In overwrite mode the live part of C is
NaN beforehand (overwrite must not read C).  C's padding columns and a guard row before and after it hold a sentinel whose bits must
not change.

Largest err / bound seen per route family in the rounding regime (MI355X; overwrite / accumulate; the bound is NOT tightened to
these; the module prints the table again after every run under -s):
                     f32>f32          bf16>f32         bf16>bf16
  gemm scalar        0.383 / 0.378    0.171 / 0.197    0.996 / 0.498
  gemm vec           0.372 / 0.342    0.171 / 0.202    0.996 / 0.496
  gemm ring          0.023 / 0.022    0.004 / 0.004    0.960 / 0.486
  gemm split (any)                    0.001 / 0.001
  tile8                               0.009 / 0.009    0.978 / 0.492
(bf16 output: the bound is dominated by r, half a bf16 ulp is up to 2^-8 |ref|, so a correctly rounded result reaches ~1 in overwrite
mode and ~0.5 under accumulate's doubled r.)"""
import functools

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests.gemm_cases import CASES, LAYOUTS, gemm_args, route_key

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "bf16": torch.bfloat16}
DT = {"f32": L.F32, "bf16": L.BF16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SENTINEL = 1232.0          # exact in bf16 and f32
U_F32, U_BF16 = 2.0 ** -24, 2.0 ** -8

# err / bound maxima of the rounding regime, per family (kernel, in dtype, out dtype, mode): recorded, never asserted against
MAXIMA = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def _report_maxima():
    yield
    for fam in sorted(MAXIMA):
        print(f"\n[gemm matrix] err/bound max {MAXIMA[fam]:.4f}  {fam}", end="")
    print()


@functools.lru_cache(maxsize=2)
def operands(M, N, K, in_dtype, regime):
    """Logical A [M, K], B [N, K], bias [N], C0 [M, N] in fp64 (already rounded to the dtypes they are stored in, C0 to bf16 so that it
    is exact in either output dtype) and the fp64 products A B^T and |A| |B|^T: one per (shape, in dtype, regime), shared by every
    layout, output dtype and mode."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 10007 + K * 101 + (in_dtype == "bf16") + 2 * (regime == "exact"))
    if regime == "exact":
        A = torch.randint(-3, 4, (M, K), generator=g).double()
        B = torch.randint(-3, 4, (N, K), generator=g).double()
        bias = torch.randint(-3, 4, (N,), generator=g).double()
        C0 = torch.randint(-3, 4, (M, N), generator=g).double()
        absP = None
    else:
        A = torch.randn(M, K, generator=g).to(TD[in_dtype]).double()
        B = torch.randn(N, K, generator=g).to(TD[in_dtype]).double()
        bias = torch.randn(N, generator=g).double()                       # f32
        C0 = torch.randn(M, N, generator=g).bfloat16().double()
        absP = A.abs() @ B.abs().t()
    return A, B, bias, C0, A @ B.t(), absP


def stored(X, k_contiguous, ld, td, regime, gen):
    """The operand as the kernel addresses it: [rows, ld] with the logical [R, K] matrix in [:, :K] (k-contiguous) or its transpose in
    [:, :R].  The padding columns are NaN in the exact regime and behind an m- / n-contiguous operand; behind a K tail in the rounding
    regime they hold ordinary numbers.  The split is deliberate, keep both: NaN shows any read of the padding at all, ordinary numbers
    are what the decoder's column-slice operands really have beside them (a read that NaN would only flag shows there as a wrong sum)."""
    body = X if k_contiguous else X.t()
    buf = torch.full((body.shape[0], ld), float("nan"), dtype=torch.float64)
    if k_contiguous and regime == "rounding" and ld > body.shape[1]:
        buf[:, body.shape[1]:] = torch.randn(body.shape[0], ld - body.shape[1], generator=gen).double()
    buf[:, :body.shape[1]] = body
    return buf.to(td)


def family(case):
    kernel = case.key[0]
    name = kernel.split("<")[0]
    if name == "gemm":
        f = kernel[5:-1].split(",")
        name = "gemm " + ("ring" if f[9] == "true" else "vec" if f[6] == "true" else "scalar") + (" split" if case.key[1] == "split" else "")
    return f"{name} {case.in_dtype}>{case.out_dtype} {'acc' if case.accumulate else 'ovw'}"


def run(E, dev, case, regime):
    M, N, K = case.M, case.N, case.K
    a_kc, b_kc = LAYOUTS[case.layout]
    lda, ldb, ldc = case.leading_dims()
    in_td, out_td = TD[case.in_dtype], TD[case.out_dtype]
    A, B, bias, C0, P, absP = operands(M, N, K, case.in_dtype, regime)
    gen = torch.Generator().manual_seed(7)
    Ad = stored(A, a_kc, lda, in_td, regime, gen).to(dev)
    Bd = stored(B, b_kc, ldb, in_td, regime, gen).to(dev)
    bias_d = bias.float().to(dev) if case.bias else None
    # C with a guard row on either side: sentinel everywhere but the live [M, N], which holds C0 (accumulate) or NaN (overwrite)
    buf = torch.full((M + 2, ldc), SENTINEL, dtype=out_td, device=dev)
    buf[1:M + 1, :N] = C0.to(out_td).to(dev) if case.accumulate else float("nan")
    before = buf.clone()
    Cd = buf[1:]

    E.set_deterministic(case.det)
    try:
        with E.route_only() as r:
            status = L.load().gic_gemm(*gemm_args(case, Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), bias_d.data_ptr() if case.bias else None, DT))
            line = r.last()
        assert status == 0 and route_key(line) == case.key, line
        E.gemm(Ad, Bd, Cd, M, N, K, lda, ldb, ldc, a_kc=bool(a_kc), b_kc=bool(b_kc), bias=bias_d, accumulate=bool(case.accumulate), alpha=case.alpha)
        torch.cuda.synchronize()
    finally:
        E.set_deterministic(False)

    got = buf[1:M + 1, :N].clone()
    buf[1:M + 1, :N] = before[1:M + 1, :N]
    touched = int((buf.view(BITS[out_td]) != before.view(BITS[out_td])).sum())
    assert touched == 0, f"{case.id} {regime}: {touched} elements of C's padding columns / guard rows changed"

    got_cpu = got.cpu()
    ref = case.alpha * P + (bias if case.bias else 0.0) + (C0 if case.accumulate else 0.0)
    if regime == "exact":
        want = ref.float().to(out_td)
        differ = int((got_cpu.view(BITS[out_td]) != want.view(BITS[out_td])).sum())
        if out_td == torch.bfloat16 and case.accumulate:
            # the bound is 2^-8 |ref|, which a single rounding always meets.  Both kernels add C to the f32 accumulators and round once,
            # so `differ` is expected to be 0 as well: it is printed and carried in the message so that a return of tile8's old double
            # rounding (product to bf16, then the sum: up to a whole ulp off) stays visible even where it slips under the bound
            over = int(((got_cpu.double() - ref).abs() > U_BF16 * ref.abs()).sum())
            print(f"[gemm matrix] {case.id} exact: {differ} of {M * N} elements differ from the once-rounded reference, {over} by more than 2^-8 |ref|")
            assert over == 0, f"{case.id} exact: {over} elements beyond 2^-8 |ref| ({differ} of {M * N} differ from the once-rounded reference)"
        else:
            print(f"[gemm matrix] {case.id} exact: {differ} of {M * N} elements differ")
            assert differ == 0, f"{case.id} exact: {differ} of {M * N} elements are not bit-identical to the fp64 reference cast to {case.out_dtype}"
        return
    bound = (K + 4) * U_F32 * (abs(case.alpha) * absP + (bias.abs() if case.bias else 0.0) + (C0.abs() if case.accumulate else 0.0))
    if out_td == torch.bfloat16:
        bound = bound + (2 * U_BF16 * (ref.abs() + C0.abs()) if case.accumulate else U_BF16 * ref.abs())
    err = (got_cpu.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = float((err / bound).max())
    print(f"[gemm matrix] {case.id} rounding: err/bound max {ratio:.4f}")
    fam = family(case)
    MAXIMA[fam] = max(MAXIMA.get(fam, 0.0), ratio)
    over = int((err > bound).sum())
    assert over == 0, f"{case.id} rounding: {over} of {M * N} elements beyond the bound, err/bound max {ratio}"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_variant(E, dev, case):
    run(E, dev, case, "exact")
    run(E, dev, case, "rounding")


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
def test_k_zero_is_the_empty_sum(E, dev, in_dtype, acc):
    """K = 0: C = bias (+ C0), exactly, and neither operand is read (they are NaN)."""
    M, N = 64, 72
    g = torch.Generator().manual_seed(11)
    bias, C0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    Ad = torch.full((M, 8), float("nan"), dtype=TD[in_dtype], device=dev)
    Bd = torch.full((N, 8), float("nan"), dtype=TD[in_dtype], device=dev)
    Cd = C0.to(dev) if acc else torch.full((M, N), float("nan"), device=dev)
    E.gemm(Ad, Bd, Cd, M, N, 0, 8, 8, N, bias=bias.to(dev), accumulate=acc, alpha=0.5)
    torch.cuda.synchronize()
    want = (bias + C0) if acc else bias.expand(M, N)
    assert torch.equal(Cd.cpu(), want)
