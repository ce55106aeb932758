"""What `gic::gemm()` runs in a train step and `gic_gemm` cannot express (tests/gemm_cases.py WGRAD_CASES), through gic_debug_gemm_desc,
element by element against an fp64 product: the weight-gradient form (EPI_WGRAD of csrc/gemm.hip: the column sums of A folded into
the product as a_sum / a_sum2, a second output matrix C2 from column n_split on, its own zero-fill launch under split-K) on both tile
widths and in both split states, and the caller-only flags c_zeroed and no_split.

Each case asserts its route (and status) with the real pointers before it launches, and then runs the two data regimes of
tests/test_gpu_gemm_matrix.py, whose operands, stored layouts and sentinel idiom are used by import:

  exact     integers in [-3, 3], alpha +-2^j, 9 K |alpha| < 2^24: C, C2, a_sum and a_sum2 are bit-identical to the fp64 reference cast to
            the output type under any order, split-K atomics included (bf16 accumulate: within 2^-8 |ref|); a_sum2 is bit-equal to a_sum.
  rounding  C and C2 per element within (K + 4) 2^-24 (|alpha| |A| |B|^T + |bias| + |C0|) + r, r as in the matrix test; a_sum[m] within
            (K + 4) 2^-24 (sum_k |A(m,k)| + |s0[m]|): the worst case of an f32 sum of K + 1 numbers in any order.  Derived, nothing is
            fitted to what the GPU returns.

The contract, with no element and no case left out (gemm_cases.check_wgrad):
  overwrite   C, C2 and the sums hold NaN beforehand; accumulate: a bf16-exact C0 / s0 that the reference adds; c_zeroed: zero.
  C2          its own buffer with a padded ldc2, a guard row on either side and sentinel padding columns: their bits must not change.
              The columns of C from n_split on keep their sentinel (the product must not write them), and so does everything of C2 left
              of column 0 (the guard row / the row above's padding).
  sums        a_sum and a_sum2 carry SUM_GUARD sentinel words on either side: entries m >= M do not exist.
  padding     the m- / n-contiguous row padding behind M and N is NaN in both regimes; the k rows from K up to a whole extra K tile are
              NaN in the exact regime and ordinary numbers in the rounding regime: a NaN (a wrong sum) in any output names the read.
  fall-backs  a route line without the a_sum= / n_split= suffix: a_sum, a_sum2 and C2 keep their prefill bit for bit, NaN included,
              and C is the plain product.  A refused descriptor (GIC_STATUS_UNSUPPORTED) writes nothing at all.
  no_split    two calls give the same bits, and the same again under engine.set_deterministic(True).
  launches    gic_debug_wgrad_launches moves by (1, 1 if C2 else 0) where the form is taken and by (0, 0) where it is not.
tests/test_gemm_cases.py shows without a GPU that the checker passes a plain numpy emulation of the form at every case and fails each of
gemm_cases.FAULTS.

Largest err / bound seen per family in the rounding regime (MI355X; C | C2, then a_sum; recorded, never asserted against; the module
prints the table again after every run under -s):
                               C | C2  ovw / acc      a_sum  ovw / acc
  wgrad 64        bf16>f32     0.1231 / 0.1521        0.0005 / 0.0005
  wgrad 64        bf16>bf16    0.9690 / 0.4441        0.0005 / 0.0000
  wgrad 64 split  bf16>f32     0.0011 / 0.0012        0.0001 / 0.0001
  wgrad 128       bf16>f32     0.1773 / 0.1908        0.0000 / 0.0000
  wgrad 128       bf16>bf16    0.9959 / 0.4969        0.0000 / 0.0000
  wgrad 128 split bf16>f32     0.0012 / 0.0012        0.0001 / 0.0001
  plain no_split  bf16>f32     0.0021 / 0.0019
  plain c_zeroed  bf16>f32     0.0739 /
  plain fall-back bf16>f32     0.0945 / 0.0905
  plain fall-back f32>f32      0.1475 /
(bf16 output: the bound is dominated by r as in the matrix test.  The sums are far inside their bound: the operands are bf16 numbers of
one magnitude, whose f32 sums round little; the exact regime and the NaN padding are what pin their structure.)"""
import ctypes
import functools

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests.gemm_cases import LAYOUTS, SUM_GUARD, WGRAD_CASES, check_wgrad, desc_args, route_key
from tests.test_gpu_gemm_matrix import BITS, DT, SENTINEL, TD, operands, stored

pytestmark = pytest.mark.gpu

DEVICE_REF_FROM = 2 ** 30          # M N K from which the fp64 reference products are formed on the device
MAXIMA = {}                        # err / bound maxima of the rounding regime per family: recorded, never asserted against


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
        print(f"\n[gemm wgrad] err/bound max {MAXIMA[fam]:.4f}  {fam}", end="")
    print()


@functools.lru_cache(maxsize=2)
def products(M, N, K, in_dtype, regime):
    """tests/test_gpu_gemm_matrix.py's `operands`; from DEVICE_REF_FROM on (a few GFLOP in fp64) the same draw with the two products
    formed by torch in fp64 on the device, where there is one."""
    if M * N * K < DEVICE_REF_FROM or not torch.cuda.is_available():
        return operands(M, N, K, in_dtype, regime)
    g = torch.Generator().manual_seed(M * 1000003 + N * 10007 + K * 101 + (in_dtype == "bf16") + 2 * (regime == "exact"))
    if regime == "exact":
        A, B = torch.randint(-3, 4, (M, K), generator=g).double(), torch.randint(-3, 4, (N, K), generator=g).double()
        bias, C0 = torch.randint(-3, 4, (N,), generator=g).double(), torch.randint(-3, 4, (M, N), generator=g).double()
    else:
        A, B = torch.randn(M, K, generator=g).to(TD[in_dtype]).double(), torch.randn(N, K, generator=g).to(TD[in_dtype]).double()
        bias, C0 = torch.randn(N, generator=g).double(), torch.randn(M, N, generator=g).bfloat16().double()
    Ad, Bd = A.cuda(), B.cuda()
    P = (Ad @ Bd.t()).cpu()
    absP = None if regime == "exact" else (Ad.abs() @ Bd.abs().t()).cpu()
    return A, B, bias, C0, P, absP


def k_rows(buf, k_contiguous, R, K, regime, gen):
    """An m- / n-contiguous operand [K, ld] with the k rows from K up to a whole K tile past the last one: NaN in the exact regime, ordinary
    numbers over the R live columns in the rounding regime (the row padding stays NaN).  The contract says none of them is read."""
    if k_contiguous:
        return buf
    tail = torch.full((-K % 64 + 64, buf.shape[1]), float("nan"), dtype=torch.float64)
    if regime == "rounding":
        tail[:, :R] = torch.randn(tail.shape[0], R, generator=gen).double()
    return torch.cat([buf, tail.to(buf.dtype)])


def make_host(case, regime):
    """The buffers of a run and its fp64 reference (gemm_cases: `host`), on the CPU."""
    M, N, K = case.M, case.N, case.K
    a_kc, b_kc = LAYOUTS[case.layout]
    lda, ldb, ldc = case.leading_dims()
    in_td, out_td = TD[case.in_dtype], TD[case.out_dtype]
    A, B, bias, C0, P, absP = products(M, N, K, case.in_dtype, regime)
    gen = torch.Generator().manual_seed(7)
    A_st = k_rows(stored(A, a_kc, lda, in_td, regime, gen), a_kc, M, K, regime, gen)
    B_st = k_rows(stored(B, b_kc, ldb, in_td, regime, gen), b_kc, N, K, regime, gen)
    s0 = (torch.randint(-3, 4, (M,), generator=gen) if regime == "exact" else torch.randn(M, generator=gen).bfloat16()).double()
    fill = lambda X0: X0 if case.accumulate else 0.0 if case.c_zeroed else float("nan")
    two = case.form and case.c2                       # (a refused or fallen-back C2 is a buffer nobody may write)
    ns = case.n_split if two else N
    C = torch.full((M + 2, ldc), SENTINEL, dtype=out_td)
    C[1:M + 1, :ns] = fill(C0[:, :ns].to(out_td))
    C2 = None
    if case.c2:
        C2 = torch.full((M + 2, case.ldc2), SENTINEL, dtype=out_td)
        w = min(max(N - case.n_split, 0), case.ldc2)
        C2[1:M + 1, :w] = fill(C0[:, N - w:].to(out_td))
    sums = []
    for i in range(2):
        s = None
        if case.sums > i:
            s = torch.full((M + 2 * SUM_GUARD,), SENTINEL, dtype=torch.float32)
            s[SUM_GUARD:SUM_GUARD + M] = s0.float() if case.accumulate else float("nan")
        sums.append(s)
    return {"A": A_st, "B": B_st, "bias": bias.float() if case.bias else None, "C": C, "C2": C2, "s1": sums[0], "s2": sums[1],
            "ref": {"A": A, "B": B, "bias": bias, "C0": C0, "s0": s0, "P": P, "absP": absP}}


def wgrad_launches():
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    L.load().gic_debug_wgrad_launches(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def upload(t, dev, off=0):
    """`t` on the device, `off` elements past an allocation's (16-byte aligned) start."""
    if t is None:
        return None
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    view = flat[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def launch(E, dev, case, host, det, tag):
    """One call on fresh device buffers under deterministic mode `det`; where `det` is the case's own mode the route, the status and the
    launch counter are asserted.  Returns what it left (gemm_cases: `after`)."""
    lib = L.load()
    M = case.M
    a_kc, b_kc = LAYOUTS[case.layout]
    lda, ldb, ldc = case.leading_dims()
    Ad, Bd = upload(host["A"], dev, case.misalign == "A"), upload(host["B"], dev, case.misalign == "B")
    bias, C, C2, s1, s2 = (upload(host[k], dev) for k in ("bias", "C", "C2", "s1", "s2"))
    ptr = lambda t, skip: None if t is None else t[skip:].data_ptr()
    E.set_deterministic(det)
    try:
        own = det == case.det
        if own:
            with E.route_only() as r:
                status = lib.gic_debug_gemm_desc(*desc_args(case, Ad.data_ptr(), Bd.data_ptr(), ptr(C, 1), ptr(bias, 0), DT, ptr(s1, SUM_GUARD),
                                                            ptr(s2, SUM_GUARD), ptr(C2, 1)))
                line = r.last()
            assert status == case.status and route_key(line) == case.key, f"{tag}: status {status}, {line}"
        n0 = wgrad_launches()
        if case.status:
            status = lib.gic_debug_gemm_desc(*desc_args(case, Ad.data_ptr(), Bd.data_ptr(), ptr(C, 1), ptr(bias, 0), DT, ptr(s1, SUM_GUARD),
                                                        ptr(s2, SUM_GUARD), ptr(C2, 1))[:-1], E.stream_ptr())
            assert status == case.status, f"{tag}: status {status}"
        else:
            E.gemm_desc(Ad, Bd, C[1:], M, case.N, case.K, lda, ldb, ldc, a_kc=bool(a_kc), b_kc=bool(b_kc), bias=bias, accumulate=bool(case.accumulate),
                        alpha=case.alpha, c_zeroed=case.c_zeroed, no_split=case.no_split, wgrad=case.wgrad,
                        a_sum=None if s1 is None else s1[SUM_GUARD:], a_sum2=None if s2 is None else s2[SUM_GUARD:],
                        C2=C2[1:] if case.c2 else None, ldc2=case.ldc2, n_split=case.n_split)
        torch.cuda.synchronize()
        n1 = wgrad_launches()
    finally:
        E.set_deterministic(False)
    if own:
        took = (1, int(case.c2)) if case.form else (0, 0)
        assert (n1[0] - n0[0], n1[1] - n0[1]) == took, f"{tag}: folded / two-matrix launches {n1[0] - n0[0]} / {n1[1] - n0[1]}, expected {took}"
    return {"C": C.cpu(), "C2": None if C2 is None else C2.cpu(), "s1": None if s1 is None else s1.cpu(), "s2": None if s2 is None else s2.cpu()}


def family(case):
    if not case.form:
        return f"plain {'c_zeroed' if case.c_zeroed else 'no_split' if case.no_split else 'fall-back'} {case.in_dtype}>{case.out_dtype} {'acc' if case.accumulate else 'ovw'}"
    return f"wgrad {case.key[0].split(',')[4]}{' split' if case.key[1] == 'split' else ''} bf16>{case.out_dtype} {'acc' if case.accumulate else 'ovw'}"


def same_bits(a, b):
    return a is b or bool((a.view(BITS[a.dtype]) == b.view(BITS[b.dtype])).all())


def run(E, dev, case, regime):
    tag = f"{case.id} {regime}"
    host = make_host(case, regime)
    after = launch(E, dev, case, host, case.det, tag)
    ratios = check_wgrad(case, regime, host, after)
    print(f"[gemm wgrad] {tag}: " + ("ok" if regime == "exact" or not ratios else "  ".join(f"{k} err/bound max {v:.4f}" for k, v in ratios.items())))
    for k, v in ratios.items():
        fam = f"{family(case)} {k}"
        MAXIMA[fam] = max(MAXIMA.get(fam, 0.0), v)
    if case.no_split:
        again, det = launch(E, dev, case, host, case.det, tag), launch(E, dev, case, host, not case.det, tag)
        assert all(same_bits(after[k], again[k]) for k in ("C", "C2", "s1", "s2")), f"{tag}: two no_split calls differ"
        assert same_bits(after["C"], det["C"]), f"{tag}: no_split gives other bits in the deterministic mode"


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.id for c in WGRAD_CASES])
def test_gemm_descriptor(E, dev, case):
    run(E, dev, case, "exact")
    run(E, dev, case, "rounding")
