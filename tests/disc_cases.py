"""The sequence discriminator (csrc/disc.hip) stage by stage: the case table, the fp64 reference of every stage, the per-element bounds
and the checker behind tests/test_disc_cases.py (no GPU: route pins, the selection restated and held to the library's own, checker self-test) and
tests/test_gpu_disc_stages.py (which runs every case on the GPU).  Nothing here touches the GPU.

Every stage is checked against an fp64 reference formed from the buffers the kernels themselves wrote upstream of it (`emb`, `pooled`,
`argmax`, `hpre`, `keep`, `ydrop`, `feat`, `dfeat`, `dydrop`, `dh`, `dpooled`, `demb`), so errors do not compound and a max-pool
near-tie upstream excuses nothing downstream.  `run_forward` / `run_backward` walk the stages in order; with a Report they compare the
buffers given, without one they FILL the buffers from the references (a correct result in storage precision: what the checker's
self-test mutates).

Bounds, per element, u = 2^-24, r = 2^-8 |ref| where the output is bf16 (else 0).  All derived, none fitted:
  sum     a sum of n products in any order (MFMA, split-K, atomics):  (n + 4) u (sum |terms| + |bias| + |C0|) + r
  max     |pooled - max_t relu(pre_t)| <= the largest window bound of that (row, filter) + r; the fp64 relu(pre) at the kernel's own
          argmax lies within twice that bound of the maximum.  No entry is excluded, no flip is tolerated.
  point   the highway gate and its derivative: 8 u (sum of the magnitudes of the expression's terms) keep_scale + r.  8 counts the f32
          operations of highway_gate / its derivative with expf at 1 ulp; "terms" are the operands before any cancellation:
          1 - sg counts as 1 + sg, relu(h) - x as |relu(h)| + |x|.
  Every non-zero bound carries an underflow floor of 2^-110 (results below the smallest normal number may be flushed to zero).
  exact   bit equality (gather, dfeat, keep, pad columns, weight images, and everything in the integer regime).
A forward-only pass saves no `hpre`: its `ydrop` is checked against the fp64 gate of the fp64 product, the bound widened by the product's
own bound times sup |dy/dh| <= 1 + (|h| + |x|) / 4."""
import math
from typing import NamedTuple, Optional, Tuple

import torch

U, U8 = 2.0 ** -24, 2.0 ** -8
TINY = 2.0 ** -110         # underflow: up to 2^16 operations each flushing a result below the smallest normal 2^-126 to zero
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
OUT, OUT_PAD = 100, 104
K_MAX_TAPS = 32
DROP_P = 0.2
SENTINEL = 1232.0          # exact in bf16 and f32


class Case(NamedTuple):
    name: str
    B: int
    L: int
    R: int
    De: int
    fs: Tuple[int, ...]
    nf: Tuple[int, ...]
    dtype: str                    # "f32" | "bf16"
    fwd: str                      # the forward convolution kernel: "mfma" | "bf16" | "scalar8" | "scalar32"
    bwd_x: Optional[str]          # "small1" | "small4" (rows per block) | "general"; None: no backward (forward only)
    bwd_w: Optional[str]          # "lds" | "w8" | "w32"
    forward_only: bool = False
    fp_align: int = 64
    exact: bool = True            # the integer regime runs too (>= 100 tied and >= 100 zero maxima: test_disc_cases.py)
    det: bool = False             # the backward runs again in deterministic mode
    V: int = 50

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    @property
    def s(self):
        return self.De // self.R

    @property
    def F(self):
        return sum(self.nf)

    @property
    def Fp(self):
        return (self.F + self.fp_align - 1) // self.fp_align * self.fp_align

    @property
    def MR(self):
        return self.B * self.R


def select(case):
    """select_disc_fwd's and select_disc_bwd's choice of convolution kernels (csrc/disc.hip), restated without the library: (fwd, bwd_x,
    bwd_w).  tests/test_disc_cases.py::test_library_plan_is_the_restated_selection holds it to gic_debug_disc_plan on every case."""
    s, MR = case.s, case.MR
    mt = max(f * s for f in case.fs)
    assert mt <= K_MAX_TAPS and case.L <= 255 and all(1 <= f <= case.L for f in case.fs)
    if s == 1 and mt <= 8 and case.dtype == "bf16" and case.forward_only and case.L <= 64:
        fwd = "bf16"
    elif s == 1 and mt <= 8:
        fwd = "mfma"
    else:
        fwd = "scalar8" if mt <= 8 else "scalar32"
    if case.forward_only:
        return fwd, None, None
    lds = mt <= 8 and s == 1 and case.R <= 64 and case.R <= case.De and case.L <= 64
    bwd_w = "lds" if lds else ("w8" if mt <= 8 else "w32")
    if case.L * s <= 32 and case.F <= 1024 and mt <= 8:
        bwd_x = "small4" if MR >= 2048 else "small1"
    else:
        bwd_x = "general"
    return fwd, bwd_x, bwd_w


def det_plan(case, det=True):
    """select_disc_bwd's grids, restated without the library (held to it by the same test as `select`): (blocks of disc_out_bwd, whether
    their partials are folded, block rows of the conv weight gradient, whether theirs are).  Deterministic mode: what `dydrop` (MR * Fp
    floats) has room for; det=False: the grids outside it, nothing folded."""
    s, MR = case.s, case.MR
    dy = MR * case.Fp
    out_blocks = max(1, min(256, dy // (OUT + 1))) if det else 256
    mt = max(f * s for f in case.fs)
    lds = select(case)[2] == "lds"
    gy = min(64, -(-MR // 32))
    rows_y = min(MR // case.R, 64) if lds else gy
    mt1 = (8 if mt <= 8 else K_MAX_TAPS) + 1
    if det and rows_y * case.F * mt1 > dy:
        rows_y = dy // (case.F * mt1)
    rows_y = max(1, rows_y)
    return out_blocks, det and out_blocks > 1, rows_y, det and rows_y > 1


W5 = ((1, 2, 4, 5, 8), (5, 16, 17, 33, 20))          # nine filter tiles of 16 (the `tile & 7` round robin wraps), five of 32; F = 91


def _both(name, *a, **kw):
    return [Case(name, *a[:6], "f32", *a[6:], **kw), Case(name, *a[:6], "bf16", *a[6:], **kw)]


CASES = (
    # 1. f32-product MFMA forward, bwd_x_small (1 row per block), LDS weight gradient: 72 pairs = four 16-pair groups and one of 8
    _both("r24-L11", 3, 11, 24, 24, *W5, "mfma", "small1", "lds", det=True)
    + _both("r24-L8", 3, 8, 24, 24, *W5, "mfma", "small1", "lds")                                # width 8: one window
    # 2. R > 32: the second r0 pass; 70 captions > 64 block rows; 2800 rows: 4 rows per block.  Then 2050 rows = 512 * 4 + 2
    + _both("r40-b70", 70, 11, 40, 40, *W5, "mfma", "small4", "lds")
    + _both("r10-b205", 205, 9, 10, 10, (1, 3, 6, 7), (12, 20, 9, 23), "mfma", "small4", "lds")
    # 3. long captions: argmax up to 254, general bwd_x with NG = 1, weight gradient <8>; either side of L = 64 and L = 32; R > 64
    + _both("r5-L255", 1, 255, 5, 5, (1, 8), (300, 24), "mfma", "general", "w8", det=True)
    + _both("r24-L65", 3, 65, 24, 24, *W5, "mfma", "general", "w8")
    + _both("r24-L33", 3, 33, 24, 24, *W5, "mfma", "general", "lds")
    + _both("r72-L9", 2, 9, 72, 72, (2, 3, 7), (20, 30, 14), "mfma", "small1", "w8")
    # 4. s > 1: the scalar forward kernels
    + _both("s2-L16", 40, 16, 3, 6, (1, 3, 4), (20, 20, 24), "scalar8", "small1", "w8", det=True)
    + _both("s2-L130", 20, 130, 3, 6, (1, 3, 4), (160, 20, 24), "scalar8", "general", "w8")
    + _both("s4-L12", 30, 12, 4, 16, (2, 8), (40, 24), "scalar32", "general", "w32", det=True)
    # 5. F > 1024 leaves the four-filters-per-thread bwd_x_small
    + _both("f1030", 2, 4, 4, 4, (1,), (1030,), "mfma", "general", "lds")
    # 5b. the general bwd_x past 64 KB of dynamic LDS, which its launcher asks the grant for (common.h grant_lds): geff, tst, meta [Fp = 1472]
    # + part [NG = 32][n_out = 8] + the staged weights [1465 * 8] = (3 * 1472 + 256 + 11720) * 4 = 65568 bytes; one filter fewer is 65536,
    # within the default.  The smallest bank of the width-8 / L = 8 family that crosses it (one window per filter: no ties, no integer regime)
    + _both("lds-grant", 2, 8, 3, 3, (8,), (1465,), "mfma", "general", "lds", exact=False)
    # 7. no pad columns at all
    + _both("fp8", 3, 11, 24, 24, (1, 2, 4, 5, 8), (5, 16, 17, 30, 20), "mfma", "small1", "lds", fp_align=8)
    # 10. deterministic mode with room in dydrop for one block row only (MR = 5, Fp = 64, F = 40); then for one disc_out_bwd block only
    + _both("det-cap5", 1, 6, 5, 5, (2, 3), (24, 16), "mfma", "small1", "lds", exact=False, det=True)
    + _both("det-cap3", 1, 6, 3, 3, (2, 3), (24, 16), "mfma", "small1", "lds", exact=False, det=True)
    # 6. bf16 forward only: the bf16-product kernel up to L = 64 (odd and even window counts, a partial 32-pair group), beyond it the f32 MFMA
    + [Case("fo-r24-L11", 3, 11, 24, 24, *W5, "bf16", "bf16", None, None, forward_only=True),
       Case("fo-r24-L8", 3, 8, 24, 24, *W5, "bf16", "bf16", None, None, forward_only=True),
       Case("fo-r24-L64", 3, 64, 24, 24, *W5, "bf16", "bf16", None, None, forward_only=True),
       Case("fo-r24-L65", 3, 65, 24, 24, *W5, "bf16", "mfma", None, None, forward_only=True),
       Case("fo-r24-L11", 3, 11, 24, 24, *W5, "f32", "mfma", None, None, forward_only=True)]
)

# 8. highway forward: (rows, F, Fp, dtype, hpre offset in bytes) -> the route line up to " lds=".  One shape per distinct route of
# HIGHWAY_SCAN (test_disc_cases.py reads which routes exist from the scan and fails for any that has no shape here); rows are off the
# 4-row Philox quads and the 128-row tiles, F % 8 != 0 puts live and dead columns into one 8-column patch.
HIGHWAY_SCAN_ROWS = (5, 72, 130, 2050, 4100, 4101, 8200, 8201, 16500, 22301)
HIGHWAY_SCAN_F = ((91, 128), (200, 256), (203, 256), (260, 320), (900, 960))


class Highway(NamedTuple):
    rows: int
    F: int
    Fp: int
    dtype: str
    off: int                      # hpre starts this many bytes off its 16-byte alignment
    route: str

    @property
    def id(self):
        return f"{self.rows}x{self.F}-{self.dtype}{'-off' + str(self.off) if self.off else ''}"

    def case(self):
        """The discriminator around the product: one caption of `rows` representations, one bank of F filters of width 2 over L = 3."""
        return Case("hw-" + self.id, 1, 3, self.rows, self.rows, (2,), (self.F,), self.dtype, "mfma", None, None,
                    fp_align=self.Fp, exact=False)


HIGHWAY = [
    Highway(5, 91, 128, "bf16", 0, "gemm<bf16,bf16,true,true,64,64,true,1,false,false> grid=2x1 block=256"),
    Highway(5, 91, 128, "f32", 0, "gemm<f32,f32,true,true,64,64,true,1,false,false> grid=2x1 block=256"),
    Highway(5, 203, 256, "f32", 0, "gemm<f32,f32,true,true,64,64,true,1,false,true> grid=4x1 block=256"),
    Highway(5, 900, 960, "bf16", 0, "gemm<bf16,bf16,true,true,64,64,true,1,false,true> grid=15x1 block=256"),
    Highway(4101, 203, 256, "bf16", 0, "tile8<bf16,64,1,false,4,false,false,1024> grid=132 block=512"),
    Highway(4101, 900, 960, "bf16", 0, "tile8<bf16,128,1,false,2,false,false,1024> grid=264 block=512"),
    Highway(4101, 900, 960, "bf16", 8, "gemm<bf16,bf16,true,true,128,128,true,1,false,true> grid=264x1 block=256"),
    Highway(8201, 203, 256, "bf16", 0, "tile8<bf16,64,1,false,2,false,false,1024> grid=260 block=512"),
    Highway(8201, 260, 320, "bf16", 0, "tile8<bf16,128,1,false,4,false,false,1024> grid=195 block=512"),
    Highway(8201, 260, 320, "bf16", 8, "gemm<bf16,bf16,true,true,128,128,true,1,false,false> grid=195x1 block=256"),
    Highway(8201, 260, 320, "f32", 0, "gemm<f32,f32,true,true,128,128,true,1,false,true> grid=195x1 block=256"),
    Highway(22301, 260, 320, "f32", 0, "gemm<f32,f32,true,true,128,128,true,1,false,false> grid=525x1 block=256"),
]


# ---------------------------------------------------------------------------------------------------------------- data
def make_params(case, regime, gen):
    """Master weights in the engine's order [emb, (conv_w, conv_b) * nconv, hw_w, hw_b, f2o_w, f2o_b, o2l_w, o2l_b], float32 on the CPU.
    exact: integers (embedding [-3, 3], filters [-2, 2], biases [-3, 3]).  rounding: Gaussian, the filter biases set so that about half
    of the maxima over time are positive (P(max of T windows <= 0) = 1/2 at bias -z for independent unit-variance windows; overlapping
    windows are not independent, 0.8 z brings the table's cases to 0.3 .. 0.6)."""
    s, F = case.s, case.F
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    P = [ri(-3, 3, case.De, case.V) if regime == "exact" else rn(case.De, case.V)]
    for f, n in zip(case.fs, case.nf):
        if regime == "exact":
            P += [ri(-2, 2, n, 1, f, s), ri(-3, 3, n)]
        else:
            T = case.L - f + 1
            z = float(torch.special.ndtri(torch.tensor(0.5 ** (1.0 / T), dtype=torch.float64)))
            P += [rn(n, 1, f, s) / math.sqrt(f * s), -0.8 * z + 0.3 * rn(n)]
    P += [2.0 * rn(F, F) / math.sqrt(F), 0.5 * rn(F), rn(OUT, F) / math.sqrt(F), 0.1 * rn(OUT), 0.1 * rn(1, OUT), rn(1)]
    return P


def make_inputs(case, gen, soft=False, train=True, mask=True):
    """ids [B, L] or a Gaussian soft input [B, L, V] / sqrt(V) in the activation dtype, the keep mask [MR, F] (train) and d_logits [MR]."""
    X = {"train": train, "ids": None, "soft": None, "mask": None}
    if soft:
        X["soft"] = (torch.randn(case.B, case.L, case.V, generator=gen) / math.sqrt(case.V)).to(TD[case.dtype])
    else:
        X["ids"] = torch.randint(0, case.V, (case.B, case.L), generator=gen)
    if train and mask:
        X["mask"] = (torch.rand(case.MR, case.F, generator=gen) >= DROP_P).to(torch.uint8)
    X["d_logits"] = torch.randn(case.MR, generator=gen)
    return X


def images(case, P):
    """The compute-dtype weight images gic_disc_prepare keeps: master.to(dtype), zero-padded to [Fp, Fp] / [104, Fp]."""
    td, F, Fp, n = TD[case.dtype], case.F, case.Fp, len(case.fs)
    hw = torch.zeros(Fp, Fp, dtype=td)
    hw[:F, :F] = P[1 + 2 * n].to(td)
    f2o = torch.zeros(OUT_PAD, Fp, dtype=td)
    f2o[:OUT, :F] = P[3 + 2 * n].to(td)
    return {"emb": P[0].to(td), "hw_w": hw, "f2o_w": f2o, "hw_w_t": hw.t().contiguous()}


# ---------------------------------------------------------------------------------------------------------------- checker
class Report:
    """Per stage: the largest err / bound seen and, for a stage with an element beyond its bound, a message."""

    def __init__(self):
        self.ratio, self.failed = {}, {}

    def check(self, stage, got, ref, bound):
        err = (got.double() - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        bound = bound.expand_as(err) if torch.is_tensor(bound) else torch.full_like(err, bound)
        bound = torch.where(bound > 0, bound + TINY, bound)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        top = float(ratio.max()) if ratio.numel() else 0.0
        self.ratio[stage] = max(self.ratio.get(stage, 0.0), top)
        over = int((err > bound).sum())
        if over:
            self.failed.setdefault(stage, f"{over} of {err.numel()} elements beyond the bound, err/bound max {top:.4g}")

    def exact(self, stage, ok, what=""):
        ok = ok if torch.is_tensor(ok) else torch.tensor(bool(ok))
        self.ratio.setdefault(stage, 0.0)
        bad = int((~ok).sum())
        if bad:
            self.failed.setdefault(stage, f"{bad} of {ok.numel()} elements {what or 'differ'}")

    def bits(self, stage, got, want, what=""):
        want = want.to(got.dtype)
        self.exact(stage, got.contiguous().view(BITS.get(got.dtype, got.dtype)) == want.contiguous().view(BITS.get(got.dtype, got.dtype)),
                   what or "are not bit-identical")


def _r(ref, bf16):
    return U8 * ref.abs() if bf16 else 0.0


def sum_bound(n, mag, ref, bf16_out=False):
    return (n + 4) * U * mag + _r(ref, bf16_out)


class _Emit:
    """Compare a buffer with its reference (report given) or fill it from the reference (none)."""

    def __init__(self, buf, rep):
        self.buf, self.rep = buf, rep

    def __call__(self, name, ref, bound, dtype, cols=None, stage=None):
        stage = stage or name
        if self.rep is None:
            if cols is None:
                self.buf[name] = ref.to(dtype)
            else:
                self.buf[name][:, :cols] = ref.to(dtype)
        else:
            got = self.buf[name] if cols is None else self.buf[name][:, :cols]
            self.rep.check(stage, got, ref, bound)

    def same(self, name, want, cols=None, stage=None):
        stage = stage or name
        if self.rep is None:
            if cols is None:
                self.buf[name] = want.clone()
            else:
                self.buf[name][:, :cols] = want
        else:
            self.rep.bits(stage, self.buf[name] if cols is None else self.buf[name][:, :cols], want)

    def pad_zero(self, name, F):
        if self.rep is not None and self.buf[name].shape[1] > F:
            self.rep.exact(name + " pad", self.buf[name][:, F:].float() == 0, "of the pad columns are not zero")


def conv_windows(case, emb, f):
    """emb [B*L, De] -> the windows [B*R, T, f*s] of width f (tap index j * s + e), row b * R + r."""
    x = emb.view(case.B, case.L, case.R, case.s)
    return x.unfold(1, f, 1).permute(0, 2, 1, 4, 3).reshape(case.MR, case.L - f + 1, f * case.s)


def conv_pre(case, P, emb_f32, rounded=None):
    """Per bank: (relu(pre) [MR, T, n], per-window bound [MR, T, n]) in fp64 from the f32 embedding buffer.  The bf16-product kernel
    rounds the embedding and the filters to bf16 (not the bias)."""
    bf = case.fwd == "bf16" if rounded is None else rounded
    emb = (emb_f32.bfloat16() if bf else emb_f32).double()
    out = []
    for k, f in enumerate(case.fs):
        w, b = P[1 + 2 * k].reshape(case.nf[k], -1), P[2 + 2 * k].double()
        w = (w.bfloat16() if bf else w).double()
        win = conv_windows(case, emb, f)
        pre = win @ w.t() + b
        mag = win.abs() @ w.abs().t() + b.abs()
        out.append((torch.relu(pre), (f * case.s + 4) * U * mag))
    return out


def first_max(v):
    """max over dim 1 of v [MR, T, n] with the FIRST index on ties."""
    vmax = v.max(1).values
    t = torch.arange(v.shape[1]).view(1, -1, 1).expand_as(v)
    first = torch.where(v == vmax.unsqueeze(1), t, torch.full_like(t, v.shape[1])).min(1).values
    return vmax, first


def tie_counts(case, P, ids):
    """(entries with a tied positive maximum, entries with maximum 0) over all (row, filter) of the integer regime."""
    emb = P[0].t()[ids.reshape(-1)].contiguous()
    tied = zero = 0
    for v, _ in conv_pre(case, P, emb, rounded=False):
        vmax = v.max(1).values
        tied += int((((v == vmax.unsqueeze(1)).sum(1) > 1) & (vmax > 0)).sum())
        zero += int((vmax == 0).sum())
    return tied, zero


def new_state(case):
    """State buffers as DiscEngine.alloc_state shapes them (CPU; pads as a correct run leaves them)."""
    td, MR, Fp = TD[case.dtype], case.MR, case.Fp
    st = {"emb": torch.zeros(case.B * case.L, case.De), "pooled": torch.zeros(MR, Fp, dtype=td), "ydrop": torch.zeros(MR, Fp, dtype=td),
          "feat": torch.zeros(MR, OUT), "logits": torch.zeros(MR), "argmax": None, "hpre": None, "keep": None}
    if not case.forward_only:
        st.update(argmax=torch.zeros(MR, Fp, dtype=torch.uint8), hpre=torch.zeros(MR, Fp), keep=torch.zeros(MR, Fp, dtype=torch.uint8))
    return st


def new_ws(case):
    td, MR, Fp = TD[case.dtype], case.MR, case.Fp
    return {"dfeat": torch.zeros(MR, OUT_PAD, dtype=td), "dh": torch.zeros(MR, Fp, dtype=td), "dydrop": torch.zeros(MR, Fp),
            "dpooled": torch.zeros(MR, Fp), "demb": torch.zeros(case.B * case.L, case.De, dtype=td)}


def run_forward(case, P, img, X, buf, rep=None, exact=False, mut=None, stages=None):
    """Walk the forward stages over `buf` (new_state's keys + "logits").  rep: check; None: fill.  `mut`: a mutation of the fill (the
    checker's self-test).  `stages`: only these."""
    td, F, Fp, MR = TD[case.dtype], case.F, case.Fp, case.MR
    bf = case.dtype == "bf16"
    emit = _Emit(buf, rep)
    want = lambda s: stages is None or s in stages
    # 1. embedding: a gather (bit for bit) or inp W_emb^T over the compute-dtype image
    if want("emb"):
        if X["ids"] is not None:
            emit.same("emb", P[0].t()[X["ids"].reshape(-1)].contiguous())
        else:
            a, w = X["soft"].reshape(-1, case.V).double(), img["emb"].double()
            emit("emb", a @ w.t(), sum_bound(case.V, a.abs() @ w.abs().t(), None), torch.float32)
    # 2. convolution + relu + max over time
    if want("pooled"):
        Pm = P
        if mut == "no_taps_4_7":
            Pm = list(P)
            for k, f in enumerate(case.fs):
                if f > 4:
                    Pm[1 + 2 * k] = P[1 + 2 * k].clone()
                    Pm[1 + 2 * k][:, :, 4:, :] = 0
        off = 0
        for k, (v, wb) in enumerate(conv_pre(case, Pm, buf["emb"])):
            n, T = case.nf[k], v.shape[1]
            if mut == "drop_last_t" and T > 1:
                v = v[:, :T - 1]
            vmax, first = first_max(v)
            mb = torch.zeros_like(vmax) if exact else wb.max(1).values
            if rep is None:
                if mut == "argmax_ge":
                    t = torch.arange(v.shape[1]).view(1, -1, 1).expand_as(v)
                    last = torch.where(v == vmax.unsqueeze(1), t, torch.full_like(t, -1)).max(1).values
                    first = torch.where(vmax > 0, last, torch.zeros_like(last))
                buf["pooled"][:, off:off + n] = vmax.to(td)
                if buf["argmax"] is not None:
                    buf["argmax"][:, off:off + n] = first.to(torch.uint8)
            else:
                got = buf["pooled"][:, off:off + n]
                if exact:
                    rep.bits("pooled", got, vmax.float().to(td))
                else:
                    rep.check("pooled", got, vmax, mb + _r(vmax, bf))
                if buf["argmax"] is not None:
                    am = buf["argmax"][:, off:off + n].long()
                    inside = am < T
                    at = v.gather(1, am.clamp_max(T - 1).unsqueeze(1)).squeeze(1)
                    if exact:
                        rep.exact("argmax", inside & (am == first), "are not the first index of the maximum")
                    else:
                        rep.exact("argmax", inside & (at >= vmax - 2 * mb), "are not within twice the bound of the maximum")
            off += n
        if rep is None:
            if mut == "partial_group_unwritten" and MR % 16:
                buf["pooled"][MR // 16 * 16:, :F] = SENTINEL
            if mut == "tile_to_neighbour":
                a, b = case.nf[0], case.nf[0] + 16
                buf["pooled"][:, a:a + 32] = torch.cat([buf["pooled"][:, b:b + 16], buf["pooled"][:, a:a + 16]], 1)
        emit.pad_zero("pooled", F)
        if buf["argmax"] is not None:
            emit.pad_zero("argmax", F)
    if exact:
        return
    # 3. highway: h = pooled W^T + b (saved), y = sg relu(h) + (1 - sg) x, ydrop = y keep scale
    if want("ydrop"):
        x = buf["pooled"][:, :F].double()
        W, b = img["hw_w"][:F, :F].double(), P[-5].double()
        h_ref = x @ W.t() + b
        h_bnd = sum_bound(Fp, x.abs() @ W.abs().t() + b.abs(), None)
        if buf["hpre"] is not None:
            emit("hpre", h_ref, h_bnd, torch.float32, cols=F)
        scale = 1.0 / (1.0 - DROP_P) if X["train"] else 1.0
        keep = 1.0
        if X["train"]:
            if X["mask"] is not None:
                m = X["mask"]
                if rep is None and mut == "keep_quad_shift":
                    m = m.clone()
                    m[4:8] = torch.roll(m[4:8], 1, 0)
                emit.same("keep", m, cols=F)
            keep = buf["keep"][:, :F].double()
        h = buf["hpre"][:, :F].double() if buf["hpre"] is not None else h_ref
        sg = torch.sigmoid(h)
        y_ref = (sg * torch.relu(h) + (1 - sg) * x) * keep * scale
        y_bnd = 8 * U * (sg * torch.relu(h) + (1 + sg) * x.abs()) * keep * scale
        if buf["hpre"] is None:
            y_bnd = y_bnd + (1 + 0.25 * (h.abs() + h_bnd + x.abs())) * h_bnd * scale
        emit("ydrop", y_ref, y_bnd + _r(y_ref, bf), td, cols=F)
        emit.pad_zero("ydrop", F)
    # 4. head: feat = ydrop W_f2o^T + b; logits = feat . w + b
    if want("feat"):
        y = buf["ydrop"][:, :F].double()
        W, b = img["f2o_w"][:OUT, :F].double(), P[-3].double()
        emit("feat", y @ W.t() + b, sum_bound(Fp, y.abs() @ W.abs().t() + b.abs(), None), torch.float32)
        f, w, b = buf["feat"].double(), P[-2].double().reshape(-1), P[-1].double()
        emit("logits", f @ w + b, sum_bound(OUT, f.abs() @ w.abs() + b.abs(), None), torch.float32)


def conv_grads(case, P, st, dpooled, rows=None):
    """fp64 from the saved state and the GPU's dpooled: demb [B*L, De] with its magnitude sum, and per bank (dw, |dw| sum, db, |db| sum).
    `rows`: a 0/1 row weight (the weight gradients of a subset of the rows)."""
    B, L, R, s, MR = case.B, case.L, case.R, case.s, case.MR
    xrow = st["emb"].double().view(B, L, R, s).permute(0, 2, 1, 3).reshape(MR, L, s)
    dx, dxm = torch.zeros(MR, L, s, dtype=torch.float64), torch.zeros(MR, L, s, dtype=torch.float64)
    banks, off = [], 0
    for k, f in enumerate(case.fs):
        n = case.nf[k]
        w = P[1 + 2 * k].double().reshape(n, f, s)
        g = torch.where(st["pooled"][:, off:off + n].double() > 0, dpooled[:, off:off + n].double(), torch.zeros((), dtype=torch.float64))
        t0 = st["argmax"][:, off:off + n].long().clamp_max(L - f)
        gw = g if rows is None else g * rows.double().unsqueeze(1)
        dw, dwm = torch.zeros(n, f, s, dtype=torch.float64), torch.zeros(n, f, s, dtype=torch.float64)
        for j in range(f):
            idx = (t0 + j).unsqueeze(2).expand(MR, n, s)
            src = g.unsqueeze(2) * w[None, :, j, :]
            dx.scatter_add_(1, idx, src)
            dxm.scatter_add_(1, idx, src.abs())
            xg = xrow.gather(1, idx)
            dw[:, j, :] = (gw.unsqueeze(2) * xg).sum(0)
            dwm[:, j, :] = (gw.unsqueeze(2) * xg).abs().sum(0)
        banks.append((dw.reshape(n, 1, f, s), dwm.reshape(n, 1, f, s), gw.sum(0), gw.abs().sum(0)))
        off += n
    back = lambda t: t.view(B, R, L, s).permute(0, 2, 1, 3).reshape(B * L, R * s)
    return back(dx), back(dxm), banks


def run_backward(case, P, img, X, st, ws, grads, G0, d_inp, rep=None, mut=None, det=False, mixed=None):
    """Walk the backward stages.  st: the saved forward state; ws: new_ws's keys; grads: the parameter gradients in the engine's order or
    None; G0: what they held before the call (accumulate) or None; d_inp: [B*L, V] or None.  det: `dydrop` was scratch
    (deterministic mode), its stage and `dpooled`'s, which is formed from it, are checked in the other mode only.
    mixed: (ids [B/2, L], soft [B/2, L, V]) of a mixed batch; the state then holds the ids pass in its first half of the rows."""
    td, F, Fp, MR, n = TD[case.dtype], case.F, case.Fp, case.MR, len(case.fs)
    bf = case.dtype == "bf16"
    emit = _Emit(ws, rep)

    def grad(i, name, ref, mag, nsum):
        if grads is None:
            return
        if i < 0:
            i += len(P)
        c0 = G0[i].double() if G0 is not None else torch.zeros_like(ref)
        ref, bound = ref.reshape(c0.shape) + c0, sum_bound(nsum, mag.reshape(c0.shape) + c0.abs(), None)
        if rep is None:
            grads[i] = ref.float()
        else:
            rep.check(name, grads[i], ref, bound)

    dl = X["d_logits"].float()
    # 1. out2logits: dfeat = dlogit * w, one f32 product
    w = P[-2].float().reshape(-1)
    emit.same("dfeat", (dl[:, None] * w[None, :]).to(td), cols=OUT)
    emit.pad_zero("dfeat", OUT)                                          # (the kernel's g * 0: zero of either sign)
    feat = st["feat"].double()
    grad(-2, "o2l_w", dl.double() @ feat, dl.double().abs() @ feat.abs(), MR)
    grad(-1, "o2l_b", dl.double().sum(), dl.double().abs().sum(), MR)
    # 2. feature2out
    dfe, W = ws["dfeat"].double(), img["f2o_w"].double()
    if not det:
        emit("dydrop", dfe @ W, sum_bound(OUT_PAD, dfe.abs() @ W.abs(), None), torch.float32)
    y = st["ydrop"][:, :F].double()
    grad(-4, "f2o_w", dfe[:, :OUT].t() @ y, dfe[:, :OUT].abs().t() @ y.abs(), MR)
    grad(-3, "f2o_b", dfe[:, :OUT].sum(0), dfe[:, :OUT].abs().sum(0), MR)
    # 3. highway backward: dy = dydrop keep scale; dh = dy (sg (1 - sg) (relu(h) - x) + sg [h > 0]); dpooled = dy (1 - sg) + dh W
    x, h = st["pooled"][:, :F].double(), st["hpre"][:, :F].double()
    sg = torch.sigmoid(h)
    W = img["hw_w"][:F, :F].double()
    if not det:
        scale = 1.0 / (1.0 - DROP_P) if X["train"] else 1.0
        dy = ws["dydrop"][:, :F].double() * scale * (st["keep"][:, :F].double() if X["train"] else 1.0)
        pos = (h > 0).double()
        dh_ref = dy * (sg * (1 - sg) * (torch.relu(h) - x) + pos * sg)
        dh_bnd = 8 * U * dy.abs() * (sg * (1 + sg) * (torch.relu(h) + x.abs()) + pos * sg)
        emit("dh", dh_ref, dh_bnd + _r(dh_ref, bf), td, cols=F)
        emit.pad_zero("dh", F)
        dh = ws["dh"][:, :F].double()
        direct = dy * (1 - sg)
        emit("dpooled", direct + dh @ W, 8 * U * dy.abs() * (1 + sg) + sum_bound(Fp, dh.abs() @ W.abs() + direct.abs(), None), torch.float32, cols=F)
        emit.pad_zero("dpooled", F)
    dh = ws["dh"][:, :F].double()
    grad(-6, "hw_w", dh.t() @ x, dh.abs().t() @ x.abs(), MR)
    grad(-5, "hw_b", dh.sum(0), dh.abs().sum(0), MR)
    # 4. convolution / max-pool backward from the saved argmax and the relu gate
    skip = None
    if mut == "wgrad_block_row_omitted":
        if select(case)[2] == "lds":                                     # the LDS kernel's block row y serves the captions b = y (mod rows_y)
            skip = (torch.arange(MR) // case.R != case.B - 1).long()
        else:                                                            # the general kernel's the rows m with (m / 4) % gy == y
            gy = min(64, -(-MR // 32))
            skip = 1 - ((torch.arange(MR) // 4) % gy == gy - 1).long()
    demb_ref, demb_mag, banks = conv_grads(case, P, st, ws["dpooled"], skip)
    emit("demb", demb_ref, sum_bound(F, demb_mag, demb_ref, bf), td)
    for k, (dw, dwm, db, dbm) in enumerate(banks):
        grad(1 + 2 * k, f"conv_w.{k}", dw, dwm, MR)
        grad(2 + 2 * k, f"conv_b.{k}", db, dbm, MR)
    # 5. embedding: scatter (ids), demb^T inp (soft), or both halves of a mixed batch
    demb = ws["demb"].double()
    rowsBL = case.B * case.L
    ids, soft = (X["ids"], X["soft"]) if mixed is None else mixed
    ge, gm = torch.zeros(case.De, case.V, dtype=torch.float64), torch.zeros(case.De, case.V, dtype=torch.float64)
    lo = 0
    if ids is not None:
        lo = ids.numel()
        ge.index_add_(1, ids.reshape(-1), demb[:lo].t())
        gm.index_add_(1, ids.reshape(-1), demb[:lo].abs().t())
    if soft is not None:
        a = soft.reshape(-1, case.V).double()
        ge += demb[lo:].t() @ a
        gm += demb[lo:].abs().t() @ a.abs()
    grad(0, "emb_w", ge, gm, rowsBL)
    if d_inp is not None or (rep is None and mixed is None and soft is not None):
        We = img["emb"].double()
        ref, bound = demb @ We, sum_bound(case.De, demb.abs() @ We.abs(), demb @ We, bf)
        if rep is None:
            ws["d_inp"] = ref.to(td)
        else:
            rep.check("d_inp", d_inp.reshape(-1, case.V), ref, bound)


def check_images(case, P, shadow, rep):
    """The shadow images equal master.to(dtype) zero-padded; hw_w_t is the exact transpose (bf16 mode keeps one)."""
    want = images(case, P)
    rep.bits("hw_w image", shadow["hw_w"], want["hw_w"])
    rep.bits("f2o_w image", shadow["f2o_w"], want["f2o_w"])
    if shadow.get("emb") is not None:
        rep.bits("emb image", shadow["emb"], want["emb"])
    if shadow.get("hw_w_t") is not None:
        rep.bits("hw_w_t image", shadow["hw_w_t"], shadow["hw_w"].t().contiguous())
