"""The LSTM decoder's teacher-forced path (csrc/teacher_forced.hip: gic_decoder_forward_tf / _tf_bwd and their scheduled-sampling and
dropout forms) stage by stage: the case table, a restatement of the route selection, the fp64 reference of every stage, the per-element
bounds and the checker behind tests/test_decoder_tf_cases.py (no GPU) and tests/test_gpu_decoder_tf_stages.py (every case on the GPU).
Nothing here touches the GPU.

The contract is that of tests/decoder_cases.py, whose rules are imported, not copied: every stage is checked against an fp64 reference
formed from the buffers the device itself wrote upstream of it, so errors do not compound, a flipped pick excuses nothing at the next
step and bf16 is checked as tightly as f32.  `run_forward` / `run_backward` walk the stages in order; with a Report they compare the
buffers given, without one they FILL them from the references in storage precision (what the checker's self-test mutates).

Bounds: every one is a rule of tests/decoder_cases.py (sum_bound, the gate / c / h rules of cell_forward, gumbel, y, out, dlogits, the
dgates chain of cell_backward with its carried dc bound, bit equality).  No constant is measured here.  Two details:
  out   the teacher-forced epilogue (gumbel_softmax_rows: the 256-thread gumbel_softmax_argmax_kernel over B * Tmax rows) rounds a bf16
        `out` once: one r, not the fused route's two.
  libm  that kernel calls logf / expf in both dtypes: K_LIBM applies, the fast-intrinsic constants do not.
What the path leaves behind decides where a rule is applied.  With pretrain = 0 the kernel writes y = (o + b + g) T back over the f32
logits workspace and forms the softmax from those stored values (every thread re-reads what it wrote itself), so after the call the
workspace holds y, not the logits: stage `y` holds it to the y rule (the product's bound, the Gumbel bound with u indexed
[B, Tmax, V], the two additions and the product with T), and `out` is the softmax of the DEVICE's y -- the `out` rule with dy = 0:
p u (2 K_LIBM (1 + |x|) + V + tiles + 16) + r.  With pretrain = 1 (and under scheduled sampling) the workspace keeps the logits: stage
`logits` is the sum rule over H from the device's hout (hdrop under dropout), `out` the same reference + r.
`dhout` is checked in its final state against the product's reference: inside the lengths the sum rule over V (under dropout, kept
elements: the product times s = 1 / (1 - p), one more rounding), past the lengths (and at dropped elements) reference 0 with bound 0,
which the checker takes as exact equality.  The same holds for dgates and the carried dc at padded (row, step) pairs -- every factor of
every term is a stored 0, so the chain rule's own reference and bound are 0 there -- and for the rows of d_embed no caption names.

Scheduled sampling: the coin is exact (coin_u < prob in f32, live positions only); a replaced position's pick must have an fp64
score (the logit from the device's hout / hdrop, + the fp64 Gumbel value for pick = sample) within twice the row's largest bound of the
row maximum -- every pick, no position excluded, a near tie admits the tied candidates only -- and everything downstream (inputs, the x
row of the next slot, the next step) is formed from the DEVICE's pick."""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests import decoder_cases as D
from tests import gen_dropout_oracle as GD
from tests import philox_ref as PR
from tests.decoder_cases import DXH_FILL, K_LIBM, R_OUT  # noqa: F401  (DXH_FILL: what the GPU module fills dxh with)
from tests.disc_cases import TD, U, U8, Report, sum_bound  # noqa: F401

TEMPERATURE = D.TEMPERATURE
DROP_P = 0.3
SEED = 404
PHILOX_SEED = 0x1234_5678_9ABC_DEF0
DROP_SEED = 0x0FED_CBA9_8765_4321

ORDER = ("slot0", "xrows", "gates", "c", "h", "pad gates", "pad state", "h copies", "hout", "hdrop", "logits", "y", "replaced", "pick", "inputs",
         "ss tail", "out", "h_n", "c_n", "untouched",
         "dlogits", "dhout", "d_w_out", "d_b_out", "dgates", "dc", "dxh", "dxh keep", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "d_b_ih == d_b_hh",
         "d_features", "d_embed")
FORWARD = ORDER[:ORDER.index("dlogits")]


class Case(NamedTuple):
    name: str
    B: int
    T: int                        # steps the state is allocated for: caption length + 1 (the entry point's dims.L)
    V: int
    E: int
    H: int
    NL: int
    lengths: Tuple[int, ...]
    dtype: str                    # "f32" | "bf16"
    route: str                    # route_str(select(case)), pinned in tests/test_decoder_tf_cases.py
    gemm: str                     # what the library's GEMM selection answers for the case's products (the test's probe), pinned there too

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    @property
    def Lc(self):
        return self.T - 1

    @property
    def Tmax(self):
        return max(self.lengths)

    def din(self, l):
        return self.E if l == 0 else self.H

    def ldx(self, l):
        return self.din(l) + self.H

    @property
    def nblk(self):
        return -(-self.V // D.KTILE)


class Mode(NamedTuple):
    pretrain: bool = True
    ss: Optional[Tuple[float, str]] = None       # scheduled sampling (prob, pick); the call is then pretrain = 1, T = 1
    drop: float = 0.0
    philox: bool = False                         # the noise of the epilogue / the keep mask drawn on the device (host replica: philox_ref)
    det: bool = False                            # the backward runs in deterministic mode

    @property
    def id(self):
        s = "pretrain" if self.pretrain and not self.ss else ("adv" if not self.ss else f"ss{self.ss[0]:g}-{self.ss[1]}")
        return s + ("-drop" if self.drop else "") + ("-philox" if self.philox else "") + ("-det" if self.det else "")


def view_case(case, pretrain):
    """The Tmax view the backward runs on, as a case of tests/decoder_cases.py (L = Tmax)."""
    return D.Case(case.name, case.B, case.Tmax, case.V, case.E, case.H, case.NL, case.dtype, "", pretrain=pretrain)


def select(case):
    """The routes gic_decoder_forward_tf / _ss / _tf_bwd take for a case, restated."""
    c = case
    s = D.select(view_case(c, False))
    step_ok = c.V >= 4 and c.V % 4 == 0 and c.E % 8 == 0 and c.H % 8 == 0 and c.nblk <= 1024           # decoder_fused_rows
    scatter = "none" if c.Tmax == 1 else ("rows" if c.E % 4 == 0 and c.ldx(0) % 4 == 0 else "scalar")   # embed_scatter_time
    nv = 4 if c.dtype == "f32" else 8
    return {"bwd": s["bwd"], "softmax_bwd": s["softmax_bwd"], "scatter": scatter,
            "ss_logits": "fused" if c.B <= D.MAX_ROWS and step_ok else "gemm",                        # teacher_forced()'s ss_fused
            "drop": ("vec" if c.H % nv == 0 else "scalar") + "/" + ("vec" if c.H % 4 == 0 else "scalar"),   # hidden_dropout_fwd / _bwd
            "view": f"{c.Tmax}/{c.T}"}


def route_str(s):
    return f"bwd={s['bwd']} softmax_bwd={s['softmax_bwd']} scatter={s['scatter']} ss_logits={s['ss_logits']} drop={s['drop']} Tmax/T={s['view']}"


def _both(name, B, T, V, E, H, NL, lengths, r32, r16, g32, g16):
    assert len(lengths) == B and 1 <= min(lengths) and max(lengths) <= T
    return [Case(name, B, T, V, E, H, NL, tuple(lengths), "f32", r32, g32), Case(name, B, T, V, E, H, NL, tuple(lengths), "bf16", r16, g16)]


ROWS_LENGTHS = tuple(1 + (7 * b + 1) % 9 for b in range(40))            # ragged, 1..9
WIDE_LENGTHS = tuple(1 + (5 * b + 2) % 9 for b in range(64))
_S1 = "gate=1 wgrad=unfolded out=unfolded proj=64"
CASES = (
    # fused BPTT over two layers (h_up of padded rows), Tmax = T, a row of length 1; bf16: d_w_out folds its bias sum, the recurrent weight
    # gradients (din = 16 is off the 64-wide tile) do not
    _both("tf-base", 5, 7, 64, 16, 32, 2, (4, 7, 1, 6, 3),
          "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=7/7",
          "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=7/7",
          "gate=1,1 wgrad=unfolded,unfolded out=unfolded proj=64", "gate=1,1 wgrad=unfolded,unfolded out=folded proj=64")
    # Tmax = 5 < T: the Tmax view, ids_stride = 6 != Tmax - 1, slots above Tmax untouched
    + _both("tf-short", 5, 7, 64, 16, 32, 2, (4, 5, 1, 5, 3),
            "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=5/7",
            "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=5/7",
            "gate=1,1 wgrad=unfolded,unfolded out=unfolded proj=64", "gate=1,1 wgrad=unfolded,unfolded out=folded proj=64")
    # H % 8 != 0: generic BPTT; V % 4 != 0: the scalar softmax backward; the GEMM route of ss_step_logits; scalar dropout in bf16
    + _both("tf-generic", 3, 6, 50, 12, 20, 1, (1, 6, 4),
            "bwd=generic softmax_bwd=scalar scatter=rows ss_logits=gemm drop=vec/vec Tmax/T=6/6",
            "bwd=generic softmax_bwd=scalar scatter=rows ss_logits=gemm drop=scalar/vec Tmax/T=6/6", _S1, _S1)
    # nothing aligned: the scalar embedding scatter (ldx % 4 != 0), unfolded weight gradients + colsum in both dtypes
    + _both("tf-odd", 3, 5, 51, 10, 21, 2, (5, 2, 3),
            "bwd=generic softmax_bwd=scalar scatter=scalar ss_logits=gemm drop=scalar/scalar Tmax/T=5/5",
            "bwd=generic softmax_bwd=scalar scatter=scalar ss_logits=gemm drop=scalar/scalar Tmax/T=5/5",
            "gate=1,1 wgrad=unfolded,unfolded out=unfolded proj=64", "gate=1,1 wgrad=unfolded,unfolded out=unfolded proj=64")
    # Tmax = 1 < T: no scatter rows, d_embed all zero, dc_zero at the only step
    + _both("tf-len1", 4, 4, 16, 8, 8, 1, (1, 1, 1, 1),
            "bwd=fused softmax_bwd=vec8 scatter=none ss_logits=fused drop=vec/vec Tmax/T=1/4",
            "bwd=fused softmax_bwd=vec5 scatter=none ss_logits=fused drop=vec/vec Tmax/T=1/4", _S1, "gate=1 wgrad=unfolded out=folded proj=64")
    # T = 1: caps is null
    + _both("tf-nocaps", 1, 1, 16, 8, 8, 1, (1,),
            "bwd=fused softmax_bwd=vec8 scatter=none ss_logits=fused drop=vec/vec Tmax/T=1/1",
            "bwd=fused softmax_bwd=vec5 scatter=none ss_logits=fused drop=vec/vec Tmax/T=1/1", _S1, "gate=1 wgrad=unfolded out=folded proj=64")
    # ldx = 512: the bf16 gate GEMM splits K four ways in the plain call (and must not under scheduled sampling); din = 256 sits on a
    # tile boundary: dW_ih | dW_hh is one product with both bias sums folded
    + _both("tf-splitk", 4, 3, 64, 256, 256, 1, (3, 1, 2, 3),
            "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=3/3",
            "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=3/3", _S1, "gate=4 wgrad=folded out=folded proj=64")
    # 16 vocabulary tiles of 64; the fused vocab_step_logits under scheduled sampling; Tmax = 6 < T
    + _both("tf-tiles", 5, 7, 1000, 16, 32, 2, (5, 3, 6, 2, 4),
            "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=6/7",
            "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=6/7",
            "gate=1,1 wgrad=unfolded,unfolded out=unfolded proj=64", "gate=1,1 wgrad=unfolded,unfolded out=folded proj=64")
    # B * Tmax = 360 rows: the projection is 6 x 5 tiles, the weight gradients sum over six K tiles; E = 64 puts din on a tile boundary:
    # the merged dW_ih | dW_hh product with folded bias sums
    + _both("tf-rows", 40, 9, 264, 64, 64, 1, ROWS_LENGTHS,
            "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=9/9",
            "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=9/9", _S1, "gate=1 wgrad=folded out=folded proj=64")
    # 576 rows by 4872 columns: the projection leaves the 64-wide GEMM tile (195 tiles of 128 x 128); bf16: d_hout splits K = V 16 ways,
    # d_w_out folds db_out over 77 tiles
    + _both("tf-wide", 64, 9, 4872, 64, 64, 1, WIDE_LENGTHS,
            "bwd=fused softmax_bwd=vec8 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=9/9",
            "bwd=fused softmax_bwd=vec5 scatter=rows ss_logits=fused drop=vec/vec Tmax/T=9/9",
            "gate=1 wgrad=unfolded out=unfolded proj=128", "gate=1 wgrad=folded out=folded proj=128")
)

_PLAIN = (Mode(True), Mode(False))
_SS = tuple(Mode(True, (p, pick)) for p in (0.5, 1.0) for pick in ("sample", "argmax"))
_EXTRA = {
    "tf-base": (Mode(False, philox=True), Mode(False, det=True)) + _SS
               + (Mode(False, drop=DROP_P), Mode(True, drop=DROP_P, philox=True), Mode(True, (0.5, "sample"), DROP_P), Mode(True, (1.0, "argmax"), DROP_P, philox=True)),
    "tf-odd": (Mode(False, det=True),),
    "tf-generic": _SS + (Mode(False, drop=DROP_P), Mode(True, drop=DROP_P, philox=True), Mode(True, (0.5, "sample"), DROP_P), Mode(True, (1.0, "argmax"), DROP_P, philox=True)),
    "tf-tiles": _SS, "tf-splitk": _SS, "tf-nocaps": _SS,
}
RUNS = tuple((c, m) for c in CASES for m in _PLAIN + _EXTRA.get(c.name, ()))


def run_id(run):
    return f"{run[0].id}-{run[1].id}"


# ---------------------------------------------------------------------------------------------------------------- data
def data(case, mode=Mode()):
    """The parameters and inputs every test of a case uses.  The draws are those of the mode: explicit uniforms, or (mode.philox) the host
    replica of what the device draws (tests/philox_ref.py: the epilogue's stream 0x7466 at the flat index row * V + v; the dropout map of
    tests/gen_dropout_oracle.py)."""
    c = case
    gen = torch.Generator().manual_seed(SEED)
    P = D.make_params(c, gen)
    rnd = lambda *shape: torch.rand(*shape, generator=gen)
    X = {"features": torch.randn(c.B, c.E, generator=gen), "caps": torch.randint(0, c.V, (c.B, c.Lc), generator=gen),
         "lengths": torch.tensor(c.lengths, dtype=torch.int32), "u": rnd(c.B, c.Tmax, c.V), "d_pred": torch.randn(c.B, c.Tmax, c.V, generator=gen),
         "T": TEMPERATURE, "coin_u": rnd(c.B, c.Lc), "ss_noise": rnd(c.Lc, c.B, c.V), "keep_u": rnd(c.B, c.Tmax, c.H)}
    if c.name == "tf-base":                                      # out-of-range ids in a row that is live at every step: clamped to 0 and V - 1
        X["caps"][1, 0], X["caps"][1, 2] = -3, c.V + 5
    if mode.philox:
        X["u"] = torch.from_numpy(np.ascontiguousarray(PR.tf_u(PHILOX_SEED, c.B, c.Tmax, c.V)))
        X["keep_u"] = torch.from_numpy(np.ascontiguousarray(GD.dropout_u(DROP_SEED, c.B, c.Tmax, c.H)))
    if mode.ss:
        X["T"] = 1.0
    return P, X


def images(case, P):
    return D.images(case, P)


def new_state(case):
    """The state as DecoderEngine.alloc_state(B, T) shapes it and every buffer a forward call writes (CPU), NaN / -7 beforehand.  `hout`
    is the flat allocation of B * T * H values, of which the call uses the first B * Tmax * H as [B, Tmax, H]."""
    c, td, nan = case, TD[case.dtype], float("nan")
    return {"xh": [torch.full((c.T + 1, c.B, c.ldx(l)), nan, dtype=td) for l in range(c.NL)],
            "gates": [torch.full((c.T, c.B, 4 * c.H), nan) for _ in range(c.NL)],
            "c": [torch.full((c.T + 1, c.B, c.H), nan) for _ in range(c.NL)],
            "hout": torch.full((c.B * c.T * c.H,), nan, dtype=td), "logits_ws": torch.full((c.B * c.Tmax, c.V), nan),
            "out": torch.full((c.B, c.Tmax, c.V), nan, dtype=td), "h_n": torch.full((c.NL, c.B, c.H), nan), "c_n": torch.full((c.NL, c.B, c.H), nan),
            "hdrop": torch.full((c.B, c.Tmax, c.H), nan, dtype=td), "inputs": torch.full((c.B, c.Lc), -7, dtype=torch.int64),
            "replaced": torch.full((c.B, c.Lc), -7, dtype=torch.int32)}


def new_ws(case):
    return D.new_ws(view_case(case, False))


def new_grads(case, P):
    return D.new_grads(case, P)


def hout_view(case, st):
    c = case
    return st["hout"][:c.B * c.Tmax * c.H].view(c.B, c.Tmax, c.H)


def keep_mask(mode, X):
    return GD.keep_of(X["keep_u"], mode.drop) if mode.drop else None


def live_mask(case, X):
    """[B, Tmax]: t < lengths[b]."""
    return torch.arange(case.Tmax)[None, :] < X["lengths"].long()[:, None]


# ---------------------------------------------------------------------------------------------------------------- forward
def run_forward(case, mode, P, img, X, st, rep=None, mut=None, gaps=None):
    """Walk the forward stages over `st` (new_state's keys).  rep: check; None: fill.  `mut`: a mutation of the fill.  gaps: a list that
    receives the fp64 top-2 score gap of every replaced position (scheduled sampling, fill)."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, T, V, E, H, NL, Lc, Tmax = c.B, c.T, c.V, c.E, c.H, c.NL, c.Lc, c.Tmax
    lens, caps = X["lengths"].long(), X["caps"]
    pretrain = mode.pretrain or mode.ss is not None
    Tm = float(X["T"])
    hout, logits = hout_view(c, st), st["logits_ws"].view(B, Tmax, V)
    keep = keep_mask(mode, X)
    hproj = st["hdrop"] if mode.drop else hout
    Wout, bout = img["wout"].double(), P[-1].double()

    def emit(stage, view, ref, bound):
        if rep is None:
            view.copy_(ref.to(view.dtype))
        else:
            rep.check(stage, view, ref, bound)

    def same(stage, view, want):
        if rep is None:
            view.copy_(want)
        else:
            rep.bits(stage, view, want)

    zero = lambda stage, view: same(stage, view, torch.zeros(view.shape, dtype=view.dtype))
    # slot 0 and c_0 of every layer: zeros; the x rows: features, then the teacher's embedding rows for EVERY slot below T
    for l in range(NL):
        zero("slot0", st["xh"][l][0][:, c.din(l):])
        zero("slot0", st["c"][l][0])
    teacher = D.clamp_ids(caps, V)
    if rep is None:
        st["xh"][0][0][:, :E] = X["features"].to(td)
        for t in range(1, T):
            st["xh"][0][t][:, :E] = P[0][teacher[:, t - 1]].to(td)
    lref_all, lb_all = torch.zeros(B, Tmax, V, dtype=torch.float64), torch.zeros(B, Tmax, V, dtype=torch.float64)
    for t in range(Tmax):
        live = t < lens
        pad = ~live
        for l in range(NL):
            din = c.din(l)
            a, W, bs = st["xh"][l][t].double(), img["wcat"][l].double(), img["bsum"][l].double()
            g_t, c_prev, c_next = st["gates"][l][t], st["c"][l][t], st["c"][l][t + 1]
            h_prev, hv = st["xh"][l][t][:, din:], st["xh"][l][t + 1][:, din:]
            top = l + 1 == NL
            up = hout[:, t] if top else st["xh"][l + 1][t][:, :H]
            if rep is None:
                tg, tc, th = torch.zeros(B, 4 * H), torch.zeros(B, H), torch.zeros(B, H, dtype=td)
                D.cell_forward(emit, bf, a, W, bs, tg, c_prev, tc, th)
                hold = pad & (mut != "pad_advance")
                g_t.copy_(torch.where(pad[:, None] & (mut != "pad_gates"), torch.zeros_like(tg), tg))
                c_next.copy_(torch.where(hold[:, None], c_prev, tc))
                hv.copy_(torch.where(hold[:, None], h_prev, th))
                up.copy_(torch.where(pad[:, None] & (mut != "pad_hout"), torch.zeros_like(hv), hv) if top else hv)
            else:
                D.cell_forward(emit, bf, a[live], W, bs, g_t[live], c_prev[live], c_next[live], hv[live])
                rep.exact("pad gates", g_t[pad] == 0, "of the gates of a padded step are not zero")
                rep.bits("pad state", c_next[pad], c_prev[pad], "of a padded row's c moved")
                rep.bits("pad state", hv[pad], h_prev[pad], "of a padded row's h moved")
                if top:
                    rep.bits("hout", up[live], hv[live])
                    rep.exact("hout", up[pad] == 0, "of an hout row past its length are not zero")
                else:
                    rep.bits("h copies", up, hv)
        if rep is None and mut == "hout_stride_T" and t == Tmax - 1:             # rows T * H apart instead of Tmax * H
            rows = hout.clone()
            st["hout"].fill_(float("nan"))
            st["hout"].view(B, T, H)[:, :Tmax] = rows
        # the dropped rows of step t, then its logits (scheduled sampling forms them here, the plain call after the loop: the same rule)
        if mode.drop:
            want = GD.apply(hout[:, t].contiguous(), keep[:, t], mode.drop)
            if rep is None and mut == "hdrop_scaled":
                want = GD.apply(hout[:, t].contiguous(), torch.ones_like(keep[:, t]), mode.drop)
            same("hdrop", hproj[:, t], want)
        hp = hproj[:, t].double()
        lref = hp @ Wout.t() + bout
        lb = sum_bound(H, hp.abs() @ Wout.abs().t() + bout.abs(), None)
        lref_all[:, t], lb_all[:, t] = lref, lb
        if pretrain:
            emit("logits", logits[:, t], lref, lb)
        else:
            u = X["u"][:, t] if mut != "u_tbv" else X["u"].reshape(Tmax, B, V)[t]
            g, dg = D.gumbel(u, K_LIBM)
            y = (lref + g) * Tm
            emit("y", logits[:, t], y, (lb + dg + U * (lref.abs() + (lref + g).abs())) * abs(Tm) + U * y.abs())
        if mode.ss and t + 1 < Tmax:
            prob, pick = mode.ss
            want_rep = (X["coin_u"][:, t] < torch.tensor(prob, dtype=torch.float32)) & (t + 1 < lens)
            score, sb = lref, lb
            if pick == "sample":
                g, dg = D.gumbel(X["ss_noise"][t], K_LIBM)
                score = lref + g
                sb = lb + dg + U * score.abs()
            smax, bmax = score.max(1).values, sb.max(1).values
            if rep is None:
                top2 = score.topk(2, 1)
                if gaps is not None:
                    gaps += (top2.values[:, 0] - top2.values[:, 1])[want_rep].tolist()
                best = top2.indices[:, 1] if mut == "pick_second" else D.first_argmax(score)
                st["inputs"][:, t] = torch.where(want_rep, best, teacher[:, t])
                st["replaced"][:, t] = want_rep.to(torch.int32)
                if mut == "replaced_past":
                    st["replaced"][:, t] = (want_rep | (t + 1 >= lens)).to(torch.int32)
                if mut != "xrow_teacher":
                    st["xh"][0][t + 1][:, :E] = P[0][st["inputs"][:, t]].to(td)
            else:
                inp = st["inputs"][:, t]
                rep.exact("replaced", st["replaced"][:, t] == want_rep.to(torch.int32), "of `replaced` are not coin < prob at a live position")
                ok = (inp >= 0) & (inp < V)
                at = score.gather(1, inp.clamp(0, V - 1)[:, None])[:, 0]
                rep.exact("pick", ~want_rep | (ok & (at >= smax - 2 * bmax)), "picks are not within twice the bound of the row maximum")
                rep.exact("inputs", want_rep | (inp == teacher[:, t]), "of `inputs` are not the teacher's clamped id")
    if mode.ss and Lc > Tmax - 1:                             # the positions no step is fed from
        same("ss tail", st["inputs"][:, Tmax - 1:], caps[:, Tmax - 1:])
        zero("ss tail", st["replaced"][:, Tmax - 1:])
    if rep is not None:                                       # the x rows, from the device's own inputs
        ids = D.clamp_ids(st["inputs"], V) if mode.ss else teacher
        rep.bits("xrows", st["xh"][0][0][:, :E], X["features"].to(td))
        for t in range(1, T):
            rep.bits("xrows", st["xh"][0][t][:, :E], P[0][ids[:, t - 1]].to(td))
    # the epilogue
    if pretrain:
        emit("out", st["out"], lref_all, lb_all + (U8 * lref_all.abs() if bf else 0.0))
    else:
        y = logits.double()                                   # the device's y
        p = torch.softmax(y, 2)
        x = (y - y.max(2, keepdim=True).values).abs()
        emit("out", st["out"], p, p * U * (2 * K_LIBM * (1 + x) + V + c.nblk + 16) + R_OUT(p, bf))
    # h_n / c_n: slot Tmax, where every row's state at its own last step sits
    rows = torch.arange(B)
    for l in range(NL):
        slot = T if (rep is None and mut == "hn_slot_T") else Tmax
        same("h_n", st["h_n"][l], st["xh"][l][slot][:, c.din(l):].float())
        same("c_n", st["c_n"][l], st["c"][l][slot])
        if rep is not None:
            rep.bits("h_n", st["h_n"][l], st["xh"][l][lens, rows][:, c.din(l):].float(), "differ from the row's h at its own last step")
            rep.bits("c_n", st["c_n"][l], st["c"][l][lens, rows], "differ from the row's c at its own last step")
    if rep is not None:
        check_untouched(case, st, rep)


def check_untouched(case, st, rep):
    """What no teacher-forced call writes: slot T's x row, the h columns and cells of the slots above Tmax, the upper layers' x columns and
    the gates from slot Tmax on, hout behind its first B * Tmax * H values."""
    c = case
    for l in range(c.NL):
        din = c.din(l)
        parts = [st["xh"][l][c.Tmax + 1:, :, din:], st["c"][l][c.Tmax + 1:], st["gates"][l][c.Tmax:],
                 st["xh"][0][c.T][:, :c.E] if l == 0 else st["xh"][l][c.Tmax:, :, :din]]
        for p in parts:
            rep.exact("untouched", torch.isnan(p), "of the slots above Tmax were written")
    rep.exact("untouched", torch.isnan(st["hout"][c.B * c.Tmax * c.H:]), "behind hout's [B, Tmax, H] view were written")


# ---------------------------------------------------------------------------------------------------------------- backward
def run_backward(case, mode, P, img, X, st, ws, grads, rep=None, mut=None):
    """Walk the backward stages (gic_decoder_forward_tf_bwd / _drop_bwd on the Tmax view).  st: the forward's buffers; ws: new_ws's keys
    (Tmax steps); grads: new_grads' list."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, V, E, H, NL, Tmax = c.B, c.V, c.E, c.H, c.NL, c.Tmax
    BL = B * Tmax
    pretrain = mode.pretrain or mode.ss is not None
    vc = view_case(c, pretrain)
    hproj = st["hdrop"] if mode.drop else hout_view(c, st)
    stv = {"xh": [x[:Tmax + 1] for x in st["xh"]], "gates": [g[:Tmax] for g in st["gates"]], "c": [x[:Tmax + 1] for x in st["c"]],
           "hout": hproj, "out": st["out"], "ids": None}
    Xv = {"d_out": X["d_pred"], "T": X["T"]}
    if not pretrain:
        D.run_backward(vc, P, img, Xv, stv, ws, grads, rep, only={"dlogits"})
        dlog = ws["dlogits"].double().reshape(BL, V)
    else:
        dlog = X["d_pred"].to(td).double().reshape(BL, V)
    # dhout in its final state: the product inside the lengths (kept elements: times s, one more rounding), exact zeros elsewhere
    W = img["wout"].double()
    ref, bound = dlog @ W, sum_bound(V, dlog.abs() @ W.abs(), None)
    m = live_mask(c, X)[:, :, None].expand(B, Tmax, H)
    if mode.drop:
        s = float(GD.scale(mode.drop))
        ref = ref * s
        bound = bound * s + U * ref.abs()
        m = m & keep_mask(mode, X)
    m = m.reshape(BL, H)
    if not (rep is None and mut == "dhout_unmasked"):
        ref, bound = torch.where(m, ref, torch.zeros_like(ref)), torch.where(m, bound, torch.zeros_like(bound))
    if rep is None:
        ws["dhout"].view(BL, H).copy_(ref)
    else:
        rep.check("dhout", ws["dhout"].view(BL, H), ref, bound)
    D.run_backward(vc, P, img, Xv, stv, ws, grads, rep, state_grads=False, det=mode.det,
                   only={"d_w_out", "d_b_out", "dgates", "dc", "dxh", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "d_features"})
    if rep is not None:      # (the chain's own reference and bound are 0 at a padded pair; said once more on its own)
        for l in range(NL):
            rep.exact("dgates", ws["dgates"][l][padded_pairs(c, X)] == 0, "of dgates at a padded (step, row) pair are not zero")
    # d_embed: the rows (t, b), 1 <= t < Tmax, through the ids the forward was fed (rows Lc apart)
    ids = st["inputs"] if mode.ss else X["caps"]
    ge, gm = torch.zeros(V, E, dtype=torch.float64), torch.zeros(V, E, dtype=torch.float64)
    if Tmax > 1:
        used = ids[:, :Tmax - 1]
        if rep is None and mut == "ids_stride_tm1":
            used = ids.reshape(-1)[:B * (Tmax - 1)].view(B, Tmax - 1)
        idx = D.clamp_ids(used, V).t().reshape(-1)                              # (t - 1, b) order
        src = ws["dxh"][0][1:Tmax, :, :E].double().reshape(-1, E)
        ge.index_add_(0, idx, src)
        gm.index_add_(0, idx, src.abs())
    if rep is None:
        grads[0].copy_(ge)
    else:
        rep.check("d_embed", grads[0], ge, sum_bound(B * max(Tmax - 1, 1), gm, None))


def padded_pairs(case, X):
    """[Tmax, B]: the (step, row) pairs past a caption's length."""
    return ~live_mask(case, X).t()
