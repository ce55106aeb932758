"""The visual-attention caption decoder (csrc/attention.hip, csrc/attn_beam.hip in its packed K = 1 form, csrc/attn_rollout.hip) stage
by stage: the case table, a restatement of the launch geometry, the fp64 reference of every stage, the per-element bounds and the
checker behind tests/test_attn_cases.py (no GPU) and tests/test_gpu_attn_stages.py (every case on the GPU).  Nothing here touches the
GPU.

Every stage is checked against an fp64 reference formed from the buffers the kernels themselves wrote upstream of it (`fproj`, `hproj`,
`alpha`, `xh` with its z columns, `gates`, `c`, `hout`, `dgates`, `dhproj`, `dfproj`, `dwa_rows`, `dx`, the roll-out's workspace), so
errors do not compound and bf16 is as tightly checkable as f32.  `run_forward` / `run_backward` / `run_rollout` walk the stages in
order; with a Report they compare the buffers given, without one they FILL them from the references in storage precision (what the
checker's self-test mutates).  The cell (gates, c, h, d_gates) and the output layer's backward (dlogits, dhout, d_w_out, d_b_out) are
the rules of tests/decoder_cases.py, imported, not copied.  `part`, `out` and `ids` of the forward are the LSTM decoder's vocab_step
and sample_finish: their references are woven into decoder_cases.run_forward and do not apply without copying, so they stay with
tests/test_gpu_decoder_stages.py (the kernels) and tests/test_gpu_attention.py (their use here); `out` and `ids` enter here as the
device wrote them (the x rows and the softmax backward are formed from them).

Bounds, per element, with the conventions of tests/decoder_cases.py: u = 2^-24, r = 2^-8 |ref| where the output is bf16, the 2^-110
floor on every non-zero bound, "sum" = (n + 4) u sum |terms| + r in any order.  All derived, none fitted; K_TANH and K_LIBM are the
constants of tests/decoder_cases.py (the same tanhf / expf); the f32 division is correctly rounded in this build (no fast-math flag)
and is one of the 16 roundings the softmax rule counts.
  fproj     sum over C of fmap W_f^T + b_f (+ r)
  hproj     sum over H of h_{t-1} W_h^T; exactly 0 where h_{t-1} is the zero state
  alpha     e_i = sum_j w_a_j tanh(fp_ij + hp_j) is not saved: de_i = sum_j |w_a_j| (u |fp + hp| + K_TANH u |th|) + the sum rule over A;
            |d alpha| <= alpha (expm1(2 max de) + u (2 K_LIBM (1 + |x|) + P + 16)), x = e - max e (the `out` rule of decoder_cases);
            where x < -106 - 2 max de the device's expf argument is below -104 and its result exactly 0: reference 0, bound 0.
  alpha sum each row sums to 1 within P u + the sum of its bounds
  z         sum over P of alpha_i fmap_i from the device's alpha (+ r)
  dz        d_gates W_z, sum over 4H; overwritten (re-zeroed behind its reader), so carried in fp64 with its bound
  dalpha    dz . fmap_i (+ d_alphas): sum over C + sum_c |f_c| ddz_c (+ u |ref| for the added term); carried; the buffer holds step 0's
  de        alpha (dalpha - dot), dot = sum alpha dalpha: ddot = sum alpha ddalpha + (P + 4) u sum |alpha dalpha|,
            dde = alpha (ddalpha + ddot) + 3 u alpha (|dalpha| + |dot|)        (terms before the cancellation)
  dhproj    sum_i de_i w_a_j q_ij, q = 1 - th^2: dth = u |fp + hp| + K_TANH u |th|, dq = 2 |th| dth + 2 u (1 + th^2),
            per term dde |w q| + |de w| dq + 3 u |term|, then the sum rule over P (+ r)
  dfproj    the same terms summed over the steps: the per-step bounds + (L + 4) u sum |terms|
  dwa_rows  sum_i de_i th_ij per step (dde |th| + |de| dth + u |term|, the sum rule over P), over the steps as dfproj
  dgates    the cell rule with dh = dhout + dgates_{t+1} W_hh + dhproj_{t+1} W_h (the stored dhproj), n = 1 + 4H + A
  d_w_f     from the compute-dtype cast of dfproj (bit-checked against dfproj_act), K = B P; bf16: + 2^-8 sum |terms|
  exact     bit equality: weight images, slot 0, the x rows, the copies of h, P = 1 (alpha = 1, z = the feature row, zero attention
            gradients), zero-state hproj, rows past their length, dz / dh_extra after the call, d_features, what a call does not own.
Roll-out: alpha is not saved, so z of a running row is held to sum_i dalpha_i |f_i| + the sum rule over P + r, in bf16 plus
2^-8 sum alpha_i |f_i| for the alpha operand of the MFMA; a row that joins at the last step carries the teacher-forced z bit for bit."""
import math
from typing import NamedTuple, Optional, Tuple

import torch

from tests import decoder_cases as D
from tests.decoder_cases import K_LIBM, K_TANH
from tests.disc_cases import TD, U, U8, Report  # noqa: F401  (Report: re-exported for the tests)

ORDER = ("wf", "wh", "wcat", "wcat_t", "bsum", "wout", "slot0", "xrows", "fproj", "hproj", "alpha", "alpha sum", "z", "past length", "gates", "c",
         "h", "h copies", "alphas out", "h_n c_n", "untouched", "dlogits", "dhout", "d_w_out", "d_b_out", "dgates", "dc", "dalpha", "dhproj",
         "dfproj", "dwa_rows", "dz zero", "dh_extra zero", "dfproj_act", "dx", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "d_w_h", "d_w_f", "d_b_f",
         "d_w_a", "d_features", "d_embed", "rollout z", "rollout joined")
NAMES = ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a")
TEMPERATURE = 0.75
SEED = 404
ZERO_X = 106.0              # x = e - max e below -(ZERO_X + 2 de): the device's expf is exactly 0


class Case(NamedTuple):
    name: str
    family: str                   # "train" | "tf" | "rollout"
    B: int
    L: int                        # steps (train), T = caption length + 1 (tf), caption length (rollout)
    V: int
    E: int
    H: int
    C: int
    P: int
    A: int
    dtype: str
    N: int = 0                    # roll-outs per caption and prefix
    states: bool = True           # explicit (h0, c0) (train)
    lengths: Optional[Tuple[int, ...]] = None
    sat: bool = False

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    @property
    def din(self):
        return self.E + self.C

    @property
    def ldx(self):
        return self.E + self.C + self.H

    @property
    def lens(self):
        return torch.tensor(self.lengths if self.family == "tf" else [self.L] * self.B)

    @property
    def steps(self):
        return max(self.lengths) if self.family == "tf" else self.L

    @property
    def rows(self):
        return (self.L - 1) * self.N * self.B

    @property
    def running(self):
        """Roll-out rows that attn_rows serves at the last step (the rest join there)."""
        return (self.L - 2) * self.N * self.B


def _both(name, family, *shape, **kw):
    return [Case(name, family, *shape, dt, **kw) for dt in ("f32", "bf16")]


_BASE = (3, 3, 64, 8, 16, 24, 9, 16)
_TF = (5, 7, 64, 8, 16, 24, 9, 16)
CASES = (
    _both("base", "train", *_BASE)
    + _both("zero-state", "train", *_BASE, states=False)
    + _both("one-pos", "train", 2, 2, 64, 8, 16, 24, 1, 16)
    + _both("wide-A", "train", 2, 2, 64, 8, 16, 24, 5, 520)
    + _both("max-A", "train", 1, 2, 64, 8, 16, 16, 3, 2048)
    + _both("many-P", "train", 2, 2, 64, 8, 16, 24, 300, 16)
    + _both("max-P", "train", 1, 2, 64, 8, 16, 8, 1024, 8)
    + _both("wide-C", "train", 2, 2, 64, 8, 16, 2056, 5, 16)
    + _both("steps", "train", 5, 6, 64, 8, 16, 24, 9, 16)
    + _both("saturated", "train", *_BASE, sat=True)
    + _both("tf-base", "tf", *_TF, lengths=(4, 7, 1, 6, 3))
    + _both("tf-chunks", "tf", 3, 4, 64, 8, 16, 264, 70, 264, lengths=(4, 2, 3))
    + _both("tf-short", "tf", *_TF, lengths=(4, 5, 1, 5, 3))
    + _both("tf-max-P", "tf", 1, 2, 64, 8, 16, 8, 1024, 8, lengths=(2,))
    + _both("tf-max-A", "tf", 1, 2, 64, 8, 16, 16, 3, 2048, lengths=(2,))
    + _both("r-tiles", "rollout", 3, 3, 64, 8, 16, 24, 9, 16, N=40)
    + _both("r-chunks", "rollout", 2, 3, 64, 8, 16, 136, 70, 136, N=5)
    + _both("r-tall", "rollout", 1, 3, 64, 8, 16, 72, 1024, 8, N=20)
)
FAMILY = {f: [c for c in CASES if c.family == f] for f in ("train", "tf", "rollout")}


# ---------------------------------------------------------------------------------------------------------------- geometry
MAX_P, MAX_A = 1024, 2048                                # kAttnMaxP, kAttnMaxA
FWD_POS, Z_POS, BWD_POS = 16, 8, 16                      # positions per pass: 4 waves x kFwdPos, kZ, 4 waves x kBwdPos
ENERGY_POS, CTX_PIECES = 8, 32                           # kEnergyPos, kCtxPieces
ROWS_PC, ROWS_AC = 64, 64                                # kPC, kAC


def cdiv(a, b):
    return -(-a // b)


def _last(n, per):
    """(blocks or passes, live elements of the last)."""
    k = cdiv(n, per)
    return k, n - (k - 1) * per


def rows_lds(tr, P):
    """attn_rows_lds<TR>(P)."""
    ppad = cdiv(P, ROWS_PC) * ROWS_PC
    return (tr * (ppad + 4) + ROWS_PC * (ROWS_AC + 4) + tr * (ROWS_AC + 4) + ROWS_AC) * 4


def geometry(case):
    """Blocks, passes and the live part of the last of every kernel a case launches (csrc/attention.hip, attn_beam.hip, attn_rollout.hip)."""
    c = case
    nv = 4 if c.dtype == "f32" else 8                    # elements of a 16-byte piece
    cols = 64 * nv                                       # columns of an attn_bwd block = of a width pass of a wave
    g = {"nv": nv,
         "bwd_blocks": _last(c.A, cols),                 # attn_bwd: grid.x, live columns of the last block
         "width_passes": _last(c.A, cols),               # attn_fwd / attn_step_energy: passes of a wave over the width, live columns of the last
         "softmax_passes": cdiv(c.P, 256),
         "fwd_pos": _last(c.P, FWD_POS), "z_pos": _last(c.P, Z_POS), "bwd_pos": _last(c.P, BWD_POS),
         "z_chan": _last(c.C, 256 * nv),                 # attn_fwd's z: channel passes, live channels of the last
         "dalpha_blocks": _last(c.B * c.P, 4),           # rows of the last block
         "dalpha_lanes": cdiv(c.C, cols),                # passes of attn_dalpha's lane loop
         "dz_zero": cdiv(c.C, 1024),                     # passes of the dz re-zero loop
         "lstm_chunks": D.lstm_plan(c.dtype, c.din, c.H, False)[0],
         "lds_fwd": (c.A + c.P) * 4, "lds_bwd": (c.P + 8 * cols) * 4,
         "energy_blocks": _last(c.P, ENERGY_POS),        # attn_step_energy: grid.y, live positions of the last
         "ctx_blocks": _last(c.C, CTX_PIECES * nv),      # attn_step_ctx: grid.y, live channels of the last
         "lds_energy": lambda k: k * c.A * 4}
    if c.family == "rollout":
        tr = 32 if rows_lds(32, c.P) <= 64 * 1024 else 16
        per_image = cdiv(c.running, c.B)
        g.update(rows_tile=tr, rows_lds=rows_lds(tr, c.P), rows_tiles=_last(per_image, tr), rows_pos=cdiv(c.P, ROWS_PC),
                 rows_width=_last(c.A, ROWS_AC), rows_chan=_last(c.C, 128 if c.dtype == "bf16" else 64))
    return g


def gumbelmax_from(case):
    """gumbelmax_from_cols for the roll-out's vocabulary product (M = V, K = H): the row count from which a step takes the fused product;
    0 = never."""
    c = case
    if c.dtype != "bf16" or c.V < 128 or c.V % 4 or c.H % 8 or c.ldx % 8:
        return 0
    mt = cdiv(c.V, 128)
    nt = (160 + mt - 1) // mt
    return max(128 * (nt - 1) + 1, 128)


def rollout_layout(case):
    """The roll-out's workspace as csrc/attn_rollout.hip's header states it: ({name: (byte offset, bytes)}, total); every region
    256-byte aligned."""
    c = case
    R, asz = c.rows, 4 if c.dtype == "f32" else 2
    frm = gumbelmax_from(c)
    logit_rows = R if frm == 0 or R < frm else frm - 1
    at, out = 0, {}
    for name, nbytes in (("xh", R * c.ldx * asz), ("c", 2 * R * c.H * 4), ("gpre", R * 4 * c.H * 4), ("hp", R * c.A * 4), ("rowkey", c.L * R * 8),
                         ("logits", logit_rows * c.V * 4)):
        out[name] = (at, nbytes)
        at += (nbytes + 255) & ~255
    return out, at


def rollout_views(case, ws):
    """The xh [rows, ldx] and hp [rows, A] regions of a uint8 workspace."""
    lay, total = rollout_layout(case)
    assert ws.numel() >= total
    o, n = lay["xh"]
    xh = ws[o:o + n].view(TD[case.dtype]).view(case.rows, case.ldx)
    o, n = lay["hp"]
    return xh, ws[o:o + n].view(torch.float32).view(case.rows, case.A)


# ---------------------------------------------------------------------------------------------------------------- data
def data(case):
    """Master weights in NAMES order (float32, CPU) and the inputs of a case: Gaussian, pre-activations, energies and logits of unit
    order; `sat`: w_f and w_a scaled until energies spread by more than 104 and |fp + hp| exceeds 10."""
    c, td = case, TD[case.dtype]
    gen = torch.Generator().manual_seed(SEED)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    s = 1.0 / math.sqrt(c.ldx)
    P = [rn(c.V, c.E), rn(4 * c.H, c.din) * s, rn(4 * c.H, c.H) * s * 2.0, 0.3 * rn(4 * c.H), 0.3 * rn(4 * c.H),
         2.0 * rn(c.V, c.H) / math.sqrt(c.H), 0.5 * rn(c.V),
         rn(c.A, c.C) / math.sqrt(c.C), 0.3 * rn(c.A), 2.0 * rn(c.A, c.H) / math.sqrt(c.H), 3.0 * rn(c.A) / math.sqrt(c.A)]
    if c.sat:
        P[7] = P[7] * 30.0
        P[10] = 15.0 * rn(c.A)
    S = c.steps
    X = {"features": rn(c.B, c.E), "fmap": rn(c.B, c.P, c.C).to(td), "T": TEMPERATURE, "h0": None, "c0": None, "d_alphas": None, "caps": None}
    if c.family == "train":
        X["u"] = torch.rand(c.L, c.B, c.V, generator=gen)
        X["d_out"] = rn(c.B, c.L, c.V)
        if c.states:
            X["h0"], X["c0"] = 0.5 * rn(c.B, c.H), rn(c.B, c.H)
    else:
        if c.family == "rollout":
            X["Y"] = torch.randint(0, c.V, (c.B, c.L), generator=gen)
            X["caps"] = X["Y"][:, :-1].contiguous()
            X["u_roll"] = torch.rand(c.L, c.rows, c.V, generator=gen)
        else:
            X["caps"] = torch.randint(0, c.V, (c.B, c.L - 1), generator=gen)
        X["u"] = torch.rand(c.B, S, c.V, generator=gen)
        live = (torch.arange(S)[None, :] < c.lens[:, None])
        X["d_out"] = rn(c.B, S, c.V) * live[:, :, None]                    # a loss never reads a padded step
        X["d_alphas"] = rn(c.B, S, c.P)
    return P, X


def images(case, P):
    """The weight images gic_attn_prepare keeps."""
    td = TD[case.dtype]
    wcat = torch.cat([P[1], P[2]], 1).to(td)
    return {"wcat": wcat, "wcat_t": wcat.t().contiguous(), "bsum": P[3] + P[4], "wout": P[5].to(td), "wf": P[7].to(td), "wh": P[9].to(td)}


def check_images(case, P, shadow, rep):
    want = images(case, P)
    for k in ("wf", "wh", "wcat", "bsum"):
        rep.bits(k, shadow[k], want[k])
    rep.bits("wcat_t", shadow["wcat_t"], shadow["wcat"].t().contiguous())
    if shadow.get("wout") is not None:
        rep.bits("wout", shadow["wout"], want["wout"])


def new_state(case):
    """The state as AttnDecoderEngine.alloc_state shapes it (CPU, NaN), with the outputs that belong to it: `out` and `ids` hold what a
    device could have written (a fill needs tokens and probabilities to go on from)."""
    c, td, nan = case, TD[case.dtype], float("nan")
    L, S = c.L, c.steps
    gen = torch.Generator().manual_seed(SEED + 1)
    st = {"xh": torch.full((L + 1, c.B, c.ldx), nan, dtype=td), "gates": torch.full((L, c.B, 4 * c.H), nan), "c": torch.full((L + 1, c.B, c.H), nan),
          "hout": torch.full((c.B * L * c.H,), nan, dtype=td), "fproj": torch.full((c.B, c.P, c.A), nan, dtype=td),
          "alpha": torch.full((L, c.B, c.P), nan), "hproj": torch.full((L, c.B, c.A), nan),
          "out": torch.softmax(2.0 * torch.randn(c.B, S, c.V, generator=gen), 2).to(td),
          "ids": torch.randint(0, c.V, (c.B, S), generator=gen)}
    if c.family != "train":
        st.update(alphas=torch.full((c.B, S, c.P), nan), h_n=torch.full((c.B, c.H), nan), c_n=torch.full((c.B, c.H), nan))
    return st


def new_ws(case):
    """AttnDecoderEngine.alloc_bwd_ws (CPU, NaN)."""
    c, td, nan = case, TD[case.dtype], float("nan")
    L = c.L
    return {"dlogits": torch.full((c.B * L * c.V,), nan, dtype=td), "dhout": torch.full((c.B * L * c.H,), nan),
            "dgates": torch.full((L, c.B, 4 * c.H), nan, dtype=td), "dc": torch.full((c.B, c.H), nan), "dz": torch.full((c.B, c.C), nan),
            "dalpha": torch.full((c.B, c.P), nan), "dh_extra": torch.full((c.B, c.H), nan), "dhproj": torch.full((L, c.B, c.A), nan, dtype=td),
            "dfproj": torch.full((c.B, c.P, c.A), nan), "dfproj_act": None if c.dtype == "f32" else torch.full((c.B, c.P, c.A), nan, dtype=td),
            "dwa_rows": torch.full((c.B, c.A), nan), "dx": torch.full((L * c.B, c.E), nan)}


def new_grads(case, P):
    return [torch.full(p.shape, float("nan")) for p in P] + [torch.full((case.B, case.E), float("nan"))]


def new_rollout_ws(case):
    """The roll-out's workspace (CPU, uint8, NaN bit patterns in the regions compared)."""
    ws = torch.zeros(rollout_layout(case)[1], dtype=torch.uint8)
    xh, hp = rollout_views(case, ws)
    xh.fill_(float("nan"))
    hp.fill_(float("nan"))
    return ws


# ---------------------------------------------------------------------------------------------------------------- references
def attention(fp, hp, wa):
    """fp64 alpha [.., P] of fp [.., P, A] and hp [.., A] with its bound, the energies and their bound (module docstring)."""
    Pn, A = fp.shape[-2], fp.shape[-1]
    x = fp + hp.unsqueeze(-2)
    th = torch.tanh(x)
    terms = wa * th
    e = terms.sum(-1)
    de = (wa.abs() * (U * x.abs() + K_TANH * U * th.abs())).sum(-1) + (A + 4) * U * terms.abs().sum(-1)
    xs = e - e.max(-1, keepdim=True).values
    dmax = de.max(-1, keepdim=True).values
    al = torch.softmax(e, -1)
    bound = al * (torch.expm1(2 * dmax) + U * (2 * K_LIBM * (1 + xs.abs()) + Pn + 16))
    zero = xs < -(ZERO_X + 2 * dmax)
    return torch.where(zero, torch.zeros_like(al), al), torch.where(zero, torch.zeros_like(al), bound), e, de


def attention_bwd(al, dal, dal_b, fp, hp, wa):
    """One step of the attention backward from the device's alpha [B, P] and the carried d alpha with its bound: the d fproj terms
    [B, P, A] and d hproj [B, A], d w_a rows [B, A], each with its bound (module docstring)."""
    Pn = al.shape[1]
    dot = (al * dal).sum(1, keepdim=True)
    dot_b = (al * dal_b).sum(1, keepdim=True) + (Pn + 4) * U * (al * dal).abs().sum(1, keepdim=True)
    de = al * (dal - dot)
    de_b = al * (dal_b + dot_b) + 3 * U * al * (dal.abs() + dot.abs())
    x = fp + hp[:, None, :]
    th = torch.tanh(x)
    th_b = U * x.abs() + K_TANH * U * th.abs()
    q = 1 - th * th
    q_b = 2 * th.abs() * th_b + 2 * U * (1 + th * th)
    term = de[:, :, None] * wa * q
    term_b = de_b[:, :, None] * (wa * q).abs() + (de[:, :, None] * wa).abs() * q_b + 3 * U * term.abs()
    wt = de[:, :, None] * th
    wt_b = de_b[:, :, None] * th.abs() + de.abs()[:, :, None] * th_b + U * wt.abs()
    return term, term_b, wt, wt_b


def alpha_scale(case):
    """The `alpha_scaled` mutation's factor - 1: 2^-12 where the alpha bound can see it; the energy's sum rule over A widens the bound
    to ~ 2 (A + 4) u sum |w_a th| (A = 136..520: 2e-4..2e-3; A = 2048: 1e-2; the saturated case's |w_a| of 15: 1e-3), where the smallest
    visible power of two is larger."""
    return 2.0 ** -12 if case.A <= 24 and not case.sat else (2.0 ** -8 if case.A <= 520 else 2.0 ** -5)


class _Walk:
    """emit / same of a walk: compare with a Report, fill without one; `rows`: only these rows of the leading dimension."""

    def __init__(self, case, rep):
        self.rep, self.td = rep, TD[case.dtype]

    def emit(self, stage, view, ref, bound, rows=None):
        if torch.is_tensor(bound):
            bound = bound.expand_as(ref)
        if rows is not None:
            if self.rep is None:
                view[rows] = ref[rows].to(view.dtype)
            else:
                self.rep.check(stage, view[rows], ref[rows], bound[rows] if torch.is_tensor(bound) else bound)
        elif self.rep is None:
            view.copy_(ref.to(view.dtype))
        else:
            self.rep.check(stage, view, ref, bound)

    def same(self, stage, view, want, rows=None):
        want = want.to(view.dtype).expand_as(view)
        if rows is not None:
            if self.rep is None:
                view[rows] = want[rows]
            else:
                self.rep.bits(stage, view[rows], want[rows])
        elif self.rep is None:
            view.copy_(want)
        else:
            self.rep.bits(stage, view, want)


def hout_view(case, st):
    c = case
    return st["hout"][:c.B * c.steps * c.H].view(c.B, c.steps, c.H)


def run_forward(case, P, img, X, st, rep=None, mut=None):
    """Walk the forward stages of sample_fwd (train) or of the packed teacher-forced pass (tf, rollout) over `st` (new_state's keys).
    rep: check; None: fill, `mut` a mutation of the fill."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, L, V, E, H, C, Pn, A = c.B, c.L, c.V, c.E, c.H, c.C, c.P, c.A
    din, S, packed = c.din, c.steps, c.family != "train"
    w = _Walk(c, rep)
    emit, same = w.emit, w.same
    mut = mut if rep is None else None
    r = lambda ref: U8 * ref.abs() if bf else 0.0
    lens = c.lens
    xh, hout = st["xh"], hout_view(c, st)
    # slot 0 and the x rows (the teacher's tokens are known up front, the roll-out's are the device's own ids)
    same("slot0", xh[0][:, :E], X["features"])
    same("slot0", xh[0][:, din:], X["h0"] if X["h0"] is not None else torch.zeros(B, H))
    same("slot0", st["c"][0], X["c0"] if X["c0"] is not None else torch.zeros(B, H))
    tok = X["caps"] if packed else st["ids"]
    for t in range(1, L if packed else S):
        same("xrows", xh[t][:, :E], P[0][tok[:, t - 1].clamp(0, V - 1)])
    fm = X["fmap"].double()
    wf, wh, wa = img["wf"].double(), img["wh"].double(), P[10].double()
    fp_ref = fm @ wf.t() + P[8].double()
    emit("fproj", st["fproj"], fp_ref, D.sum_bound(C, fm.abs() @ wf.abs().t() + P[8].double().abs(), None) + r(fp_ref))
    fp = st["fproj"].double()
    one = torch.ones(B, dtype=torch.bool)
    for t in range(S):
        lv = (lens > t) if packed else one
        rows = None if bool(lv.all()) else lv
        h_prev = xh[t][:, din:].double()
        if mut == "hproj_from_h_t":                        # (a fill walks the steps twice: h_t exists on the second walk)
            h_prev = xh[t + 1][:, din:].double()
        emit("hproj", st["hproj"][t], h_prev @ wh.t(), D.sum_bound(H, xh[t][:, din:].double().abs() @ wh.abs().t(), None))
        if t == 0 and X["h0"] is None:
            same("hproj", st["hproj"][0], torch.zeros(B, A))
        hp = st["hproj"][t].double()
        al_ref, al_b, e, _ = attention(fp, hp, wa)
        if mut == "alpha_first256":
            m = e[:, :256].max(1, keepdim=True).values
            al_ref = torch.exp(e - m) / torch.exp(e[:, :256] - m).sum(1, keepdim=True)
        if mut == "alpha_scaled":
            al_ref = al_ref * (1 + alpha_scale(c))
        emit("alpha", st["alpha"][t], al_ref, al_b, rows)
        al = st["alpha"][t].double()
        if rep is not None:
            rep.check("alpha sum", al.sum(1)[lv], torch.ones(int(lv.sum()), dtype=torch.float64), (Pn * U + al_b.sum(1))[lv])
        alz = al
        if mut == "z_neighbour_alpha":
            alz = al.roll(-1, 0)
        if mut == "z_tail_dropped":
            alz = al.clone()
            alz[:, Pn - Pn % Z_POS:] = 0
        z_ref = torch.einsum("bp,bpc->bc", alz, fm)
        zv = xh[t][:, E:din]
        if mut == "z_last8_stale":
            z_ref[:, C - 8:] = 0.5
        emit("z", zv, z_ref, D.sum_bound(Pn, torch.einsum("bp,bpc->bc", al.abs(), fm.abs()), None) + r(z_ref), rows)
        if Pn == 1 and mut is None:
            same("alpha", st["alpha"][t], torch.ones(B, 1), rows)
            same("z", zv, X["fmap"][:, 0], rows)
        if rows is not None:                               # past its length: a zero alpha row, zero z, zero gates and output row, (h, c) kept
            dead = ~lv
            same("past length", st["alpha"][t], torch.zeros(B, Pn), dead)
            same("past length", zv, torch.zeros(B, C), dead)
            same("past length", st["gates"][t], torch.zeros(B, 4 * H), dead)
            same("past length", st["c"][t + 1], st["c"][t], dead)
            same("past length", xh[t + 1][:, din:], xh[t][:, din:], dead)
            same("past length", hout[:, t], torch.zeros(B, H), dead)
            if mut == "past_alpha":
                st["alpha"][t][dead] = 1.0 / Pn
            if mut == "past_z":
                zv[dead] = 2.0 ** -20
        # the cell over the full [x | z | h] row (the gw = E < din seam of lstm_step's gather is inside it)
        D.cell_forward(lambda s_, v, ref, bnd: emit(s_, v, ref, bnd, rows), bf, xh[t].double(), img["wcat"].double(), img["bsum"].double(),
                       st["gates"][t], st["c"][t], st["c"][t + 1], xh[t + 1][:, din:])
        same("h copies", hout[:, t], xh[t + 1][:, din:], rows)
    if packed:
        same("alphas out", st["alphas"], st["alpha"][:S].transpose(0, 1))
        same("h_n c_n", st["h_n"], xh[S][:, din:].float())
        same("h_n c_n", st["c_n"], st["c"][S])
    if rep is not None and S < L:                          # what a pass over Tmax < T steps does not own keeps its pre-fill
        keep = [st["alpha"][S:], st["hproj"][S:], st["gates"][S:], st["c"][S + 1:], xh[S + 1:, :, E:], xh[L:, :, :E], st["hout"][B * S * H:]]
        rep.exact("untouched", torch.cat([torch.isnan(k.float()).reshape(-1) for k in keep]), "of the slots past Tmax changed")


def fill_forward(case, P, img, X, st, mut=None):
    run_forward(case, P, img, X, st, None, None if mut == "hproj_from_h_t" else mut)
    if mut == "hproj_from_h_t":
        run_forward(case, P, img, X, st, None, mut)


def run_backward(case, P, img, X, st, ws, grads, rep=None, mut=None):
    """Walk the backward stages (sample_bwd; forward_tf_bwd with d_alphas) over `ws` (new_ws's keys) and `grads` (new_grads' list)."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, L, V, E, H, C, Pn, A = c.B, c.L, c.V, c.E, c.H, c.C, c.P, c.A
    din, S, packed = c.din, c.steps, c.family != "train"
    BS = B * S
    w = _Walk(c, rep)
    emit, same = w.emit, w.same
    mut = mut if rep is None else None
    r = lambda ref: U8 * ref.abs() if bf else 0.0
    # the output layer: decoder_output_bwd, by the rules of decoder_cases (a loss on a padded step is zero, so zero_past_length is exact)
    dcase = D.Case(c.name, B, S, V, E, H, 1, c.dtype, "")
    dhout = ws["dhout"][:BS * H].view(B, S, H)
    D.run_backward(dcase, P[:7], {"wout": img["wout"]}, {"d_out": X["d_out"], "T": X["T"]}, {"out": st["out"], "hout": hout_view(c, st)},
                   {"dlogits": ws["dlogits"][:BS * V].view(B, S, V), "dhout": dhout}, grads, rep, only={"dlogits", "dhout", "d_w_out", "d_b_out"})
    Wt = img["wcat_t"].double()
    Wx, Wz, Whh = Wt[:E], Wt[E:din], Wt[din:]
    wh, wa = img["wh"].double(), P[10].double()
    fm, fp = X["fmap"].double(), st["fproj"].double()
    d_al = X["d_alphas"] if mut != "dalpha_no_add" else None
    carry = (torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64))
    z3 = lambda: torch.zeros(B, Pn, A, dtype=torch.float64)
    z2 = lambda: torch.zeros(B, A, dtype=torch.float64)
    dfp, dfp_b, dfp_m, dwa, dwa_b, dwa_m = z3(), z3(), z3(), z2(), z2(), z2()
    dal = dal_b = None
    cols = 64 * (8 if bf else 4)
    for t in range(S - 1, -1, -1):
        dh = dhout[:, t].double()
        mag, n = dh.abs(), 1
        if t + 1 < S:
            nx = ws["dgates"][t + 1].double()
            dh, mag, n = dh + nx @ Whh.t(), mag + nx.abs() @ Whh.abs().t(), n + 4 * H + A
            hx = ws["dhproj"][t + 1].double()
            mag = mag + hx.abs() @ wh.abs()
            if mut != "dgates_no_extra":
                dh = dh + hx @ wh
        carry = D.cell_backward(emit, bf, dh, (n + 4) * U * mag, st["gates"][t], st["c"][t], st["c"][t + 1], carry, ws["dgates"][t])
        dg = ws["dgates"][t].double()
        dz, dz_b = dg @ Wz.t(), D.sum_bound(4 * H, dg.abs() @ Wz.abs().t(), None)
        dal = torch.einsum("bc,bpc->bp", dz, fm)
        dal_b = D.sum_bound(C, torch.einsum("bc,bpc->bp", dz.abs(), fm.abs()), None) + torch.einsum("bc,bpc->bp", dz_b, fm.abs())
        if d_al is not None:
            dal = dal + d_al[:, t].double()
            dal_b = dal_b + U * dal.abs()
        term, term_b, wt, wt_b = attention_bwd(st["alpha"][t].double(), dal, dal_b, fp, st["hproj"][t].double(), wa)
        tsum = term
        if mut == "dhproj_pos_dropped":
            tsum = term.clone()
            tsum[:, 3::4] = 0
        dhp = tsum.sum(1)
        if mut == "dhproj_last_block_zero":
            dhp[:, (cdiv(A, cols) - 1) * cols:] = 0
        emit("dhproj", ws["dhproj"][t], dhp, term_b.sum(1) + (Pn + 4) * U * term.abs().sum(1) + r(dhp))
        if not (mut == "dfproj_step_missing" and t == 0):
            dfp = dfp + term
        dfp_b, dfp_m = dfp_b + term_b, dfp_m + term.abs()
        dwa = wt.sum(1) if mut == "dwa_overwritten" else dwa + wt.sum(1)
        dwa_b, dwa_m = dwa_b + wt_b.sum(1) + (Pn + 4) * U * wt.abs().sum(1), dwa_m + wt.abs().sum(1)
    emit("dalpha", ws["dalpha"], dal, dal_b)               # the buffer holds step 0's
    if mut == "dfproj_last_pass":
        dfp[:, (cdiv(Pn, BWD_POS) - 1) * BWD_POS:] = 0
    emit("dfproj", ws["dfproj"], dfp, dfp_b + (S + 4) * U * dfp_m)
    emit("dwa_rows", ws["dwa_rows"], dwa, dwa_b + (S + 4) * U * dwa_m)
    emit("dc", ws["dc"], carry[0], carry[1])
    if Pn == 1:                                            # de = alpha (dalpha - alpha dalpha) with alpha = 1: exactly zero
        same("dhproj", ws["dhproj"][:S], torch.zeros(S, B, A))
        same("dfproj", ws["dfproj"], torch.zeros(B, Pn, A))
        same("dwa_rows", ws["dwa_rows"], torch.zeros(B, A))
    same("dz zero", ws["dz"], torch.zeros(B, C))
    same("dh_extra zero", ws["dh_extra"], torch.zeros(B, H))
    # batched over all steps
    dG, xs = ws["dgates"][:S].double().reshape(BS, 4 * H), st["xh"][:S].double().reshape(BS, c.ldx)
    emit("dx", ws["dx"][:BS], dG @ Wx.t(), D.sum_bound(4 * H, dG.abs() @ Wx.abs().t(), None))
    emit("d_w_ih", grads[1], dG.t() @ xs[:, :din], D.sum_bound(BS, dG.abs().t() @ xs[:, :din].abs(), None))
    emit("d_w_hh", grads[2], dG.t() @ xs[:, din:], D.sum_bound(BS, dG.abs().t() @ xs[:, din:].abs(), None))
    emit("d_b_ih", grads[3], dG.sum(0), D.sum_bound(BS, dG.abs().sum(0), None))
    emit("d_b_hh", grads[4], dG.sum(0), D.sum_bound(BS, dG.abs().sum(0), None))
    dH = ws["dhproj"][:S].double().reshape(BS, A)
    emit("d_w_h", grads[9], dH.t() @ xs[:, din:], D.sum_bound(BS, dH.abs().t() @ xs[:, din:].abs(), None))
    dF = ws["dfproj"].to(td)
    if bf:
        same("dfproj_act", ws["dfproj_act"], dF)
    dF, fm2 = dF.double().reshape(B * Pn, A), fm.reshape(B * Pn, C)
    wmag = dF.abs().t() @ fm2.abs()
    emit("d_w_f", grads[7], dF.t() @ fm2, D.sum_bound(B * Pn, wmag, None) + (U8 * wmag if bf else 0.0))
    dF32 = ws["dfproj"].double().reshape(B * Pn, A)
    emit("d_b_f", grads[8], dF32.sum(0), D.sum_bound(B * Pn, dF32.abs().sum(0), None))
    dW = ws["dwa_rows"].double()
    emit("d_w_a", grads[10], dW.sum(0), D.sum_bound(B, dW.abs().sum(0), None))
    same("d_features", grads[11], ws["dx"][:B])
    ge, gm = torch.zeros(V, E, dtype=torch.float64), torch.zeros(V, E, dtype=torch.float64)
    if S > 1:
        tok = (X["caps"] if packed else st["ids"])[:, :S - 1].t().reshape(-1).clamp(0, V - 1)        # (t - 1, b) order
        src = ws["dx"][B:BS].double()
        ge.index_add_(0, tok, src)
        gm.index_add_(0, tok, src.abs())
    emit("d_embed", grads[0], ge, D.sum_bound(B * (S - 1), gm, None))
    if rep is not None and S < L:
        keep = [ws["dgates"][S:], ws["dhproj"][S:], ws["dx"][BS:], ws["dlogits"][BS * V:], ws["dhout"][BS * H:]]
        rep.exact("untouched", torch.cat([torch.isnan(k.float()).reshape(-1) for k in keep]), "of the workspace past Tmax changed")


def run_rollout(case, P, img, X, st, ws, rep=None, mut=None):
    """The roll-out's workspace after gic_attn_rollout: rows [0, running) were served by attn_rows at the last step (their hp and z are
    still there), rows [running, rows) joined at the last step with the teacher-forced pass's z.  Fill: hp is arbitrary (the rows' h is
    the roll-out's own business), z follows from it."""
    c, bf = case, case.dtype == "bf16"
    B, E, din, Pn, M = c.B, c.E, c.din, c.P, c.running
    w = _Walk(c, rep)
    xh, hp = rollout_views(c, ws)
    if rep is None:
        hp[:M] = 0.6 * torch.randn(M, c.A, generator=torch.Generator().manual_seed(SEED + 2))
    img_of = torch.arange(M) % B
    fm, fp = X["fmap"].double(), st["fproj"].double()
    al, al_b, _, _ = attention(fp[img_of], hp[:M].double(), P[10].double())
    f = fm[img_of]                                                                        # [M, P, C]
    z = torch.einsum("mp,mpc->mc", al, f)
    mag = torch.einsum("mp,mpc->mc", al, f.abs())
    bound = torch.einsum("mp,mpc->mc", al_b, f.abs()) + D.sum_bound(Pn, mag, None) + (U8 * z.abs() + U8 * mag if bf else 0.0)
    mut = mut if rep is None else None
    if mut == "roll_chan_first_group":
        z[:, 128:] = z[:, :c.C - 128]
    w.emit("rollout z", xh[:M, E:din], z, bound)
    if mut == "roll_tail_stale":
        tr = geometry(c)["rows_tile"]
        k = (cdiv(M, B) - 1) // tr * tr                    # first row of an image's last tile
        xh[k * B + (B - 1), E:din] = 0.25
    w.same("rollout joined", xh[M:, E:din], st["xh"][c.L - 1][torch.arange(M, c.rows) % B][:, E:din])
    if mut == "roll_joined_bits":
        v = xh[M:, E:din]
        v[0, 0] = v[0, 0] * 1.5 + 0.5
