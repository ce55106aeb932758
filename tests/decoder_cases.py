"""The LSTM caption decoder (csrc/decoder_step.hip, csrc/decoder.hip) step by step: the case table, a restatement of the route
selection, the fp64 reference of every stage, the per-element bounds and the checker behind tests/test_decoder_cases.py (no GPU) and
tests/test_gpu_decoder_stages.py (every case on the GPU).  Nothing here touches the GPU.

Every stage is checked against an fp64 reference formed from the buffers the kernels themselves wrote upstream of it (`xh`, `gates`,
`c`, `hout`, `part`, `out`, `ids`, `dlogits`, `dhout`, `dgates`, `dxh`), so errors do not compound, a token flipped at one step
excuses nothing at the next, and bf16 is as tightly checkable as f32.  `run_forward` / `run_backward` walk the stages in order; with a
Report they compare the buffers given, without one they FILL them from the references (a correct result in storage precision: what
the checker's self-test mutates).

Bounds, per element, with the conventions of tests/disc_cases.py: u = 2^-24, r = 2^-8 |ref| where the output is bf16, an underflow
floor of 2^-110 on every non-zero bound.  All derived, none fitted:
  sum      n products in any order (MFMA, K halves, split-K, atomics):  (n + 4) u (sum |terms| + |bias|) + r
  gates    sigmoid / tanh of the pre-activation: Lipschitz (1/4, 1) times the product's bound + K_SIG (K_TANH) u |ref|
  c        f c' + i g: two products and a sum, 3 u (|f c'| + |i g|)
  h        o tanh(c): (K_TANH + 2) u |ref| + r
  libm     logf and expf at 1 ulp, as tests/disc_cases.py takes expf: an ulp is up to 2^-23 |ref|, so K_LIBM = 2 in units of u |ref|
  gumbel   g = -log(-log(u + eps) + eps).  a = u + eps rounds once (u |a|, so u on l1 = log a), the logarithm errs by
           K u max(|l1|, 1), a2 = eps - l1 rounds once, the second logarithm errs by K u max(|g|, 1):
             |dg| <= (u + K u max(|l1|, 1) + u a2) / a2 + K u max(|g|, 1),        K = K_LIBM (logf) or K_LOG_FAST (__logf, bf16 mode)
  y        (o + b + g) T: (the product's bound + |dg| + u (|o + b| + |o + b + g|)) |T| + u |y|;   pretrain: the product's bound
  part_m   the tile maximum: the largest bound of the tile (max rule, no entry excluded)
  part_s   sum over the tile of exp(y - m) with the DEVICE's m: per term e (expm1(|dy| + u |x|) + K u (1 + |x|)), x = y - m,
           K = K_LIBM (expf) or K_EXP_FAST (__expf), plus (64 + 4) u (sum e)
  out      softmax: |dp| <= p (expm1(2 max |dy|) + u (2 K (1 + |x|) + V + tiles + 16)) + r; the fused route rounds a bf16 `out` twice
           (the tile's e, then the scaled p): 2 r; pretrain: y's bound + r.  (Derivation revisited: half a bf16 ulp is 2^-9 |ref| only
           at the top of a binade and 2^-8 |ref| at its bottom, so two roundings are 2 * 2^-8 |ref|, not 2 * 2^-9 |ref|.)
  ids      the device's id has an fp64 y within twice the row's largest bound of the row maximum (so it IS the argmax wherever the
           margin between the two largest y exceeds that); forced positions hold the forced id clamped to [0, V)
  dlogits  T p (dp - s), s = sum p dp: |T p| (V + 4) u sum |p dp| + 3 u |T p| (|dp| + |s|) + r
  dgates   dh by the sum rule over both segments; the cell-gradient carry dc is not saved per step: the reference carries its fp64
           value and its bound E along the chain, E_t = |f_{t+1}| E_{t+1} + the local terms (below, in run_backward)
  exact    bit equality: weight images, slot 0, the x rows, the copies of h, forced ids, d_features, what a route must not touch.

K_TANH, K_SIG (tanhf and the expf-built sigmoid of the cell) and K_LOG_FAST, K_EXP_FAST (__logf / __expf of the bf16 kernels) can be
neither derived nor read from the project: they are 4 x the largest error measured on the device in an exact regime in which nothing
else contributes (tests/test_gpu_decoder_stages.py: the calibration cases; its docstring records the measurements)."""
import math
from typing import NamedTuple

import torch

from tests.disc_cases import BITS, SENTINEL, TD, U, U8, Report, sum_bound

KTILE, ROWS, MAX_ROWS = 64, 64, 512     # vocabulary tile, batch rows per block, the fused kernels' row limit
PASS_PIECES = 8 * 512                   # 16-byte pieces one staging pass of lstm_step moves
EPS32 = float(torch.tensor(1e-10, dtype=torch.float32))
# 4 x the largest error measured on an MI355X (units: u |ref| for tanh / sigmoid; the structures above for the fast intrinsics)
K_LIBM = 2.0
K_TANH, K_SIG = 4 * 1.212, 4 * 1.878
K_LOG_FAST, K_EXP_FAST = 4 * 1.352, 4 * 0.622
TEMPERATURE = 0.75
DXH_FILL = SENTINEL                     # what the input-gradient buffers hold before the backward: a route leaves what it does not write

ORDER = ("wcat", "wcat_t", "wout", "bsum", "slot0", "xrows", "gates", "c", "h", "h copies", "part_m", "part_s", "key", "ids", "out",
         "dlogits", "dhout", "d_w_out", "d_b_out", "dgates", "dc", "dxh", "dxh keep", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh",
         "d_b_ih == d_b_hh", "d_features", "d_embed")


class Case(NamedTuple):
    name: str
    B: int
    L: int
    V: int
    E: int
    H: int
    NL: int
    dtype: str                    # "f32" | "bf16"
    route: str                    # route_str(select(case)), pinned in tests/test_decoder_cases.py
    part: bool = True             # False: st["part"] = None, the generic forward
    pretrain: bool = False
    states: bool = False          # explicit (h0, c0)
    force: bool = False           # force_ids with force_len 0..L and out-of-range ids
    det: bool = False             # d_embed once more in deterministic mode

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    def din(self, l):
        return self.E if l == 0 else self.H

    def ldx(self, l):
        return self.din(l) + self.H

    @property
    def nblk(self):
        return -(-self.V // KTILE)


def lstm_plan(dtype, din, H, gather):
    """lstm_step's K chunks, staging passes and whether the x|h seam of a gathering step falls inside a chunk."""
    sz = 4 if dtype == "f32" else 2
    ve, ldx = 16 // sz, din + H
    kc_max = min((ldx + 31) // 32 * 32, 2048 // sz)                     # lstm_chunk()
    passes, seam = 1, False
    for kc0 in range(0, ldx, kc_max):
        kc = min(kc_max, ldx - kc0)
        xc = max(0, min(kc, din - kc0)) if gather else 0
        passes = max(passes, -(-max(ROWS * (xc // ve), ROWS * ((kc - xc) // ve)) // PASS_PIECES))
        seam = seam or 0 < xc < kc
    return -(-ldx // kc_max), passes, seam


def select(case):
    """The routes and kernels gic_decoder_sample_fwd / _bwd take for a case, restated."""
    c, bf = case, case.dtype == "bf16"
    sz = 2 if bf else 4
    step_ok = c.V >= 4 and c.V % 4 == 0 and c.E % 8 == 0 and c.H % 8 == 0 and c.nblk <= 1024       # decoder_fused_rows
    fwd = "fused" if c.part and c.B <= MAX_ROWS and step_ok else "generic"
    bwd = "fused" if c.H % 8 == 0 and c.B <= MAX_ROWS else "generic"
    argmax = None
    if fwd == "generic":
        argmax = "reg1" if c.V % 4 == 0 and c.V <= 4096 else ("reg4" if c.V % 4 == 0 and c.V <= 16384 else "scalar")
    if c.pretrain:
        soft = None
    elif not bf:
        soft = "vec8" if c.V % 4 == 0 and c.V <= 8192 else "scalar"
    else:
        soft = "vec5" if c.V % 8 == 0 and c.V <= 10240 else ("vec8" if c.V % 8 == 0 and c.V <= 16384 else "scalar")
    lstm = vocab = None
    if fwd == "fused":
        lstm = []
        for l in range(c.NL):
            first = lstm_plan(c.dtype, c.din(l), c.H, False)                     # step 0 (and every step above layer 0) gathers nothing
            later = lstm_plan(c.dtype, c.din(l), c.H, True) if l == 0 and c.L > 1 else (first[0], None, False)
            lstm.append((first[0], first[1], later[1], later[2]))
        kc = min((c.H + 31) // 32 * 32, 1024 // sz)                     # vocab_chunk()
        vocab = -(-c.H // kc)
    return {"fwd": fwd, "bwd": bwd, "argmax": argmax, "softmax_bwd": soft, "lstm": lstm, "vocab": vocab}


def route_str(s):
    # per layer: chunks x passes of a step that gathers nothing [/ passes of a gathering step, s: the x|h seam inside a chunk]
    lstm = "-" if s["lstm"] is None else ",".join(f"{c}x{p}" + (f"/{g}{'s' if seam else ''}" if g else "") for c, p, g, seam in s["lstm"])
    return f"{s['fwd']}/{s['bwd']} argmax={s['argmax'] or '-'} softmax_bwd={s['softmax_bwd'] or '-'} lstm={lstm} vocab={s['vocab'] or '-'}"


def _both(name, B, L, V, E, H, NL, r32, r16, **kw):
    return [Case(name, B, L, V, E, H, NL, "f32", r32, **kw), Case(name, B, L, V, E, H, NL, "bf16", r16, **kw)]


_FF = "fused/fused argmax=- softmax_bwd="
_GF = "generic/fused argmax="
CASES = (
    # smallest everything: one quad, one unit block; three layers (h_up twice)
    _both("tiny1", 1, 2, 4, 8, 8, 1, _FF + "vec8 lstm=1x1/1s vocab=1", _FF + "scalar lstm=1x1/1s vocab=1")
    + _both("tiny3", 3, 3, 4, 8, 8, 3, _FF + "vec8 lstm=1x1/1s,1x1,1x1 vocab=1", _FF + "scalar lstm=1x1/1s,1x1,1x1 vocab=1", det=True)
    # ldx = 24: a K tail inside one k-step; B = 65: one row in the second 64-row tile; V = 68: one quad in the second vocabulary tile
    + _both("tails", 65, 3, 68, 8, 16, 2, _FF + "vec8 lstm=1x1/1s,1x1 vocab=1", _FF + "scalar lstm=1x1/1s,1x1 vocab=1", det=True)
    + _both("tails-b64", 64, 3, 68, 8, 16, 2, _FF + "vec8 lstm=1x1/1s,1x1 vocab=1", _FF + "scalar lstm=1x1/1s,1x1 vocab=1")
    + _both("tails-generic", 65, 3, 68, 8, 16, 2, _GF + "reg1 softmax_bwd=vec8 lstm=- vocab=-", _GF + "reg1 softmax_bwd=scalar lstm=- vocab=-", part=False)
    # H = 512: 128 unit blocks (the row rotation wraps); f32: ldx = 520 is a second chunk of 8 columns
    + _both("h512", 5, 2, 8, 8, 512, 1, _FF + "vec8 lstm=2x2/2s vocab=2", _FF + "vec5 lstm=1x2/1s vocab=1")
    # E = 520: f32: the x|h seam in the second chunk; bf16: the gathered x part alone needs a second pass
    + _both("e520", 5, 2, 8, 520, 8, 1, _FF + "vec8 lstm=2x2/2s vocab=1", _FF + "vec5 lstm=1x2/2s vocab=1")
    # ldx = 1032: bf16: the seam in the first chunk and a second chunk of 8 columns
    + _both("h1024", 3, 2, 8, 8, 1024, 1, _FF + "vec8 lstm=3x2/2s vocab=4", _FF + "vec5 lstm=2x2/2s vocab=2")
    + _both("e520-h512", 3, 2, 8, 520, 512, 1, _FF + "vec8 lstm=3x2/2s vocab=2", _FF + "vec5 lstm=2x2/2s vocab=1")
    # the bench shape with two layers: layer 1's ldx = 1024 is two passes without a second chunk in bf16
    + _both("e512-h512-nl2", 4, 2, 8, 512, 512, 2, _FF + "vec8 lstm=2x2/2,2x2 vocab=2", _FF + "vec5 lstm=1x2/1s,1x2 vocab=1")
    # vocab_step's second chunk of 8 columns: H = 264 in f32, H = 520 in bf16
    + _both("h264", 3, 2, 68, 8, 264, 1, _FF + "vec8 lstm=1x2/2s vocab=2", _FF + "scalar lstm=1x1/1s vocab=1")
    + _both("h520", 3, 2, 8, 8, 520, 1, _FF + "vec8 lstm=2x2/2s vocab=3", _FF + "vec5 lstm=1x2/2s vocab=2")
    # 258 vocabulary tiles: sample_finish's strided loops; the scalar softmax backward in both dtypes, the scalar argmax on the generic route
    + _both("v16452", 2, 2, 16452, 8, 8, 1, _FF + "scalar lstm=1x1/1s vocab=1", _FF + "scalar lstm=1x1/1s vocab=1")
    + _both("v16452-generic", 2, 2, 16452, 8, 8, 1, _GF + "scalar softmax_bwd=scalar lstm=- vocab=-", _GF + "scalar softmax_bwd=scalar lstm=- vocab=-", part=False)
    + _both("v10248", 2, 2, 10248, 8, 8, 1, _FF + "scalar lstm=1x1/1s vocab=1", _FF + "vec8 lstm=1x1/1s vocab=1")
    + _both("v10248-generic", 2, 2, 10248, 8, 8, 1, _GF + "reg4 softmax_bwd=scalar lstm=- vocab=-", _GF + "reg4 softmax_bwd=vec8 lstm=- vocab=-", part=False)
    + _both("v12", 3, 2, 12, 8, 8, 1, _FF + "vec8 lstm=1x1/1s vocab=1", _FF + "scalar lstm=1x1/1s vocab=1")
    + _both("v12-generic", 3, 2, 12, 8, 8, 1, _GF + "reg1 softmax_bwd=vec8 lstm=- vocab=-", _GF + "reg1 softmax_bwd=scalar lstm=- vocab=-", part=False)
    + _both("v8196", 2, 2, 8196, 8, 8, 1, _FF + "scalar lstm=1x1/1s vocab=1", _FF + "scalar lstm=1x1/1s vocab=1")
    # initial states; forced prefixes of every length with ids of -1 and V among them, on both routes
    + _both("states", 5, 3, 20, 8, 16, 2, _FF + "vec8 lstm=1x1/1s,1x1 vocab=1", _FF + "scalar lstm=1x1/1s,1x1 vocab=1", states=True)
    + _both("forced", 6, 4, 20, 8, 16, 1, _FF + "vec8 lstm=1x1/1s vocab=1", _FF + "scalar lstm=1x1/1s vocab=1", force=True)
    + _both("forced-generic", 6, 4, 20, 8, 16, 1, _GF + "reg1 softmax_bwd=vec8 lstm=- vocab=-", _GF + "reg1 softmax_bwd=scalar lstm=- vocab=-", part=False, force=True)
    # more rows than the fused kernels take: the generic forward and the generic backward (every dxh slot)
    + _both("b516", 516, 2, 8, 8, 8, 1, "generic/generic argmax=reg1 softmax_bwd=vec8 lstm=- vocab=-", "generic/generic argmax=reg1 softmax_bwd=vec5 lstm=- vocab=-", det=True)
    # pretrain mode (raw logits, no softmax backward) on both routes
    + _both("pretrain", 5, 3, 68, 8, 16, 1, _FF + "- lstm=1x1/1s vocab=1", _FF + "- lstm=1x1/1s vocab=1", pretrain=True)
    + _both("pretrain-generic", 5, 3, 68, 8, 16, 1, _GF + "reg1 softmax_bwd=- lstm=- vocab=-", _GF + "reg1 softmax_bwd=- lstm=- vocab=-", part=False, pretrain=True)
)

# the exact regimes (not in CASES: they have parameters of their own)
CAL_CELL = {dt: Case("cal-cell", 64, 1, 4, 8, 128, 1, dt, "", states=True) for dt in ("f32", "bf16")}
CAL_GUMBEL = {dt: Case("cal-gumbel", 64, 2, 4096, 8, 8, 1, dt, "") for dt in ("f32", "bf16")}
TIE_PAIRS = ((3, 4), (5, 9), (15, 16), (63, 64), (127, 128), (130, 137))     # one quad, two lane groups, sub-tiles, tiles, into / inside the partial tile
TIES = {(dt, part): Case("ties" + ("" if part else "-generic"), 3, 2, 140, 8, 8, 1, dt, "", part=part, pretrain=True)
        for dt in ("f32", "bf16") for part in (True, False)}


# ---------------------------------------------------------------------------------------------------------------- data
def make_params(case, gen):
    """Master weights in the engine's order [embed, (w_ih, w_hh, b_ih, b_hh) * NL, w_out, b_out], float32 on the CPU: Gaussian, the gate
    pre-activations and the logits of unit order."""
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    P = [rn(case.V, case.E)]
    for l in range(case.NL):
        s = 1.0 / math.sqrt(case.ldx(l))
        P += [rn(4 * case.H, case.din(l)) * s, rn(4 * case.H, case.H) * s * 2.0, 0.3 * rn(4 * case.H), 0.3 * rn(4 * case.H)]
    return P + [2.0 * rn(case.V, case.H) / math.sqrt(case.H), 0.5 * rn(case.V)]


def make_inputs(case, gen):
    B, L, V = case.B, case.L, case.V
    X = {"features": torch.randn(B, case.E, generator=gen), "u": torch.rand(L, B, V, generator=gen), "T": TEMPERATURE,
         "d_out": torch.randn(B, L, V, generator=gen), "h0": None, "c0": None, "force_ids": None, "force_len": None}
    if case.states:
        X["h0"], X["c0"] = 0.5 * torch.randn(case.NL, B, case.H, generator=gen), torch.randn(case.NL, B, case.H, generator=gen)
    if case.force:
        f = torch.randint(0, V, (B, L), generator=gen)
        f[0, 0], f[1 % B, 0], f[2 % B, 1 % L] = -1, V, V + 5                      # out of range: clamped to 0 and V - 1
        X["force_ids"], X["force_len"] = f, (torch.arange(B) % (L + 1)).to(torch.int32)
        assert case.L >= 2 and int(X["force_len"][1 % B]) >= 1 and int(X["force_len"][2 % B]) >= 2 and B > L
        f[L % B, 0] = -1                                                          # (the row with force_len = L: forced at every step)
    return X


def exact_cell(case, gen):
    """The cell in an exact regime: one +-2^k per weight row, everything else a multiple of 1/8: the pre-activation of step 0 is exact in
    f32 and its operands in bf16, so the saved gates carry the error of tanhf / the sigmoid alone."""
    H, E, B = case.H, case.E, case.B
    eighth = lambda lo, hi, *shape: torch.randint(8 * lo, 8 * hi + 1, shape, generator=gen).float() / 8
    W = torch.zeros(4 * H, E + H)
    col = torch.randint(0, E + H, (4 * H,), generator=gen)
    W[torch.arange(4 * H), col] = (2.0 ** torch.randint(-2, 2, (4 * H,), generator=gen).float()) * (torch.randint(0, 2, (4 * H,), generator=gen) * 2 - 1).float()
    P = [eighth(-2, 2, case.V, E), W[:, :E].contiguous(), W[:, E:].contiguous(), eighth(-1, 1, 4 * H), eighth(-1, 1, 4 * H),
         torch.zeros(case.V, H), torch.zeros(case.V)]
    X = make_inputs(case, gen)
    X["features"], X["h0"], X["c0"] = eighth(-2, 2, B, E), eighth(-1, 1, 1, B, H), eighth(-1, 1, 1, B, H)
    return P, X


def exact_gumbel(case, gen):
    """w_out = 0, T = 1, per vocabulary tile j one entry with bias 0, one with bias -k_j that draws the SAME uniform, the rest at -200:
    part_m[t, b, j] is the device's g(u) itself and part_s = 1 + exp(x) with x = fl(fl(g - k) - g) known exactly."""
    P = make_params(case, gen)
    P[-2].zero_()
    nb = case.nblk
    j = torch.arange(nb)
    ia, ib = j * KTILE + (j * 7) % KTILE, j * KTILE + (j * 7 + 21) % KTILE
    k = 0.25 * (1 + j % 12).float()
    P[-1].fill_(-200.0)
    P[-1][ia], P[-1][ib] = 0.0, -k
    X = make_inputs(case, gen)
    X["T"] = 1.0
    u = X["u"]
    n = u[:, :, ia].numel()
    edge = torch.cat([1.0 - 2.0 ** -torch.arange(1, 25).float(), 2.0 ** -torch.arange(1, 60).float(), torch.zeros(1)])    # towards 1, towards 0, 0
    ua = u[:, :, ia].reshape(-1)
    ua[:edge.numel()] = edge
    u[:, :, ia] = ua.view(case.L, case.B, nb)
    u[:, :, ib] = u[:, :, ia]
    assert n > 4 * edge.numel()
    return P, X, ia, ib, k


def tie_params(case, gen, pair):
    """pretrain, w_out = 0, integer biases in [-3, 3] and the maximum 5 at both indices of `pair`."""
    P = make_params(case, gen)
    P[-2].zero_()
    P[-1] = torch.randint(-3, 4, (case.V,), generator=gen).float()
    P[-1][list(pair)] = 5.0
    return P


SEED = 303


def data(case):
    """The parameters and inputs every test of a case uses."""
    gen = torch.Generator().manual_seed(SEED)
    return make_params(case, gen), make_inputs(case, gen)


def images(case, P):
    """The weight images gic_decoder_prepare keeps: [w_ih | w_hh] and its transpose and w_out in the compute dtype, b_ih + b_hh in f32."""
    td = TD[case.dtype]
    wcat = [torch.cat([P[1 + 4 * l], P[2 + 4 * l]], 1).to(td) for l in range(case.NL)]
    return {"wcat": wcat, "wcat_t": [w.t().contiguous() for w in wcat], "wout": P[-2].to(td),
            "bsum": [P[3 + 4 * l] + P[4 + 4 * l] for l in range(case.NL)]}


def new_state(case):
    """State, `out` and `ids` as DecoderEngine.alloc_state shapes them (CPU); `part` split into its three planes."""
    c, td = case, TD[case.dtype]
    nan = float("nan")
    st = {"xh": [torch.full((c.L + 1, c.B, c.ldx(l)), nan, dtype=td) for l in range(c.NL)],
          "gates": [torch.full((c.L, c.B, 4 * c.H), nan) for _ in range(c.NL)],
          "c": [torch.full((c.L + 1, c.B, c.H), nan) for _ in range(c.NL)],
          "hout": torch.full((c.B, c.L, c.H), nan, dtype=td), "out": torch.full((c.B, c.L, c.V), nan, dtype=td),
          "ids": torch.full((c.B, c.L), -7, dtype=torch.int64), "part_m": None, "part_s": None, "key": None}
    if select(case)["fwd"] == "fused":
        st.update(part_m=torch.full((c.L, c.B, c.nblk), nan), part_s=torch.full((c.L, c.B, c.nblk), nan), key=torch.full((c.L, c.B), -7, dtype=torch.int64))
    return st


def new_ws(case):
    c, td = case, TD[case.dtype]
    nan = float("nan")
    return {"dlogits": torch.full((c.B, c.L, c.V), nan, dtype=td), "dhout": torch.full((c.B, c.L, c.H), nan),
            "dgates": [torch.full((c.L, c.B, 4 * c.H), nan, dtype=td) for _ in range(c.NL)],
            "dxh": [torch.full((c.L + 1, c.B, c.ldx(l)), DXH_FILL) for l in range(c.NL)],
            "dc": [torch.full((c.B, c.H), nan) for _ in range(c.NL)]}


def new_grads(case, P):
    return [torch.full(p.shape, float("nan")) for p in P] + [torch.full((case.B, case.E), float("nan"))]


def split_part(case, part):
    """st["part"] as sample_fwd_fused lays it out: [L][B][tiles] maxima, the same of sums, then (8-byte aligned) [L][B] 64-bit keys
    (ordered float << 32 | ~index); returns (part_m, part_s, key index, key value)."""
    c = case
    per = c.L * c.B * c.nblk
    assert part.numel() == 2 * per + 2 * c.L * c.B + 4, "decoder_step_part_floats"
    off = (2 * per + 1) & ~1
    key = part[off:off + 2 * c.L * c.B].clone().view(torch.int64).view(c.L, c.B)
    idx = (~key) & 0xFFFFFFFF
    o = (key >> 32) & 0xFFFFFFFF
    b = torch.where(o >= 0x80000000, o & 0x7FFFFFFF, (~o) & 0xFFFFFFFF)                   # the float's bits back from their ordered form
    val = torch.where(b >= 0x80000000, b - (1 << 32), b).to(torch.int32).view(torch.float32)
    return part[:per].view(c.L, c.B, c.nblk), part[per:2 * per].view(c.L, c.B, c.nblk), idx, val


def truncate_bf16(x):
    """fp64 -> bf16 by truncation of the f32 bits (the `truncate` mutation)."""
    return (x.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ---------------------------------------------------------------------------------------------------------------- forward
def gumbel(u32, k):
    """fp64 g(u) of the f32 uniforms and the bound on the device's (module docstring) with the logarithm's constant k."""
    a = u32.double() + EPS32
    l1 = torch.log(a)
    a2 = EPS32 - l1
    g = -torch.log(a2)
    dg = (U + k * U * l1.abs().clamp_min(1.0) + U * a2) / a2 + k * U * g.abs().clamp_min(1.0)
    return g, dg


def vocab_y(case, P, img, X, h, t, mut=None):
    """fp64 y [B, V] of step t from the device's h [B, H] and its bound."""
    c, bf = case, case.dtype == "bf16"
    W, b = img["wout"].double(), P[-1].double()
    if mut == "quad_no_bias":
        b = b.clone()
        b[c.V - 4:] = 0
    o = h.double() @ W.t()
    ob = o + b
    bnd = sum_bound(c.H, h.double().abs() @ W.abs().t() + b.abs(), None)
    if c.pretrain:
        return ob, bnd
    g, dg = gumbel(X["u"][t], K_LOG_FAST if bf else K_LIBM)
    T = float(X["T"])
    y = (ob + g) * T
    return y, (bnd + dg + U * (ob.abs() + (ob + g).abs())) * abs(T) + U * y.abs()


def tiles(case, y, fill):
    """[B, V] -> [B, tiles, 64], the partial tile padded with `fill`."""
    pad = case.nblk * KTILE - case.V
    return torch.cat([y, torch.full((y.shape[0], pad), fill, dtype=y.dtype)], 1).view(y.shape[0], case.nblk, KTILE)


def first_argmax(y):
    m = y.max(1, keepdim=True).values
    idx = torch.arange(y.shape[1]).expand_as(y)
    return torch.where(y == m, idx, torch.full_like(idx, y.shape[1])).min(1).values


def clamp_ids(f, V):
    return f.clamp(0, V - 1)


def forced_mask(case, X, t):
    """Rows whose token of step t is forced."""
    if X["force_ids"] is None:
        return torch.zeros(case.B, dtype=torch.bool)
    if X["force_len"] is None:
        return torch.ones(case.B, dtype=torch.bool)
    return t < X["force_len"].long()


def cell_forward(emit, bf, a, W, bs, gates, c_prev, c_next, h_view, am=None, after_c=None):
    """One cell step by the rules of the module docstring (shared with tests/attn_cases.py): the gates from the device's input row
    a [B, ldx] (fp64; `am`: a mutated copy that forms the reference instead), c from the device's gates, h from the device's c.
    emit(stage, view, ref, bound) compares or fills."""
    H, ldx = c_prev.shape[1], a.shape[1]
    lip = torch.cat([torch.full((H,), 0.25), torch.full((H,), 0.25), torch.ones(H), torch.full((H,), 0.25)]).double()
    kk = torch.cat([torch.full((H,), K_SIG), torch.full((H,), K_SIG), torch.full((H,), K_TANH), torch.full((H,), K_SIG)]).double()
    pre = (a if am is None else am) @ W.t() + bs
    pb = sum_bound(ldx, a.abs() @ W.abs().t() + bs.abs(), None)
    ref = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])], 1)
    emit("gates", gates, ref, lip * pb + kk * U * ref.abs())
    G = gates.double()
    gi, gf, gg, go = G[:, :H], G[:, H:2 * H], G[:, 2 * H:3 * H], G[:, 3 * H:]
    cp = c_prev.double()
    emit("c", c_next, gf * cp + gi * gg, 3 * U * ((gf * cp).abs() + (gi * gg).abs()))
    if after_c is not None:
        after_c()
    h_ref = go * torch.tanh(c_next.double())
    emit("h", h_view, h_ref, (K_TANH + 2) * U * h_ref.abs() + (U8 * h_ref.abs() if bf else 0.0))


def cell_backward(emit, bf, dh, dhb, gates, c_prev, c_cur, carry, dgates, carry_f=True):
    """d_gates of one cell step from dh [B, H] and its bound dhb, the saved gates and cell states and the cell-gradient carry (its
    fp64 value, its bound); returns the carry of the step before (shared with tests/attn_cases.py).  carry_f False: the `dc_no_f`
    mutation."""
    H = c_prev.shape[1]
    G = gates.double()
    gi, gf, gg, go = G[:, :H], G[:, H:2 * H], G[:, 2 * H:3 * H], G[:, 3 * H:]
    cp, tc = c_prev.double(), torch.tanh(c_cur.double())
    q = 1 - tc * tc
    S, Sb = carry
    term = dh * go * q
    D = S + term
    # tanhf errs by K_TANH u |tc|, so 1 - tc^2 by (2 K_TANH + 1) u tc^2 + u (1 + tc^2); two products; the sum
    Eb = Sb + dhb * (go * q).abs() + U * (dh * go).abs() * ((2 * K_TANH + 2) * tc * tc + 1) + 2 * U * term.abs() + U * (S.abs() + term.abs())
    # d_gate = dc (or dh) times a product of three factors, one of them 1 - x (terms before the cancellation: 1 + |x|): 4 u
    parts = [(D, Eb, gg * gi * (1 - gi), gg.abs() * gi * (1 + gi)),
             (D, Eb, cp * gf * (1 - gf), cp.abs() * gf * (1 + gf)),
             (D, Eb, gi * (1 - gg * gg), gi * (1 + gg * gg)),
             (dh, dhb, tc * go * (1 - go), tc.abs() * go * (1 + go) * (1 + K_TANH / 4))]
    ref = torch.cat([v * f for v, _, f, _ in parts], 1)
    bnd = torch.cat([e * f.abs() + 4 * U * v.abs() * m for v, e, f, m in parts], 1)
    emit("dgates", dgates, ref, bnd + (U8 * ref.abs() if bf else 0.0))
    return (D * gf, Eb * gf.abs() + U * (D * gf).abs()) if carry_f else (D, Eb)


def run_forward(case, P, img, X, st, rep=None, mut=None, exact=False, near=None):
    """Walk the forward stages over `st` (new_state's keys).  rep: check; None: fill.  `mut`: a mutation of the fill.  exact: the tie
    regime (ids are the FIRST maximal index, bit for bit).  near: a list that receives (rows without a clear margin, rows)."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, L, V, E, H, NL = c.B, c.L, c.V, c.E, c.H, c.NL
    fused = select(c)["fwd"] == "fused"
    cast = (lambda x: truncate_bf16(x)) if (mut == "truncate" and bf) else (lambda x: x.to(td))

    def emit(stage, view, ref, bound):
        if rep is None:
            view.copy_(cast(ref) if view.dtype == td and td != torch.float32 else ref.to(view.dtype))
        else:
            rep.check(stage, view, ref, bound)

    def same(stage, view, want):
        if rep is None:
            view.copy_(want)
        else:
            rep.bits(stage, view, want)

    r = lambda ref: U8 * ref.abs() if bf else 0.0
    # 2. slot 0: features, the initial states or zeros
    same("slot0", st["xh"][0][0][:, :E], X["features"].to(td))
    for l in range(NL):
        same("slot0", st["xh"][l][0][:, c.din(l):], X["h0"][l].to(td) if X["h0"] is not None else torch.zeros(B, H, dtype=td))
        same("slot0", st["c"][l][0], X["c0"][l] if X["c0"] is not None else torch.zeros(B, H))
    unclear = 0
    for t in range(L):
        # 4. the cell, layer by layer, each link from the device's own buffers upstream of it
        for l in range(NL):
            din, ldx = c.din(l), c.ldx(l)
            a = st["xh"][l][t].double()
            am = None
            if l == 0 and mut == "k_tail_missing":
                am = a.clone()
                am[:, ldx - 8:] = 0
            if l == 0 and mut == "seam_swapped":
                am = a.clone()
                am[:, din - 8:din], am[:, din:din + 8] = a[:, din:din + 8], a[:, din - 8:din]

            def after_c(l=l, t=t):
                if mut == "row64_unwritten" and rep is None and B > 64 and l == NL - 1 and t == L - 1:
                    st["c"][l][t + 1][64] = float("nan")

            hv = st["xh"][l][t + 1][:, din:]
            cell_forward(emit, bf, a, img["wcat"][l].double(), img["bsum"][l].double(), st["gates"][l][t], st["c"][l][t], st["c"][l][t + 1], hv,
                         am=am, after_c=after_c)
            up = st["xh"][l + 1][t][:, :H] if l + 1 < NL else st["hout"][:, t]
            same("h copies", up, hv)
            if mut == "h_up_ulp" and rep is None and l + 1 < NL:
                up.copy_((up.contiguous().view(BITS[td]) + 1).view(td))
        # 5. the vocabulary step
        y, yb = vocab_y(c, P, img, X, st["hout"][:, t], t, mut if rep is None else None)
        ymax = y.max(1).values
        bmax = yb.max(1).values
        top2 = y.topk(2, 1).values
        unclear += int(((top2[:, 0] - top2[:, 1]) <= 2 * bmax).sum()) if not exact else 0
        am = first_argmax(y)
        if rep is None and mut == "tie_later":
            last = torch.where(y == ymax[:, None], torch.arange(V).expand_as(y), torch.full((B, V), -1)).max(1).values
            am = last
        if fused:
            yt, bt = tiles(c, y, -float("inf")), tiles(c, yb, 0.0)
            emit("part_m", st["part_m"][t], yt.max(2).values, bt.max(2).values)
            if c.pretrain:
                same("part_s", st["part_s"][t], torch.zeros(B, c.nblk))
            else:
                x = yt - st["part_m"][t].double()[:, :, None]
                e = torch.exp(x)
                ke = K_EXP_FAST if bf else K_LIBM
                xa = torch.where(torch.isinf(x), torch.zeros_like(x), x.abs())
                sb = (e * (torch.expm1(bt + U * xa) + ke * U * (1 + xa))).sum(2) + (KTILE + 4) * U * e.sum(2)
                es = e
                if rep is None and mut == "part_s_subtile":
                    es = e.clone()
                    es[:, :, 16:32] = 0
                emit("part_s", st["part_s"][t], es.sum(2), sb)
            if rep is None:
                st["key"][t] = am
            else:
                k = st["key"][t]
                ok = (k >= 0) & (k < V)
                at = y.gather(1, k.clamp(0, V - 1)[:, None])[:, 0]
                rep.exact("key", ok & (k == am) if exact else ok & (at >= ymax - 2 * bmax), "are not the first index of / within twice the bound of the row maximum")
        # 6. ids and out
        fm = forced_mask(c, X, t)
        forced = clamp_ids(X["force_ids"][:, t], V) if X["force_ids"] is not None else torch.zeros(B, dtype=torch.int64)
        if rep is None:
            st["ids"][:, t] = torch.where(fm, forced, am)
        else:
            ids = st["ids"][:, t]
            ok = (ids >= 0) & (ids < V)
            at = y.gather(1, ids.clamp(0, V - 1)[:, None])[:, 0]
            good = ok & (ids == am) if exact else ok & (at >= ymax - 2 * bmax)
            if fused:
                good = good & (ids == st["key"][t])
            rep.exact("ids", torch.where(fm, ids == forced, good), "are not the forced id / the first index of / within twice the bound of the row maximum")
        if c.pretrain:
            if exact and rep is not None:
                rep.bits("out", st["out"][:, t], y.to(td))
            else:
                emit("out", st["out"][:, t], y, yb + r(y))
        else:
            p = torch.softmax(y, 1)
            x = (y - ymax[:, None]).abs()
            ke = K_EXP_FAST if bf else K_LIBM
            rel = torch.expm1(2 * bmax)[:, None] + U * (2 * ke * (1 + x) + V + c.nblk + 16)
            pm = p
            if rep is None and mut == "out_neighbour_scale" and fused:
                pm = p.clone()
                m = tiles(c, y, -float("inf")).max(2).values
                pm[:, :KTILE] = p[:, :KTILE] * torch.exp(m[:, 1] - m[:, 0])[:, None]
            emit("out", st["out"][:, t], pm, p * rel + (2 if fused else 1) * R_OUT(p, bf))
        # 3. the x rows of the next step: the embedding row of the token in the compute dtype
        if t + 1 < L:
            same("xrows", st["xh"][0][t + 1][:, :E], P[0][st["ids"][:, t].clamp(0, V - 1)].to(td))
    if near is not None:
        near.append((unclear, L * B))


def R_OUT(p, bf):
    """One bf16 rounding of a probability: half an ulp is up to 2^-8 |ref| (2^-9 only at the top of a binade)."""
    return U8 * p.abs() if bf else 0.0


def check_images(case, P, shadow, rep):
    """1. the weight images: the compute-dtype cast of [w_ih | w_hh], its exact transpose, w_out's cast, fl32(b_ih + b_hh)."""
    want = images(case, P)
    for l in range(case.NL):
        rep.bits("wcat", shadow["wcat"][l], want["wcat"][l])
        rep.bits("wcat_t", shadow["wcat_t"][l], shadow["wcat"][l].t().contiguous())
        rep.bits("bsum", shadow["bsum"][l], want["bsum"][l])
    if shadow.get("wout") is not None:
        rep.bits("wout", shadow["wout"], want["wout"])


# ---------------------------------------------------------------------------------------------------------------- backward
def run_backward(case, P, img, X, st, ws, grads, rep=None, mut=None, state_grads=True, only=None, det=False):
    """Walk the backward stages (sample_bwd with phases = 7 if state_grads else 3).  st: the saved forward state with `out` and `ids`;
    ws: new_ws's keys; grads: new_grads' list.  only: just these stages.  det: deterministic mode, in which the two bias gradients (one
    column sum stored twice) are bit-equal; otherwise three or more block rows add into each by atomics of their own, in any order."""
    c, td, bf = case, TD[case.dtype], case.dtype == "bf16"
    B, L, V, E, H, NL = c.B, c.L, c.V, c.E, c.H, c.NL
    BL = B * L
    fused = select(c)["bwd"] == "fused"
    T = float(X["T"])
    want = lambda s: only is None or s in only

    def emit(stage, view, ref, bound):
        if not want(stage):
            return
        if rep is None:
            view.copy_(ref.to(view.dtype))
        else:
            rep.check(stage, view, ref, bound)

    r = lambda ref: U8 * ref.abs() if bf else 0.0
    # 7. softmax backward
    dp = X["d_out"].to(td).double()
    if not c.pretrain:
        p = st["out"].double()
        s = (p * dp).sum(2, keepdim=True)
        sb = (V + 4) * U * (p * dp).abs().sum(2, keepdim=True)
        ref = T * p * (dp - s)
        emit("dlogits", ws["dlogits"], ref, (T * p).abs() * sb + 3 * U * (T * p).abs() * (dp.abs() + s.abs()) + r(ref))
        dlog = ws["dlogits"].double().reshape(BL, V)
    else:
        dlog = dp.reshape(BL, V)
    # 8. the output layer
    W, hout = img["wout"].double(), st["hout"].double().reshape(BL, H)
    emit("dhout", ws["dhout"].view(BL, H), dlog @ W, sum_bound(V, dlog.abs() @ W.abs(), None))
    emit("d_w_out", grads[1 + 4 * NL], dlog.t() @ hout, sum_bound(BL, dlog.abs().t() @ hout.abs(), None))
    emit("d_b_out", grads[2 + 4 * NL], dlog.sum(0), sum_bound(BL, dlog.abs().sum(0), None))
    # 9. BPTT: d_gates in reverse order; the cell-gradient carry and its bound travel along the chain in fp64
    if want("dgates"):
        Wt = [w.double() for w in img["wcat_t"]]                              # [ldx, 4H]
        carry = [(torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)) for _ in range(NL)]
        for t in range(L - 1, -1, -1):
            for l in range(NL - 1, -1, -1):
                din = c.din(l)
                if l == NL - 1:
                    dh = ws["dhout"][:, t].double()
                    mag, n = dh.abs(), 1
                else:
                    up, Wu = ws["dgates"][l + 1][t].double(), Wt[l + 1][:H]
                    dh, mag, n = up @ Wu.t(), up.abs() @ Wu.abs().t(), 4 * H
                    if mut == "no_upper_term":
                        dh = torch.zeros_like(dh)
                if t + 1 < L:
                    nx, Wr = ws["dgates"][l][t + 1].double(), Wt[l][din:]
                    dh, mag, n = dh + nx @ Wr.t(), mag + nx.abs() @ Wr.abs().t(), n + 4 * H
                dhb = (n + 4) * U * mag
                carry[l] = cell_backward(emit, bf, dh, dhb, st["gates"][l][t], st["c"][l][t], st["c"][l][t + 1], carry[l], ws["dgates"][l][t],
                                         carry_f=mut != "dc_no_f")
        for l in range(NL):
            emit("dc", ws["dc"][l], carry[l][0], carry[l][1])
    # 10. the input gradients: d[x | h] = d_gates Wcat.  Fused: the x columns of layer 0 and (state gradients) the h columns of slot 0;
    # generic: every slot, slot L zero.  The rest keeps what it held.
    if want("dxh"):
        for l in range(NL):
            din, Wc = c.din(l), img["wcat"][l].double()
            dg = ws["dgates"][l].double()
            keep = torch.ones(L + 1, B, c.ldx(l), dtype=torch.bool)
            full = dg @ Wc                                                    # [L, B, ldx]
            fb = sum_bound(4 * H, dg.abs() @ Wc.abs(), None)
            if not fused:
                emit("dxh", ws["dxh"][l][:L], full, fb)
                emit("dxh", ws["dxh"][l][L], torch.zeros(B, c.ldx(l), dtype=torch.float64), 0.0)
                keep[:] = False
            else:
                if l == 0:
                    emit("dxh", ws["dxh"][0][:L, :, :E], full[:, :, :E], fb[:, :, :E])
                    keep[:L, :, :E] = False
                if state_grads:
                    emit("dxh", ws["dxh"][l][0][:, din:], full[0][:, din:], fb[0][:, din:])
                    keep[0, :, din:] = False
            if rep is not None:
                rep.exact("dxh keep", (ws["dxh"][l] == DXH_FILL) | ~keep, "of what the route does not write changed")
    # 11. parameter and input gradients
    for l in range(NL):
        if not any(want(s) for s in ("d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")):
            break
        din = c.din(l)
        A, xh = ws["dgates"][l].double().reshape(BL, 4 * H), st["xh"][l][:L].double().reshape(BL, c.ldx(l))
        emit("d_w_ih", grads[1 + 4 * l], A.t() @ xh[:, :din], sum_bound(BL, A.abs().t() @ xh[:, :din].abs(), None))
        emit("d_w_hh", grads[2 + 4 * l], A.t() @ xh[:, din:], sum_bound(BL, A.abs().t() @ xh[:, din:].abs(), None))
        emit("d_b_ih", grads[3 + 4 * l], A.sum(0), sum_bound(BL, A.abs().sum(0), None))
        emit("d_b_hh", grads[4 + 4 * l], A.sum(0), sum_bound(BL, A.abs().sum(0), None))
        if rep is not None and det and want("d_b_hh"):
            rep.bits("d_b_ih == d_b_hh", grads[3 + 4 * l], grads[4 + 4 * l])
    if want("d_features"):
        if rep is None:
            grads[3 + 4 * NL].copy_(ws["dxh"][0][0][:, :E])
        else:
            rep.bits("d_features", grads[3 + 4 * NL], ws["dxh"][0][0][:, :E])
    if want("d_embed"):
        ge, gm = torch.zeros(V, E, dtype=torch.float64), torch.zeros(V, E, dtype=torch.float64)
        if L > 1:
            idx = st["ids"][:, :L - 1].t().reshape(-1).clamp(0, V - 1)        # (t - 1, b) order
            src = ws["dxh"][0][1:L, :, :E].double().reshape(-1, E)
            if mut == "embed_once":
                ge[idx] = src
            else:
                ge.index_add_(0, idx, src)
            gm.index_add_(0, idx, src.abs())
        emit("d_embed", grads[0], ge, sum_bound(B * (L - 1), gm, None))


def repeats(ids, L):
    """How many of the scattered tokens repeat an earlier one (d_embed must accumulate them)."""
    used = ids[:, :L - 1].reshape(-1)
    return used.numel() - used.unique().numel()
