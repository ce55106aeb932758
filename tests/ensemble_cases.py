"""ensemble_mix (csrc/ensemble.hip, gicap.h gic_ensemble_mix): the case table, an fp64 reference, the per-element bound, a plain f32
emulation of the kernel's order and seeded faults, by the method of tests/aux_cases.py.  Behind tests/test_ensemble_cases.py (no GPU:
the emulation against the bound, the faults outside it) and tests/test_gpu_ensemble_mix.py (every case on the GPU).  Nothing here
touches a GPU.

The kernel.  logits f32 [M][rows][V] -> z f32 [rows][V]; weights normalised in double, w_m and log w_m rounded to f32.  A row is T = 64
lanes (V <= 1024: one wave) or T = 256 (four waves).  Pass 1, per member: lane j folds the 16-byte vectors j, j + T, ... into an online
(max, sum-exp) pair -- per vector n = max(the four, max so far), s = s exp(max - n) + (((e0 + e1) + e2) + e3) -- then, for j < V % 4,
tail column 4 (V / 4) + j; the pairs are merged over the wave by an xor butterfly (6 levels) and over the four waves in order.  lse_m =
max + log(s).  Pass 2, per element: prob  t_m = (log w_m - lse_m) + l_m, a = max t_m, z = a + log(sum_m exp(t_m - a)) (m in order);
logprob  z = sum_m w_m (l_m - lse_m) (m in order).

Bound (the rounding model of tests/aux_cases.py: u = 2^-24 per f32 operation on the magnitudes of its operands, expf 1 ulp = 2 u, logf
2 ulp = 4 u; a contracted fma rounds less often than counted).
  s (pass 1)   Every element x_i enters s as c_i = exp(-d_i), d_i = max - x_i, through a chain of exps whose arguments are all <= 0 and
               telescope to -d_i (the running maximum only grows along a lane, a butterfly and the wave fold), so the argument roundings
               cost at most u d_i c_i in all; sum_i d_i c_i / s = H(p) - log s <= log V for p = c / s (s >= 1).  Along its path an
               element passes NE exps (its own, one rescale per trip of its lane, the tail merge, 6 butterfly levels, the wave fold)
               and NO roundings of multiplies and adds (3 adds in its vector, then a multiply and an add per trip, tail merge, level and
               wave).  rel(s) = u (log V + EXP NE + NO).
  lse          d log s = rel(s); logf costs LOG u |log s| <= LOG u log V; the add u (|max| + log V):
               e_lse = u (log V + EXP NE + NO + LOG log V + |max| + log V).
  prob         t_m carries E_m = e_lse_m + u |log w_m| (its rounding to f32) + u (|log w_m| + |lse_m|) + u (|log w_m - lse_m| + |l_m|).
               z = logsumexp_m t_m moves by at most max_m E_m (its gradient is a softmax).  The sum over m: by the argument above
               rel(S) = u (log M + EXP + M - 1); logf LOG u log M; the last add u (|a| + log M).
  logprob      lp_m = l_m - lse_m carries e_lse_m + u (|l_m| + |lse_m|); w_m lp_m costs 2 u |w_m lp_m| (w_m's rounding, the multiply); the
               M - 1 adds (M - 1) u sum_m |w_m lp_m|.
  floor        terms below 2^-126 may be flushed: (V + M) 2^-126, next to the checker's own floor.
The bound is derived, not fitted: WORST_OBSERVED records the largest err / bound seen on an MI355X and is never asserted against."""
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests.aux_cases import EXP, LOG, check, gen_for
from tests.disc_cases import U

F64 = torch.float64
MODES = ("prob", "logprob")
WAVE, WAVE_ROW_V = 64, 1024          # ensemble.hip kWaveRowV: up to here a row is one wave's
FAULTS = ("drop_normaliser", "raw_weights", "skip_tail", "swap_mode")

# Largest err / bound per mode measured on an MI355X by tests/test_gpu_ensemble_mix.py (recorded, never asserted against).
WORST_OBSERVED = {"prob": 0.611, "logprob": 0.473}


class Case(NamedTuple):
    id: str
    M: int
    rows: int
    V: int
    mode: str
    weights: Optional[Tuple[float, ...]]      # None: uniform
    scale: float = 80.0                        # logits uniform in [-scale, scale]
    special: str = ""                          # "const": member 0's row 0 is constant; "dominate": member 0 leads by 60 nats


UNEVEN = {1: (1.0,), 2: (0.7, 0.3), 3: (0.7, 0.2, 0.1), 4: (0.4, 0.3, 0.2, 0.1)}


def _cases():
    out = []
    for mode in MODES:
        for M in (1, 2, 4):
            for rows in (1, 3, 65):
                for V in (2, 5, 64, 67, 1024, 1028, 10000):      # below one vector, the tail, both sides of the one-wave limit, the workload's
                    w = None if rows == 3 else UNEVEN[M]
                    out.append(Case(f"{mode}-M{M}-r{rows}-V{V}", M, rows, V, mode, w))
        out += [
            Case(f"{mode}-M3-uneven", 3, 3, 67, mode, (0.7, 0.2, 0.1)),
            Case(f"{mode}-M3-V10000", 3, 3, 10000, mode, (0.7, 0.2, 0.1)),
            Case(f"{mode}-raw-weights", 3, 3, 67, mode, (7.0, 2.0, 1.0), 2.0),          # given un-normalised
            Case(f"{mode}-small-tail", 2, 3, 5, mode, (0.7, 0.3), 1.0),
            Case(f"{mode}-1e4", 2, 3, 1028, mode, (0.7, 0.3), 1e4),
            Case(f"{mode}-const-row", 2, 3, 67, mode, None, 80.0, "const"),
            Case(f"{mode}-dominate", 3, 3, 67, mode, (0.7, 0.2, 0.1), 3.0, "dominate"),
        ]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# the case in which each seeded fault must show (skip_tail: a tail column of visible probability)
FAULT_CASES = {"drop_normaliser": "M3-uneven", "raw_weights": "raw-weights", "skip_tail": "small-tail", "swap_mode": "M3-uneven"}


def make_inputs(case: Case):
    """(logits f32 [M, rows, V], weights as the caller gives them: a tuple of M floats)."""
    g = gen_for("ensemble_mix/" + case.id)
    x = ((torch.rand(case.M, case.rows, case.V, generator=g, dtype=F64) * 2 - 1) * case.scale).float()
    if case.special == "const":
        x[0, 0, :] = 1.25
    if case.special == "dominate":                 # member 0 puts everything on token 1: the others' terms underflow there in prob
        x[0, :, 1] += 120.0
        x[1:, :, 1] -= 60.0
    return x, tuple(case.weights or [1.0] * case.M)


def normalised(weights):
    """(w, log w) in double from the f32 values the library reads, as ensemble.hip forms them."""
    w = np.asarray([np.float32(v) for v in weights], dtype=np.float64)
    w = w / w.sum()
    return w, np.log(w)


def reference(logits, weights, mode):
    """fp64: z [rows, V]."""
    x = logits.double()
    w, logw = (torch.from_numpy(a) for a in normalised(weights))
    lp = x - torch.logsumexp(x, -1, keepdim=True)
    if mode == "prob":
        return torch.logsumexp(lp + logw.view(-1, 1, 1), 0)
    return (lp * w.view(-1, 1, 1)).sum(0)


def lanes(V):
    return WAVE if V <= WAVE_ROW_V else 4 * WAVE


def bound(logits, weights, mode):
    """The per-element bound of the module docstring, f64 [rows, V]."""
    x = logits.double()
    M, rows, V = x.shape
    w, logw = (torch.from_numpy(a).view(-1, 1, 1) for a in normalised(weights))
    T = lanes(V)
    trips = -(-(V // 4) // T)
    folds = trips + 1 + 6 + (4 if T > WAVE else 0)          # rescales: per trip, the tail merge, the butterfly, the wave fold
    NE, NO = 1 + folds, 3 + 2 * folds
    lnV, lnM = math.log(V), math.log(M)
    mx = x.amax(-1, keepdim=True)
    lse = torch.logsumexp(x, -1, keepdim=True)
    e_lse = U * (lnV + EXP * NE + NO + LOG * lnV + mx.abs() + lnV)          # [M, rows, 1]
    floor = (V + M) * 2.0 ** -126
    if mode == "prob":
        c = logw - lse
        t = c + x
        E = e_lse + U * logw.abs() + U * (logw.abs() + lse.abs()) + U * (c.abs() + x.abs())
        a = t.amax(0)
        return E.amax(0) + U * (lnM + EXP + M - 1) + LOG * U * lnM + U * (a.abs() + lnM) + floor
    lp = x - lse
    terms = (w * lp).abs().sum(0)
    return (w * (e_lse + U * (x.abs() + lse.abs()))).sum(0) + (2 + M - 1) * U * terms + floor


def bound_upper(M, V, mag, mode, w_min=None):
    """The bound above for ANY logits of magnitude <= mag and normalised weights >= w_min (None: uniform): every |l|, |max| <= mag,
    |lse| <= mag + log V, |log w| <= log(1 / w_min).  What a search's score may differ by per token because of the mix."""
    T = lanes(V)
    trips = -(-(V // 4) // T)
    folds = trips + 1 + 6 + (4 if T > WAVE else 0)
    NE, NO = 1 + folds, 3 + 2 * folds
    lnV, lnM = math.log(V), math.log(M)
    lw = math.log(M if w_min is None else 1.0 / w_min)
    lse = mag + lnV
    e_lse = U * (lnV + EXP * NE + NO + LOG * lnV + mag + lnV)
    floor = (V + M) * 2.0 ** -126
    if mode == "prob":
        E = e_lse + U * lw + U * (lw + lse) + U * (lw + lse + mag)
        return E + U * (lnM + EXP + M - 1) + LOG * U * lnM + U * (lw + lse + mag + lnM) + floor
    return e_lse + U * (mag + lse) + (2 + M - 1) * U * (mag + lse) + floor


# ---------------------------------------------------------------------------------------------------------------- f32 emulation
def _merge(m, s, m2, s2):
    """pair_merge of ensemble.hip on f32 arrays."""
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.maximum(m, m2)
        a = np.where(m == n, s, s * np.exp(m - n, dtype=np.float32))
        b = np.where(m2 == n, s2, s2 * np.exp(m2 - n, dtype=np.float32))
    return n, (a + b).astype(np.float32)


def emulate(logits, weights, mode, fault=None):
    """The kernel in plain f32 numpy, in the kernel's order (module docstring).  ``fault``: one of FAULTS."""
    x = logits.numpy().astype(np.float32)
    M, rows, V = x.shape
    T = lanes(V)
    nvec, tail = V // 4, V % 4
    f = np.float32
    if fault == "raw_weights":
        w = np.asarray(weights, dtype=np.float64)
        logw = np.log(w)
    else:
        w, logw = normalised(weights)
    w, logw = w.astype(f), logw.astype(f)
    if fault == "swap_mode":
        mode = "logprob" if mode == "prob" else "prob"
    mx = np.full((M, rows, T), -np.inf, dtype=f)
    sm = np.zeros((M, rows, T), dtype=f)
    lane = np.arange(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-(-nvec // T)):
            i = lane + k * T
            ok = i < nvec
            idx = 4 * np.where(ok, i, 0)
            v = [x[:, :, idx + q] for q in range(4)]
            n = np.maximum(np.maximum(np.maximum(v[0], v[1]), np.maximum(v[2], v[3])), mx)
            e = ((np.exp(v[0] - n, dtype=f) + np.exp(v[1] - n, dtype=f)) + np.exp(v[2] - n, dtype=f)) + np.exp(v[3] - n, dtype=f)
            s_new = np.where(mx == n, sm, sm * np.exp(mx - n, dtype=f)) + e
            mx, sm = np.where(ok, n, mx), np.where(ok, s_new, sm).astype(f)
        if tail and fault != "skip_tail":
            tl = lane < tail
            xt = x[:, :, 4 * nvec + np.where(tl, lane, 0)]
            n, s_new = _merge(mx, sm, xt, np.ones_like(xt))
            mx, sm = np.where(tl, n, mx), np.where(tl, s_new, sm)
        o = 1
        while o < WAVE:                                     # the xor butterfly inside each wave
            mx, sm = _merge(mx, sm, mx[:, :, lane ^ o], sm[:, :, lane ^ o])
            o <<= 1
        m_row, s_row = mx[:, :, 0], sm[:, :, 0]
        for wv in range(1, T // WAVE):                      # the wave fold, in wave order
            m_row, s_row = _merge(m_row, s_row, mx[:, :, wv * WAVE], sm[:, :, wv * WAVE])
        lse = (m_row + np.log(s_row, dtype=f)).astype(f)[:, :, None]
        if fault == "drop_normaliser" and M > 1:
            lse[1] = 0
        if mode == "prob":
            t = ((logw[:, None, None] - lse).astype(f) + x).astype(f)
            a = t.max(0)
            s = np.zeros_like(a)
            for m in range(M):
                s = (s + np.exp(t[m] - a, dtype=f)).astype(f)
            z = a + np.log(s, dtype=f)
        else:
            z = np.zeros((rows, V), dtype=f)
            for m in range(M):
                z = (z + w[m] * (x[m] - lse[m]).astype(f)).astype(f)
    return torch.from_numpy(z.astype(f))


def check_case(case: Case, got, logits, weights):
    """``got`` against the fp64 reference within the bound: the largest err / bound (raises aux_cases.Mismatch)."""
    return check("ensemble_mix", case.id, "z", got, reference(logits, weights, case.mode), bound(logits, weights, case.mode))
