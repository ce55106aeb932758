"""The case matrix of the decode heads' workspace contract (tests/decode_ws.py): models, heads, terminations, each case's problem and
its float64 oracle.  Behind tests/test_decode_ws.py (no GPU: every f32 case is decidable by the oracle alone and ends as its
termination says) and tests/test_gpu_decode_ws.py.  Nothing here touches a GPU.

Shapes: the smallest that reach the edges.  V = 68: two vocabulary tiles, the second ragged (4 ids); V = 50: one ragged tile,
V % 4 != 0, the generic path; B * K = 12 rows: not a wave, no multiple of 16; B = 65, K = 8: 520 rows, past the fused kernels' 512."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import constrained_oracle as CO
from tests import diverse_beam_oracle as DO
from tests import ensemble_cases as EC
from tests import ensemble_oracle as EO
from tests import forced_beam_oracle as FO
from tests import philox_ref as PR
from tests import sample_oracle as SO
from tests.decode_ws import Dims

EOS, PAD = 2, 0
MODELS = {
    "lstm1": (Dims(3, 6, 68, 8, 16, 1), 4), "lstm2": (Dims(3, 6, 68, 8, 16, 2), 4), "generic": (Dims(3, 6, 50, 8, 16, 2), 4),
    "attn": (Dims(3, 5, 52, 8, 16, 1, 24, 9, 16), 4),
    "lstm1-b1k1": (Dims(1, 6, 68, 8, 16, 1), 1), "attn-b1k1": (Dims(1, 5, 52, 8, 16, 1, 24, 9, 16), 1),
    "rows520": (Dims(65, 6, 68, 8, 16, 1), 8),
}
CONS = dict(no_repeat_ngram=2, min_length=3, suppress_tokens=(1, 3))
C_OFF = dict(no_repeat_ngram=0, min_length=0, suppress_tokens=())
LSTM_SCALE, ATTN_SCALE = 3.0, 4.0
EOS_BIAS = {"ends": 12.0, "runs": -12.0}          # every image finishes by step 2 / nothing finishes before L
M_ENS = 2


class Head(NamedTuple):
    kind: str                   # beam / forced / sample / ens-beam / ens-sample
    lp: float = 0.0
    groups: int = 1
    diversity: float = 0.0
    cons: dict = C_OFF
    alphas: bool = False
    top_k: int = 0
    top_p: float = 1.0
    philox: bool = False        # the sampler draws from Philox(seed), not from noise_u
    mode: str = "prob"


HEADS = {
    "beam-lp0": Head("beam"), "beam-lp0.7": Head("beam", lp=0.7), "diverse": Head("beam", groups=2, diversity=1.0),
    "cbeam": Head("beam", cons=CONS), "forced": Head("forced"), "forced-cons": Head("forced", cons=CONS),
    "sample-noise-k5": Head("sample", top_k=5), "sample-noise-p0.9": Head("sample", top_p=0.9),
    "sample-seed-k5": Head("sample", top_k=5, philox=True), "sample-seed-p0.9": Head("sample", top_p=0.9, philox=True),
    "csample": Head("sample", cons=CONS), "ens-beam": Head("ens-beam", mode="prob"), "ens-sample": Head("ens-sample", top_k=5, mode="logprob"),
    "beam-alphas": Head("beam", alphas=True), "forced-alphas": Head("forced", alphas=True),
}
ATTN_ONLY = ("beam-alphas", "forced-alphas")
SMALL = ("beam-lp0", "sample-noise-k5")            # the heads of the B = 1, K = 1 and the 520-row models


class Case(NamedTuple):
    model: str
    head: str
    term: str

    @property
    def id(self):
        return f"{self.model}-{self.head}-{self.term}"


def _cases():
    out = []
    for model in MODELS:
        for head in HEADS:
            full = model in ("lstm1", "lstm2", "generic", "attn")
            if (full and (model == "attn" or head not in ATTN_ONLY)) or (not full and head in SMALL):
                out += [Case(model, head, term) for term in EOS_BIAS]
    return out


CASES = _cases()

# the seed of a case's problem where the default (1) leaves an image or a row undecided under the float64 oracle (a selection margin
# below 1e-4, a draw or nucleus margin below 1e-5), or does not end as its termination says: picked by running the oracle alone;
# tests/test_decode_ws.py::test_oracle_decides_every_case asserts every case
SEEDS = {"lstm1-diverse-runs": 2, "attn-beam-lp0-runs": 2, "attn-beam-lp0.7-runs": 2, "attn-beam-alphas-runs": 2, "rows520-beam-lp0-runs": 3}


def seed_of(case: Case, twin=False) -> int:
    return SEEDS.get(case.id, 1) + (500 if twin else 0)


def force_words(d: Dims) -> torch.Tensor:
    """C = 2 sets of D <= 2 ids per image, int32 [B, 2, 2] padded with -1: image 0 holds V - 1 (the ragged last tile) and a set of
    two, image 1 one id per set, image 2 one absent set (its beams outside the initial state stay dead).  No id is special or
    suppressed by CONS."""
    rows = [[[5, 9], [d.V - 1, -1]], [[7, -1], [11, 12]], [[6, -1], [-1, -1]]]
    return torch.tensor([rows[b % 3] for b in range(d.B)], dtype=torch.int32)


class Problem(NamedTuple):
    members: list               # M parameter lists (library order), float32 on the CPU
    feats: list                 # M [B, E]
    fmaps: list                 # M [B, P, C], or None
    noise_u: object             # [L, B * K, V] or None
    seed: int                   # the sampler's Philox seed
    force: object               # int32 [B, 2, 2] or None


def problem(case: Case, twin=False, seed=None) -> Problem:
    """The case's decoder(s) and inputs.  ``twin``: other weights and features for the same head, dims and K, with the <E> bias that
    ends every search early (it leaves a finished state behind)."""
    d, K = MODELS[case.model]
    h = HEADS[case.head]
    s = seed_of(case, twin) if seed is None else seed
    bias = EOS_BIAS["ends" if twin else case.term]
    M = M_ENS if h.kind.startswith("ens") else 1
    members, feats, fmaps = [], [], []
    for m in range(M):
        if d.attn:
            p, f, fm = AO.random_problem(d.B, d.V, d.E, d.H, d.C, d.P, d.A, seed=10 * s + m, scale=ATTN_SCALE)
            p[6] = p[6].clone()
            p[6][EOS] += bias
            fmaps.append(fm)
        else:
            p = BO.random_params(d.V, d.E, d.H, d.NL, seed=10 * s + m, scale=LSTM_SCALE)
            p[-1] = p[-1].clone()
            p[-1][EOS] += bias
            f = torch.randn(d.B, d.E, generator=torch.Generator().manual_seed(10 * s + m + 5)) * 0.5
        members.append(p)
        feats.append(f)
    noise = None
    if "sample" in h.kind:
        if h.philox:
            noise = torch.from_numpy(PR.sample_us(s, d.L, d.B * K, d.V))          # what the device draws from Philox(seed = s)
        else:
            noise = torch.rand(d.L, d.B * K, d.V, generator=torch.Generator().manual_seed(s + 7))
    return Problem(members, feats, fmaps or None, noise, s, force_words(d) if h.kind == "forced" else None)


def logit_mag(members) -> float:
    """|logit| <= sum |linear.weight row| + |bias| (|h| <= 1), the largest over the members (tests/test_gpu_ensemble.py)."""
    return float(max((p[5] if len(p) == 11 else p[-2]).abs().sum(1).max() + (p[6] if len(p) == 11 else p[-1]).abs().max() for p in members))


def ensemble_atol(case: Case, members) -> float:
    """tests/test_gpu_ensemble.py's score tolerance: 1e-6 plus, per token, the mix kernel's derived bound."""
    d, _ = MODELS[case.model]
    return 1e-6 + d.L * EC.bound_upper(M_ENS, d.V, logit_mag(members), HEADS[case.head].mode, 1.0 / M_ENS)


def _oracle(case: Case, seed: int):
    d, K = MODELS[case.model]
    h = HEADS[case.head]
    pb = problem(case, seed=seed)
    p, f = pb.members[0], pb.feats[0]
    fm = pb.fmaps[0] if d.attn else None
    if h.kind == "beam":
        if h.cons is not C_OFF:
            return (CO.attn_beam_search(p, f, fm, K, d.L, h.groups, h.diversity, length_penalty=h.lp, **h.cons) if d.attn else
                    CO.beam_search(p, f, K, d.L, h.groups, h.diversity, length_penalty=h.lp, **h.cons))
        if h.groups > 1:
            return (DO.attn_diverse_beam_search(p, f, fm, K, h.groups, h.diversity, d.L, length_penalty=h.lp) if d.attn else
                    DO.diverse_beam_search(p, f, K, h.groups, h.diversity, d.L, length_penalty=h.lp))
        return AO.beam_search(p, f, fm, K, d.L, length_penalty=h.lp) if d.attn else BO.beam_search(p, f, K, d.L, length_penalty=h.lp)
    if h.kind == "forced":
        kg = K >> 2
        if d.attn:
            ids, sc, ln, al, met, margins = FO.attn_beam_search(p, f, fm, pb.force, kg, d.L, length_penalty=h.lp, **h.cons)
            return ids, sc, ln, met, margins, al
        return FO.beam_search(p, f, pb.force, kg, d.L, length_penalty=h.lp, **h.cons)
    if h.kind == "sample":
        if d.attn:
            return CO.attn_sample(p, f, fm, K, d.L, pb.noise_u, h.top_k, h.top_p, 1.0, **h.cons)
        if h.cons is not C_OFF:
            return CO.sample(p, f, K, d.L, pb.noise_u, h.top_k, h.top_p, 1.0, **h.cons)
        return SO.decode(p, f, K, d.L, pb.noise_u, h.top_k, h.top_p, 1.0)
    if h.kind == "ens-beam":
        return (EO.attn_beam_search(pb.members, pb.feats, pb.fmaps, K, d.L, None, h.mode) if d.attn else
                EO.beam_search(pb.members, pb.feats, K, d.L, None, h.mode))
    return (EO.attn_sample(pb.members, pb.feats, pb.fmaps, K, d.L, pb.noise_u, None, h.mode, h.top_k, h.top_p) if d.attn else
            EO.sample(pb.members, pb.feats, K, d.L, pb.noise_u, None, h.mode, h.top_k, h.top_p))


@functools.lru_cache(maxsize=None)
def oracle(case: Case):
    """The float64 oracle's outputs for the case, computed once and shared (callers leave them unchanged)."""
    return _oracle(case, seed_of(case))


def margins_of(case: Case, want):
    """(the smallest selection or draw margin, its threshold) of an oracle result."""
    kind = HEADS[case.head].kind
    if "sample" in kind:
        return float(want[3].min()), 1e-5
    margins = want[4] if kind == "forced" else want[-1]
    return min(sel for sel, _ in margins), 1e-4


def lengths_of(want):
    return want[2]


def decided(case: Case, want) -> str:
    """"" if the oracle decides every image (row) of the case and the search ends as the termination says, else what is wrong."""
    d, _ = MODELS[case.model]
    m, thr = margins_of(case, want)
    if not (m > thr if thr == 1e-5 else m >= thr):
        return f"smallest margin {m:.3g} under {thr:g}"
    ln = lengths_of(want)
    live = ln[ln > 0]
    if case.term == "ends" and not (int(live.max()) <= 3 and int(live.max()) < d.L):
        return f"the <E> bias should end every caption within 3 steps: lengths {ln.tolist()}"
    if case.term == "runs" and not bool((live == d.L).all()):
        return f"the <E> bias should keep every caption running to L: lengths {ln.tolist()}"
    return ""
