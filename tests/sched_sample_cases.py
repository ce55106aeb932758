"""The scheduled-sampling cases of tests/test_sched_sample_api.py (CPU: the oracle's top-2 gap condition) and
tests/test_gpu_sched_sample.py (GPU: every case against the oracle): seeded inputs with explicit coins and uniforms, at the smallest
shapes at which gic_decoder_forward_ss / gic_attn_forward_ss can still go wrong.

Picks are discrete, so a case is only usable when the oracle's top-2 gap of the maximised quantity is >= MIN_GAP at every replaced
position (DESIGN.md section 17's bar for roll-out ids); test_sched_sample_api.py asserts it, and a seed that fails is replaced here."""
import functools

import torch

from oracle import cpu_step as O
from tests import attn_beam_oracle as AO
from tests.gpu_util import dec_param_names

MIN_GAP = 1e-3
PROBS = (0.5, 1.0)
PICKS = ("sample", "argmax")

CASES = {
    # one sampled position
    "L1": dict(kind="lstm", B=1, T=2, V=8, E=8, H=8, NL=1, lengths=[2], seed=101),
    # V % 4 != 0 (scalar tail), shapes the fused step declines, a caption that never steps
    "L2": dict(kind="lstm", B=3, T=6, V=50, E=12, H=20, NL=1, lengths=[1, 6, 4], seed=102),
    # several 64-wide vocabulary tiles, fused step admitted, two layers, Tmax < T
    "L3": dict(kind="lstm", B=5, T=7, V=1000, E=16, H=32, NL=2, lengths=[5, 3, 6, 2, 4], seed=103),
    # no sampled position at all (caps empty)
    "L4": dict(kind="lstm", B=4, T=1, V=16, E=8, H=8, NL=1, lengths=[1, 1, 1, 1], seed=104),
    # smallest attention shape
    "A1": dict(kind="attn", B=3, T=6, V=64, E=16, H=32, C=16, P=4, A=24, lengths=[6, 4, 5], seed=105),
    # the 7x7 map, several tiles, ragged lengths
    "A2": dict(kind="attn", B=5, T=7, V=1000, E=16, H=32, C=64, P=49, A=40, lengths=[4, 7, 1, 6, 3], seed=106),
}
SCALE = 6.0          # the weights' scale over their U(-0.05, 0.05) init: logits of order 1, as tests/attn_beam_oracle.random_problem


def attn_names():
    return ["decoder." + n for n in AO.NAMES]


def make(kind, B, T, V, E, H, lengths, seed, NL=1, C=0, P=0, A=0, scale=SCALE):
    """A problem as a dict: names / params (library order, f32 CPU), features, fmap (attention) or None, caps int64 [B, T-1], lengths,
    coin f32 [B, T-1], u f32 [T-1, B, V]."""
    g = torch.Generator().manual_seed(seed)
    if kind == "lstm":
        gp = O.make_gen_params(V, E, H, NL, g)
        names = dec_param_names(NL)
        params = [(gp[n] * scale).float().contiguous() for n in names]
        feats, fmap = (torch.randn(B, E, generator=g) * 0.5).float(), None
    else:
        params, feats, fmap = AO.random_problem(B, V, E, H, C, P, A, seed=seed, scale=scale)
        names = attn_names()
    caps = torch.randint(0, V, (B, T - 1), generator=g)
    coin = torch.rand(B, T - 1, generator=g)
    u = torch.rand(T - 1, B, V, generator=g)
    return dict(kind=kind, names=names, params=params, feats=feats, fmap=fmap, caps=caps, lengths=list(lengths), coin=coin, u=u,
                dims=dict(B=B, T=T, V=V, E=E, H=H, NL=NL, C=C, P=P, A=A))


@functools.lru_cache(maxsize=None)
def problem(name):
    """The problem of case ``name`` (shared: callers leave its tensors unchanged)."""
    return make(**CASES[name])


def as_f64(pr, requires_grad=False):
    """(parameter dict, features, fmap or None) of a problem as float64 leaves."""
    gp = {n: p.double().clone().requires_grad_(requires_grad) for n, p in zip(pr["names"], pr["params"])}
    feats = pr["feats"].double().clone().requires_grad_(requires_grad)
    return gp, feats, None if pr["fmap"] is None else pr["fmap"].double()


@functools.lru_cache(maxsize=None)
def reference(name, p, pick):
    """The float64 oracle of case ``name`` with its explicit coins and uniforms, with the gradients of
    loss = sum(pred * d_pred) (+ sum(alphas * d_alphas)): the dict of tests/sched_sample_oracle.scheduled plus d_pred, d_alphas and
    grads (names order, then d features).  Computed once per (case, p, pick)."""
    from tests import sched_sample_oracle as SO
    pr = problem(name)
    gp, feats, fmap = as_f64(pr, requires_grad=True)
    r = SO.scheduled(gp, feats, fmap, pr["caps"], pr["lengths"], p, pick, pr["coin"], pr["u"])
    g = torch.Generator().manual_seed(CASES[name]["seed"] + 1000)
    r["d_pred"] = torch.randn(r["pred"].shape, generator=g) * 0.1
    loss = (r["pred"] * r["d_pred"].double()).sum()
    r["d_alphas"] = None
    if r["alphas"] is not None:
        r["d_alphas"] = torch.randn(r["alphas"].shape, generator=g)
        loss = loss + (r["alphas"] * r["d_alphas"].double()).sum()
    r["grads"] = list(torch.autograd.grad(loss, [gp[n] for n in pr["names"]] + [feats], allow_unused=True))
    for k in ("pred", "h_n", "c_n", "alphas"):
        r[k] = None if r[k] is None else r[k].detach()
    return r
