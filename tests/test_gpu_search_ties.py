"""The search kernels (beam_tile_topk, vocab_step's beam epilogue, beam_select plain / diverse / with ban lists, beam_finalize,
attn_beam_alphas) at exact ties, bit for bit against tests/tie_search_oracle.py.

With an all-zero w_out the vocabulary product is 0 and the logits are b_out exactly, in f32 and in bf16, on the generic and on the
fused path (the accumulator is 0 and the bias is added in f32); the first assertion of every test checks that premise through the
teacher-forced logits of forward_tf.  Over the dyadic tables of tie_search_oracle.tables a search is then decided by the three tie
rules alone -- beam_better (equal logits to the lower id: within a lane's 8 entries, across the 8 lanes of a tile, across tiles and
across the two tiles one lane of beam_select merges at V = 4100), sel_better (equal keys to the lower lane = parent * K + rank, within
each diverse group too) and beam_finalize (equal normalised scores to the lower beam index) -- and ids, lengths and the float32 bits of
the scores must be the oracle's.  Every result must also be the same for every image of the batch, in f32 and in bf16, and in a second
call.  The attention maps are checked with the sum-to-one / zero-past-length helper of tests/test_gpu_attn_beam.py.

Paths: the generic LSTM path at V = 50 (NL = 2) and at V = 4100 (the fused kernels take that shape, so the batch is 512 // K + 1 images:
more rows than they admit); the fused LSTM path at V = 68 and 4100; the attention decoder (V = 64).  K in {1, 2, 3, 5, 8} x alpha in
{0, 1}, diverse (K, G) in {(4, 2), (6, 3), (8, 8)}, the constrained entry points with a no-repeat bigram, min_length 3 and a suppressed
id tied for the top; L = 6; B = 3, and B = 9 at K = 8 (72 rows: a second 64-row block of beam_tile_topk).

The one number taken from the device is lse = logsumexp(table): expf / logf cannot be emulated.  Every table has maximum 0, so a
one-step search with the same K returns score[:, 0] = -lse exactly; it is read there, must be the same in every row, in f32 and bf16,
and is checked against float64 within tie_search_oracle.lse_bound, which is derived from operation counts (61 u, 67 u at V = 4100,
plus 6 u |lse|; u = 2^-24) and not fitted.  Largest |lse - lse64| / bound measured on an MI355X, per path:
    generic50 0.074   generic4100 0.074   fused68 0.095   fused4100 0.074   attn 0.042
(the largest over the six tables and every K; every test prints its own as "lse err/bound").

That each rule is pinned is shown without a GPU: tests/test_tie_search_oracle.py reverses each in the oracle and finds runs that change.

alpha = 1: powf and the division are not emulated, so the order is asserted where two beams are a true tie (equal score and equal
length) or their normalised scores differ by more than 4 ulp; other neighbours, and the true ties that adjoin them, are compared as
a set (tie_search_oracle.search's clusters)."""
import numpy as np
import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import beam_oracle as BO
from tests import tie_search_oracle as TO
from tests.test_gpu_attn_beam import _check_alphas

pytestmark = pytest.mark.gpu

ATTN_DIMS = (64, 16, 32, 40, 49, 24)                       # V, E, H, C, P, A: tests/test_gpu_attn_beam.py's ORACLE_SHAPE
# path -> (decoder, V, NL, fused)
PATHS = {"generic50": ("lstm", 50, 2, False), "generic4100": ("lstm", 4100, 1, False), "fused68": ("lstm", 68, 1, True),
         "fused4100": ("lstm", 4100, 1, True), "attn": ("attn", 64, 1, True)}
E, H = 8, 16
TABLES = ("all_equal", "seam8", "eos_top", "eos_tied", "two_level", "tile_seam")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _batches(path, K):
    if path == "generic4100":
        return (512 // K + 1,)                             # B * K > 512 rows: beyond what the fused step kernels admit
    return (3, 9) if K == 8 else (3,)


class _Path:
    """One path's engines (f32, bf16) and, per table, its parameters on the device (kept alive: the engines cache by address)."""

    def __init__(self, path, dev):
        from gan_image_captioning_amd import engine
        self.path, self.dev = path, dev
        self.kind, self.V, self.NL, self.fused = PATHS[path]
        if self.kind == "lstm":
            self.eng = [engine.DecoderEngine(self.V, E, H, self.NL, dt) for dt in (0, 1)]
            self.base = BO.random_params(self.V, E, H, self.NL, seed=self.V, scale=2.0)
            self.wout, self.bout = len(self.base) - 2, len(self.base) - 1
            self.E = E
        else:
            self.eng = [engine.AttnDecoderEngine(*ATTN_DIMS, dt) for dt in (0, 1)]
            self.base, _, self.fmap_cpu = AO.random_problem(16, *ATTN_DIMS, seed=3, scale=2.0)
            self.wout, self.bout = 5, 6
            self.E = ATTN_DIMS[1]
        self.params, self.inputs = {}, {}

    def table_params(self, name, table):
        if name not in self.params:
            p = [t.clone() for t in self.base]
            p[self.wout] = torch.zeros_like(p[self.wout])
            p[self.bout] = torch.from_numpy(table.copy())
            self.params[name] = [t.to(self.dev) for t in p]
        return self.params[name]

    def ins(self, B):
        """(features[, fmap]) of a batch of B different images."""
        if B not in self.inputs:
            feats = torch.randn(B, self.E, generator=torch.Generator().manual_seed(B)).to(self.dev)
            if self.kind == "attn":
                fm = self.fmap_cpu[torch.arange(B) % self.fmap_cpu.shape[0]]
                self.inputs[B] = (feats, fm.contiguous().to(self.dev))
            else:
                self.inputs[B] = (feats,)
        return self.inputs[B]

    def logits_tf(self, dt, params, B, T):
        caps = torch.randint(0, self.V, (B, T - 1), generator=torch.Generator().manual_seed(1)).to(self.dev)
        out = self.eng[dt].forward_tf(params, *self.ins(B), caps, [T] * B, 1.0, pretrain=True)
        return out[0]

    def search(self, dt, params, B, K, L, groups=1, lam=0.0, alpha=0.0, no_repeat_ngram=0, min_length=0, suppress=()):
        eng = self.eng[dt]
        kw = dict(length_penalty=alpha, no_repeat_ngram=no_repeat_ngram, min_length=min_length, suppress_tokens=tuple(suppress))
        if self.kind == "attn":
            kw["want_alphas"] = True
        else:
            assert eng.beam_fused(B, K) == self.fused, (self.path, B, K)
        if groups == 1:
            return eng.beam_search(params, *self.ins(B), L, K, **kw)
        return eng.diverse_beam_search(params, *self.ins(B), L, K, groups, lam, **kw)


@pytest.fixture(scope="module")
def paths(dev):
    cache = {}

    def get(path):
        if path not in cache:
            cache[path] = _Path(path, dev)
        return cache[path]
    return get


def _np(out):
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.int64)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _beam_key(ids, sc, ln, j):
    return tuple(ids[j].tolist()), int(ln[j]), int(sc[j:j + 1].view(np.int32)[0])


def _check(out, want, what):
    """Every image of the batch holds the oracle's beams: slot by slot, or cluster by cluster as a set where alpha = 1 leaves an order
    too close to call; the float32 bits of the scores included."""
    ids, sc, ln = _np(out)
    assert (ids == ids[:1]).all() and (ln == ln[:1]).all() and (sc.view(np.int32) == sc[:1].view(np.int32)).all(), \
        f"{what}: the images of a batch differ"
    wid, wsc, wln = want["ids"], want["scores"], want["lengths"]
    for cluster in want["clusters"]:
        got = sorted(_beam_key(ids[0], sc[0], ln[0], j) for j in cluster)
        ref = sorted(_beam_key(wid, wsc, wln, j) for j in cluster)
        assert got == ref, f"{what}: slots {cluster}\n got {got}\nwant {ref}\nall got {ids[0].tolist()} {ln[0].tolist()} {sc[0].tolist()}" \
                           f"\nall want {wid.tolist()} {wln.tolist()} {wsc.tolist()}"


def _device_lse(P, params, K, table, what):
    """lse as the device computes it, read from a one-step search with the same K (score[:, 0] = 0 + (0 - lse)); the same in every row
    and in both dtypes; within the derived bound of float64.  Returns (lse f32, err / bound)."""
    vals = []
    for dt in (0, 1):
        for B in _batches(P.path, K):
            sc = P.search(dt, params, B, K, 1)[1][:, 0].cpu().numpy()
            assert (sc.view(np.int32) == sc[:1].view(np.int32)).all(), f"{what}: lse differs between the rows of a batch"
            vals.append(np.float32(-sc[0]))
    assert all(v.view(np.int32) == vals[0].view(np.int32) for v in vals), f"{what}: lse differs between f32 and bf16 or batch sizes: {vals}"
    err, bound = abs(float(vals[0]) - TO.lse64(table)), TO.lse_bound(len(table), table)
    assert err <= bound, f"{what}: |lse - lse64| = {err:.3e} > {bound:.3e}"
    return vals[0], err / bound


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("path", list(PATHS))
def test_ties_bit_for_bit(dev, paths, path, name):
    P = paths(path)
    table = TO.tables(P.V)[name]
    params = P.table_params(name, table)
    # ---- the premise: logits == b_out exactly, f32 and bf16 (the bf16 store holds the dyadic values unchanged)
    want_logits = torch.from_numpy(table)
    for dt in (0, 1):
        pred = P.logits_tf(dt, params, 3, 4)
        torch.cuda.synchronize()
        assert torch.equal(pred.float().cpu(), want_logits.expand(3, 4, -1)), f"{path}/{name}: the logits are not b_out (dtype {dt})"
    worst, lse_k = 0.0, {}
    for label, kw in TO.runs(table):
        K = kw["K"]
        what = f"{path}/{name}/{label}"
        if K not in lse_k:
            lse_k[K], ratio = _device_lse(P, params, K, table, what)
            worst = max(worst, ratio)
        want = TO.search(table, lse_k[K], **kw)
        for B in _batches(path, K):
            outs = [P.search(dt, params, B, **kw) for dt in (0, 1)]
            again = P.search(0, params, B, **kw)
            torch.cuda.synchronize()
            _check(outs[0], want, what + f"/B{B}")
            assert _same(outs[0][:3], outs[1][:3]), f"{what}: f32 and bf16 differ"
            assert _same(outs[0], again), f"{what}: two calls differ"
            if P.kind == "attn":
                for o in outs:
                    _check_alphas(o[3], o[2])
    print(f"{path}/{name}: lse err/bound {worst:.3f}")
