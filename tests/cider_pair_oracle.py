"""CPU oracle of pairwise CIDEr-D (gic_cider_pairwise): float64, on top of tests/cider_oracle.py.  Lives under
tests/: the package never imports an oracle.

M[i, j] = cider_oracle.cider_d(c_i, [c_j], df, N): caption i as the candidate against caption j as the single reference (0..10; not
symmetric).  consensus[i] = the mean of row i without the diagonal (0 for K = 1).  S = (M + M^T) / 20.  self_cider =
clamp(-ln(lambda_max(S) / trace S) / ln K, 0, 1), 0 for K = 1 or trace S = 0 (numpy eigvalsh on the float64 S).

``lambda_ratio_f32`` restates the kernel's lambda_max iteration in float32 numpy: SQUARINGS trace-normalised squarings of S, then the
Rayleigh quotient of S at the row sums of the power.  TOL_SELF_CIDER is 4 x the largest |self_cider_f32 - self_cider_f64| that
tests/test_cider_pair_api.py measures over the GPU test's problems and the near-degenerate two-cluster spectra below; the 4 x covers the
device's different summation order."""
import math

import numpy as np

from tests import cider_oracle as CO

SQUARINGS = 16
# the measured maximum (tests/test_cider_pair_api.py::test_lambda_max_budget prints it) is 1.115e-6
TOL_SELF_CIDER = 4 * 1.115e-6

# (V, B, K, Lmax) of tests/test_gpu_cider_pair.py; the df table of FOREIGN_DF comes from a corpus the captions are not in
CASES = [(8, 4, 5, 12), (50, 6, 8, 16), (10000, 5, 32, 64), (32768, 3, 2, 64), (300, 4, 1, 20)]
FOREIGN_DF = (50, 6, 8, 16)


# ------------------------------------------------------------------------------------------------ the definitions
def pair_matrix(caps, df, n_images):
    """M float64 [K, K] of one image's captions (id lists).  Each caption's vectors are built once; the sum is cider_d's."""
    log_n = math.log(float(n_images)) if n_images else 0.0
    vecs = [CO._vec(CO.ngrams(CO.tokens(c)), df, log_n) for c in caps]
    K = len(caps)
    M = np.zeros((K, K))
    for i, (vh, nh, lh) in enumerate(vecs):
        for j, (vr, nr, lr) in enumerate(vecs):
            M[i, j] = sum(CO._sim(vh, vr, nh, nr, lh, lr)) / 4.0 / 1.0 * 10.0
    return M


def consensus(M):
    K = M.shape[0]
    return (M.sum(1) - np.diag(M)) / (K - 1) if K > 1 else np.zeros(K)


def similarity(M):
    return (M + M.T) / 20.0


def self_cider_of_ratio(ratio, K):
    return min(max(-math.log(ratio) / math.log(K), 0.0), 1.0)


def self_cider_s(S):
    """Self-CIDEr of a similarity matrix S (float64, eigvalsh)."""
    S = np.asarray(S, dtype=np.float64)
    K, tr = S.shape[0], float(np.trace(S))
    if K == 1 or not tr > 0.0:
        return 0.0
    return self_cider_of_ratio(float(np.linalg.eigvalsh(S)[-1]) / tr, K)


def self_cider(M):
    return self_cider_s(similarity(np.asarray(M, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ the kernel's iteration, in float32
def lambda_ratio_f32(S):
    """lambda_max(S) / trace(S) as the kernel forms it, in float32 (numpy's summation order, not the device's)."""
    f = np.float32
    S = np.asarray(S, dtype=f)
    tr = f(0)
    for r in range(S.shape[0]):
        tr = f(tr + S[r, r])
    X, scale = S.copy(), f(1) / tr
    for _ in range(SQUARINGS):
        X = (X @ X) * f(scale * scale)
        t = f(0)
        for r in range(S.shape[0]):
            t = f(t + X[r, r])
        scale = f(1) / t
    v = X.sum(1, dtype=f)
    w = S @ v
    return f(f(v @ w) / f(v @ v) / tr)


def self_cider_s_f32(S):
    S = np.asarray(S, dtype=np.float32)
    K = S.shape[0]
    if K == 1 or not float(np.trace(S)) > 0.0:
        return 0.0
    ratio = lambda_ratio_f32(S)
    sc = np.float32(-np.log(ratio) / np.log(np.float32(K)))
    return float(min(max(sc, np.float32(0)), np.float32(1)))


def self_cider_f32(M):
    M = np.asarray(M, dtype=np.float32)
    return self_cider_s_f32((M + M.T) / np.float32(20))


# ------------------------------------------------------------------------------------------------ the GPU test's problems
KINDS = ["base", "prefix", "dup", "subst", "repeat", "short", "specials", "empty", "full", "subst", "prefix", "random", "dup", "short"]


def problem(V, B, K, Lmax, seed=0, foreign_df=False):
    """ids int64 [B, K, Lmax], lengths int32 [B, K] and a df corpus.  Caption k of an image is of kind KINDS[k % len]: the image's base
    sentence, a prefix of it plus noise, an exact duplicate of an earlier caption, the base with substitutions, a few tokens repeated
    (counts > 1), 1-3 tokens, specials only, empty, and -- with Lmax = 64 -- one caption of exactly 64 ids.  Past each length lie ids
    that must not count.  The corpus is the captions themselves, grouped by image, plus 8 images of random captions; ``foreign_df``:
    those 8 images alone, so most n-grams are absent from the table."""
    rng = np.random.RandomState(1000 * seed + V % 997 + 31 * K)
    maxtok = Lmax - 2
    tok = lambda n: rng.randint(3, V, size=int(n)).tolist()          # noqa: E731
    ids = np.zeros((B, K, Lmax), dtype=np.int64)
    lengths = np.zeros((B, K), dtype=np.int32)
    groups = []
    for b in range(B):
        base = [V - 1] + tok(rng.randint(min(4, maxtok - 1), min(maxtok, 20)))      # the largest id opens every base sentence
        rows = []
        for k in range(K):
            kind = KINDS[k % len(KINDS)]
            wrap = True
            if kind == "base":
                t = list(base)
            elif kind == "prefix":
                p = rng.randint(2, len(base) + 1)
                t = (base[:p] + tok(rng.randint(0, 4)))[:maxtok]
            elif kind == "dup":
                row, wrap = list(rows[rng.randint(0, len(rows))]), False
            elif kind == "subst":
                t = [x if rng.rand() > 0.3 else tok(1)[0] for x in base]
            elif kind == "repeat":
                few = base[:rng.randint(1, 4)]
                t = [few[i] for i in rng.randint(0, len(few), size=min(maxtok, 9))]
            elif kind == "short":
                t = base[:rng.randint(1, 4)]
            elif kind == "specials":
                t, wrap = [], False
                row = [1, 2, 0, 1, 2, 0][:min(Lmax, 6)]
            elif kind == "empty":
                t, wrap, row = [], False, []
            elif kind == "full" and Lmax == 64:
                t, wrap = (base + [V - 1] + tok(64))[:64], False
                row = list(t)
            else:
                t = tok(rng.randint(4, maxtok + 1))
            if wrap:
                row = [1] + t + [2]
            assert len(row) <= Lmax
            ids[b, k, :len(row)] = row
            lengths[b, k] = len(row)
            if k % 2:
                ids[b, k, len(row):] = rng.randint(3, V, size=Lmax - len(row))         # ids past the length: not part of the caption
            rows.append(row)
        groups.append(rows)
    extra = np.random.RandomState(seed + 4242)
    others = [[extra.randint(3, V, size=extra.randint(4, 12)).tolist() for _ in range(3)] for _ in range(8)]
    corpus = others if foreign_df else groups + others
    return {"ids": ids, "lengths": lengths, "corpus": corpus, "V": V}


def captions(prob, b):
    return [prob["ids"][b, k, :prob["lengths"][b, k]].tolist() for k in range(prob["ids"].shape[1])]


def reference(prob):
    """(M [B, K, K], consensus [B, K], self_cider [B]) float64 of a problem."""
    df, n = CO.document_frequency(prob["corpus"])
    Ms = [pair_matrix(captions(prob, b), df, n) for b in range(prob["ids"].shape[0])]
    return np.stack(Ms), np.stack([consensus(M) for M in Ms]), np.array([self_cider(M) for M in Ms])


_REFERENCES = {}


def case_problem(case):
    """The problem of one of CASES and its reference, computed once per process and shared (read-only) by the tests."""
    if case not in _REFERENCES:
        prob = problem(*case, seed=CASES.index(case), foreign_df=case == FOREIGN_DF)
        _REFERENCES[case] = (prob, reference(prob))
    return _REFERENCES[case]


# ------------------------------------------------------------------------------------------------ near-degenerate spectra
def two_clusters(K, first, a, b, c):
    """S of two clusters (the first ``first`` captions, the rest): diagonal 1, in-cluster similarity a resp. b, cross similarity c."""
    S = np.full((K, K), float(c))
    S[:first, :first] = a
    S[first:, first:] = b
    np.fill_diagonal(S, 1.0)
    return S


def near_degenerate_spectra():
    """Two clusters whose cross similarity sweeps 0 .. 0.99 of the in-cluster one.  Equal clusters: lambda_1 = lambda_2 at 0, and the
    all-ones start is the top eigenvector.  The second cluster looser by a relative delta (or the clusters of unequal size): the start is
    not, and with the cross similarity near 0 the relative gap of the two top eigenvalues is about delta -- the sweep of delta passes
    1 / (2 * 2^SQUARINGS), where the Rayleigh quotient of a power iterate is worst."""
    fr = [0.0, 1e-5, 1e-4, 1e-3, 0.01, 0.03, 0.1, 0.2, 0.35, 0.5, 0.65, 0.8, 0.9, 0.95, 0.99]
    deltas = [0.0, 3e-6, 1e-5, 2e-5, 5e-5, 1e-4, 3e-4, 1e-3, 3e-3, 0.01, 0.1]
    out = []
    for K, first, a in ((2, 1, 0.6), (8, 4, 0.6), (32, 16, 0.6), (9, 4, 0.6), (32, 15, 0.3), (6, 3, 0.9)):
        out += [two_clusters(K, first, a, a * (1.0 - d), f * a * (1.0 - d)) for d in deltas for f in fr]
    return out


# ------------------------------------------------------------------------------------------------ consensus re-ranking
def rerank(scores, lengths, cons, weight, length_penalty=0.0):
    """(order, final in that order, the smallest gap between adjacent finals) per image: final = score / max(len, 1) ** length_penalty
    + weight * consensus, descending, ties to the lower index.  scores, lengths, cons: [B, K]."""
    scores, lengths, cons = (np.asarray(x, dtype=np.float64) for x in (scores, lengths, cons))
    final = scores / np.maximum(lengths, 1.0) ** length_penalty + weight * cons
    order = np.argsort(-final, axis=1, kind="stable")
    srt = np.take_along_axis(final, order, 1)
    gaps = (srt[:, :-1] - srt[:, 1:]).min(1) if final.shape[1] > 1 else np.full(final.shape[0], np.inf)
    return order, srt, gaps


def consensus_of(ids, lengths, df, n_images):
    """consensus float64 [B, K] of captions ids [B, K, L] with lengths [B, K]."""
    ids, lengths = np.asarray(ids), np.asarray(lengths)
    return np.stack([consensus(pair_matrix([ids[b, k, :lengths[b, k]].tolist() for k in range(ids.shape[1])], df, n_images))
                     for b in range(ids.shape[0])])


def table_corpus(V, seed=5, images=12):
    """A df corpus over the vocabulary of a tiny model: ``images`` images of 3 random captions each."""
    rng = np.random.RandomState(seed)
    return [[rng.randint(3, V, size=rng.randint(4, 10)).tolist() for _ in range(3)] for _ in range(images)]
