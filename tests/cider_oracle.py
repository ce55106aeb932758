"""CPU oracle of CIDEr-D: a float64, dict-based transcription of the coco-caption CiderScorer (Vedantam et al. 2015) on token ids.
Lives under tests/: the package never imports an oracle.

A caption's tokens are its ids with <PAD>=0, <S>=1, <E>=2 removed.  df(g) = the number of images of the df corpus whose references
contain g; N = the number of those images; vec_n[g] = count(g) * (log N - log max(1, df(g))); length = the number of bigrams (the
reference implementation's ``if n == 1`` quirk); sim_n as in CiderScorer.simcompute with sigma = 6; score = 10 * mean_n(sum_r sim_n)/|R|."""
import math
from collections import defaultdict

SPECIALS = (0, 1, 2)
SIGMA = 6.0


def tokens(ids):
    return [int(t) for t in ids if int(t) not in SPECIALS]


def ngrams(toks, n_max=4):
    """precook(): counts of every n-gram, n = 1..n_max, as {tuple: count}."""
    counts = defaultdict(int)
    for k in range(1, n_max + 1):
        for i in range(len(toks) - k + 1):
            counts[tuple(toks[i:i + k])] += 1
    return counts


def document_frequency(corpus):
    """corpus: per-image lists of reference id lists -> ({ngram: df}, N)."""
    df = defaultdict(int)
    for refs in corpus:
        for g in set(g for r in refs for g in ngrams(tokens(r))):
            df[g] += 1
    return dict(df), len(corpus)


def _vec(counts, df, log_n):
    vec = [dict() for _ in range(4)]
    norm = [0.0] * 4
    length = 0
    for g, tf in counts.items():
        n = len(g) - 1
        v = float(tf) * (log_n - math.log(max(1.0, df.get(g, 0.0))))
        vec[n][g] = v
        norm[n] += v * v
        if n == 1:
            length += tf
    return vec, [math.sqrt(x) for x in norm], length


def _sim(vh, vr, nh, nr, lh, lr):
    delta = float(lh - lr)
    val = [0.0] * 4
    for n in range(4):
        for g in vh[n]:
            val[n] += min(vh[n][g], vr[n].get(g, 0.0)) * vr[n].get(g, 0.0)
        if nh[n] != 0 and nr[n] != 0:
            val[n] /= nh[n] * nr[n]
        val[n] *= math.exp(-(delta ** 2) / (2 * SIGMA ** 2))
    return val


def cider_d(cand, refs, df, n_images):
    """CIDEr-D of one candidate id list against its image's reference id lists (0 without references)."""
    if not refs:
        return 0.0
    log_n = math.log(float(n_images)) if n_images else 0.0
    vh, nh, lh = _vec(ngrams(tokens(cand)), df, log_n)
    score = [0.0] * 4
    for r in refs:
        vr, nr, lr = _vec(ngrams(tokens(r)), df, log_n)
        score = [a + b for a, b in zip(score, _sim(vh, vr, nh, nr, lh, lr))]
    return sum(score) / 4.0 / len(refs) * 10.0


def corpus_scores(cands, refs_per_cand, df_corpus):
    """Scores of many candidates; refs_per_cand[i] = the references of candidate i's image."""
    df, n = document_frequency(df_corpus)
    return [cider_d(c, r, df, n) for c, r in zip(cands, refs_per_cand)]
