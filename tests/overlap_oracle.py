"""CPU oracle of the n-gram overlap metrics (gicap.h gic_caption_overlap), pure Python in float64: the ten BLEU statistics of a
candidate, the coco-caption ROUGE-L (beta = 1.2) over the textbook O(L^2) LCS table, and the add-one smoothed sentence BLEU-4.  Lives
under tests/: the package never imports an oracle.

A caption's tokens are its ids with <PAD>=0, <S>=1, <E>=2 removed.  stats = [clipped_1..4, total_1..4, len_c, closest reference length]
with clipped_n = sum over the candidate's distinct n-grams of min(count_c, max_r count_r), total_n = max(len_c - n + 1, 0) and the
closest length the minimum over the references of (|len_c - len_r|, len_r).  An image without references scores all zeros."""
import math
from collections import Counter

SPECIALS = (0, 1, 2)
BETA = 1.2


def tokens(ids):
    return [int(t) for t in ids if int(t) not in SPECIALS]


def lcs(a, b):
    """Length of the longest common subsequence of two token lists: the (len(a) + 1) x (len(b) + 1) table."""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def _counts(toks, n):
    return Counter(tuple(toks[i:i + n]) for i in range(len(toks) - n + 1))


def stats(cand, refs):
    """The ten integers of one candidate id list against its image's reference id lists."""
    if not refs:
        return [0] * 10
    c = tokens(cand)
    rs = [tokens(r) for r in refs]
    clipped, total = [], []
    for n in range(1, 5):
        cc = _counts(c, n)
        rc = [_counts(r, n) for r in rs]
        clipped.append(sum(min(k, max(x[g] for x in rc)) for g, k in cc.items()))
        total.append(max(len(c) - n + 1, 0))
    closest = min(((abs(len(c) - len(r)), len(r)) for r in rs))[1]
    return clipped + total + [len(c), closest]


def rouge_l(cand, refs):
    """coco-caption Rouge.calc_score: P = max_r lcs/len_c, R = max_r lcs/len_r, (1 + b^2) P R / (R + b^2 P), 0 unless both are positive."""
    c = tokens(cand)
    rs = [tokens(r) for r in refs]
    if not rs or not c:
        return 0.0
    prec = max(lcs(r, c) / float(len(c)) for r in rs)
    rec = max((lcs(r, c) / float(len(r)) if r else 0.0) for r in rs)
    if prec == 0.0 or rec == 0.0:
        return 0.0
    return (1.0 + BETA ** 2) * prec * rec / (rec + BETA ** 2 * prec)


def sbleu(cand, refs):
    """Sentence BLEU-4 with add-one smoothing of the orders 2..4 (Lin & Och 2004; NLTK's method 2) from the candidate's own stats."""
    s = stats(cand, refs)
    clipped, total, c_len, r_len = s[0:4], s[4:8], s[8], s[9]
    if clipped[0] == 0:
        return 0.0
    log_p = math.log(clipped[0] / total[0]) + sum(math.log((clipped[n] + 1.0) / (total[n] + 1.0)) for n in range(1, 4))
    return math.exp(min(1.0 - r_len / c_len, 0.0)) * math.exp(0.25 * log_p)


def corpus_bleu(stats_sum):
    """[BLEU-1..4] from ten summed stats: the definition of corpus BLEU with uniform weights, 0.0 once an order has no clipped match."""
    clipped, total, c_len, r_len = stats_sum[0:4], stats_sum[4:8], stats_sum[8], stats_sum[9]
    out = []
    for n in range(1, 5):
        if min(clipped[:n]) == 0:
            out.append(0.0)
        else:
            out.append(math.exp(min(1.0 - r_len / c_len, 0.0)) * math.exp(sum(math.log(clipped[i] / total[i]) for i in range(n)) / n))
    return out


def score_all(cands, refs_per_cand):
    """(stats rows, ROUGE-L, sbleu) of many candidates; refs_per_cand[i] = the references of candidate i's image."""
    return ([stats(c, r) for c, r in zip(cands, refs_per_cand)], [rouge_l(c, r) for c, r in zip(cands, refs_per_cand)],
            [sbleu(c, r) for c, r in zip(cands, refs_per_cand)])
