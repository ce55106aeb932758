"""Pairwise CIDEr-D on the MI355X.  HIP events, median of >= 50 timed launches after warm-up, the two arms
alternating; one JSON line per case.

  pairwise   gic_cider_pairwise over B = 64 images x K captions (K = 8 and K = 32), L = 20, V = 10 000 (Zipf-like captions, as
             tools/overlap_bench.py; an image's captions share a base sentence): the K x K matrix, the row consensus and the Self-CIDEr
             in one launch
  baseline   the only alternative without the kernel: gic_cider_d with each image's K captions as their own references -- the row
             means, self-match included, and nothing else
The row means of the two are compared (they agree to the CIDEr-D tolerance), and the consensus and Self-CIDEr are checked against the
float64 oracle (tests/cider_pair_oracle.py) on the first images.

python tools/cider_pair_bench.py [--runs 50] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_image_captioning_amd.cider import CiderD, RefBatch  # noqa: E402

B, L, V = 64, 20, 10000
CHECKED = 4                                                      # images compared with the oracle


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _zipf_caption(rng, weights, lo=8, hi=18):
    return rng.choices(range(4, V), cum_weights=weights, k=rng.randrange(lo, hi + 1))


def _candidates(rng, weights, K):
    """K captions of one image: a base sentence with a third of its words re-drawn, cut to L - 1 ids, then <E>."""
    base = _zipf_caption(rng, weights)
    return [[t if rng.random() > 0.33 else rng.choices(range(4, V), cum_weights=weights)[0] for t in base][:L - 1] + [2] for _ in range(K)]


def bench(K, runs, dev, emit, scorer, df, n_images, rng, weights):
    from tests import cider_pair_oracle as PO
    cands = [_candidates(rng, weights, K) for _ in range(B)]
    ids = torch.zeros(B, K, L, dtype=torch.int64)
    lens = torch.zeros(B, K, dtype=torch.int32)
    for b, cs in enumerate(cands):
        for k, c in enumerate(cs):
            ids[b, k, :len(c)] = torch.tensor(c)
            lens[b, k] = len(c)
    ids, lens = ids.to(dev), lens.to(dev)
    refs = RefBatch.pack(cands).to(dev)
    pair = lambda: scorer.pairwise(ids, lens)                    # noqa: E731
    base = lambda: scorer.score(ids, lens, refs)                 # noqa: E731
    for _ in range(5):
        pair()
        base()
    torch.cuda.synchronize()
    t_pair, t_base = [], []
    for _ in range(runs):
        t_pair.append(event_us(pair))
        t_base.append(event_us(base))
    out, means = pair(), base()
    err_mean = float((out["matrix"].mean(2) - means).abs().max())
    err_c = err_s = 0.0
    for b in range(CHECKED):
        M = PO.pair_matrix(cands[b], df, n_images)
        err_c = max(err_c, float(np.abs(out["consensus"][b].cpu().double().numpy() - PO.consensus(M)).max()))
        err_s = max(err_s, abs(float(out["self_cider"][b]) - PO.self_cider(M)))
    assert err_mean <= 1e-4 and err_c <= 1e-4 and err_s <= PO.TOL_SELF_CIDER, (err_mean, err_c, err_s)
    p, d = statistics.median(t_pair), statistics.median(t_base)
    q = lambda ts: [round(v, 2) for v in statistics.quantiles(ts, n=4)]       # noqa: E731
    emit({"case": "gic_cider_pairwise", "images": B, "K": K, "L": L, "V": V, "table_keys": int(scorer.keys.numel()),
          "pairwise_us": round(p, 2), "cider_d_self_refs_us": round(d, 2), "baseline_over_pairwise": round(d / p, 2),
          "quartiles_us_pairwise": q(t_pair), "quartiles_us_baseline": q(t_base), "max_abs_err_row_mean_vs_cider_d": err_mean,
          "max_abs_err_consensus": err_c, "max_abs_err_self_cider": err_s, "mean_self_cider": float(out["self_cider"].mean()),
          "mean_consensus": float(out["consensus"].mean())})


def main():
    from tests import cider_oracle as CO
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    rng = random.Random(0)
    weights = list(np.cumsum([1.0 / (i + 1) for i in range(V - 4)]))      # cumulative Zipf-like word frequencies: n-grams recur as in captions
    corpus = [[_zipf_caption(rng, weights) for _ in range(5)] for _ in range(2000)]
    scorer = CiderD(corpus, V, dev)
    df, n_images = CO.document_frequency(corpus)
    for K in (8, 32):
        bench(K, max(50, a.runs), dev, emit, scorer, df, n_images, rng, weights)


if __name__ == "__main__":
    main()
