"""BLEU / ROUGE-L scoring on the MI355X and what a mixed reward adds to an SCST step.  HIP events, median of
>= 50 timed runs after warm-up; one JSON line per case.

  overlap    gic_caption_overlap at the SCST shape: B = 64 images x (n = 5 samples + 1 greedy caption), 5 references each, L = 20,
             V = 10 000 (Zipf-like captions, as tools/scst_bench.py); next to the host path for the same captions: the device-to-host
             copy of ids and lengths, then utils.bleu_score over the token lists (wall clock, median); the stats are checked
             against the float64 oracle (tests/overlap_oracle.py)
  step       one SCSTStep call at the cfg2 decoder shape (B = 64, L = 20, V = 10 000, E = H = 512, bf16, --conditional-gan 0, greedy
             baseline) with reward weights (1, 0, 0) -- the plain CiderD -- against (1, 0.5, 0.5) -- RewardMix, one more launch --
             on the same generator, the two arms alternating; torch's sync debug mode counts the host syncs of the mixed step

python tools/overlap_bench.py [--runs 50] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_image_captioning_amd.cider import CiderD, RefBatch  # noqa: E402
from gan_image_captioning_amd.metrics import OverlapScorer, RewardMix, corpus_bleu  # noqa: E402

B, N, L, V, E, H, REFS = 64, 5, 20, 10000, 512, 512, 5


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def median_us(fn, runs, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return statistics.median(event_us(fn) for _ in range(runs))


def _zipf_caption(rng, weights, lo=8, hi=18):
    return rng.choices(range(4, V), weights=weights, k=rng.randrange(lo, hi + 1))


def bench_overlap(runs, dev, emit):
    from gan_image_captioning_amd.utils import bleu_score
    from tests import overlap_oracle as O
    rng = random.Random(0)
    weights = [1.0 / (i + 1) for i in range(V - 4)]             # Zipf-like word frequencies: n-grams recur as in captions
    corpus = [[_zipf_caption(rng, weights) for _ in range(REFS)] for _ in range(2000)]
    refs = corpus[:B]
    cands = [[_zipf_caption(rng, weights, 1, L - 1) + [2] for _ in range(N + 1)] for _ in range(B)]
    ids = torch.zeros(B * (N + 1), L, dtype=torch.int64)
    lens = torch.zeros(B * (N + 1), dtype=torch.int32)
    for i, c in enumerate(x for cs in cands for x in cs):
        ids[i, :len(c)] = torch.tensor(c)
        lens[i] = len(c)
    ids, lens = ids.to(dev), lens.to(dev)
    img = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(N + 1)
    rb = RefBatch.pack(refs).to(dev)
    scorer = OverlapScorer(V, dev)
    us = median_us(lambda: scorer.score(ids, lens, rb, cand_img=img), runs)
    stats, rouge, sbleu = scorer.score(ids, lens, rb, cand_img=img)
    flat = [c for cs in cands for c in cs]
    per = [refs[i // (N + 1)] for i in range(len(flat))]
    want_stats, want_rouge, want_sbleu = O.score_all(flat, per)
    assert stats.cpu().tolist() == want_stats, "stats differ from the oracle"
    err_r = float((rouge.cpu().double() - torch.tensor(want_rouge, dtype=torch.float64)).abs().max())
    err_b = float((sbleu.cpu().double() - torch.tensor(want_sbleu, dtype=torch.float64)).abs().max())
    ref_words = [[O.tokens(r) for r in group] for group in per]

    def host():                                                 # what evaluate() does per batch: copy, strip, score
        h_ids, h_len = ids.cpu(), lens.cpu()
        words = [O.tokens(h_ids[i, :int(h_len[i])].tolist()) for i in range(h_ids.shape[0])]
        return bleu_score(words, ref_words)

    host()
    ts = []
    for _ in range(max(10, runs // 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bleu4 = host()
        ts.append((time.perf_counter() - t0) * 1e6)
    host_us = statistics.median(ts)
    assert abs(corpus_bleu(stats.sum(0, dtype=torch.int64))[3] - bleu4) <= 1e-12 * max(bleu4, 1e-30)
    emit({"case": "gic_caption_overlap", "images": B, "candidates": B * (N + 1), "refs_per_image": REFS, "L": L, "V": V,
          "kernel_us": round(us, 2), "host_bleu_score_us": round(host_us, 1), "host_over_kernel": round(host_us / us, 1),
          "stats_equal_oracle": True, "max_abs_err_rouge": err_r, "max_abs_err_sbleu": err_b, "corpus_bleu4": bleu4,
          "mean_rouge_l": float(rouge.mean()), "mean_sbleu": float(sbleu.mean())})
    return corpus, refs


def bench_step(runs, dev, emit, corpus, refs):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.scst import SCSTStep
    from gan_image_captioning_amd.training import GANInstructor
    torch.manual_seed(0)
    args = default_args(device="cuda", log_file=None, model_dir=None, save_dir=None, compute_dtype="bf16", vocab_size=V, gen_embed_dim=E,
                        gen_hidden_dim=H, conditional_gan=0, max_seq_len=L)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    cider = CiderD(corpus, V, dev)
    plain = SCSTStep(inst, cider, N, "greedy")
    mixed = SCSTStep(inst, RewardMix(cider, OverlapScorer(V, dev), 1.0, 0.5, 0.5), N, "greedy")
    rb = RefBatch.pack(refs).to(dev)
    for _ in range(5):
        plain(None, rb, L)
        mixed(None, rb, L)
    torch.cuda.synchronize()
    t_plain, t_mixed = [], []
    for _ in range(runs):                                       # alternating arms: the same clocks and neighbours for both
        t_plain.append(event_us(lambda: plain(None, rb, L)))
        t_mixed.append(event_us(lambda: mixed(None, rb, L)))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            mixed(None, rb, L)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message).splitlines()[0] for w in caught
             if "synchron" in str(w.message).lower() and "prototype" not in str(w.message)]         # (not the mode's own notice)
    p, m = statistics.median(t_plain), statistics.median(t_mixed)
    q = lambda ts: [round(v, 1) for v in statistics.quantiles(ts, n=4)]       # noqa: E731
    emit({"case": "scst_step_reward_mix", "B": B, "n": N, "L": L, "V": V, "E": E, "H": H, "dtype": "bf16", "baseline": "greedy",
          "step_us_weights_1_0_0": round(p, 1), "step_us_weights_1_.5_.5": round(m, 1), "delta_us": round(m - p, 1),
          "delta_share_of_step": round((m - p) / p, 4), "quartiles_us_1_0_0": q(t_plain), "quartiles_us_1_.5_.5": q(t_mixed),
          "host_syncs_in_mixed_step": len(syncs), "sync_messages": syncs[:3]})


def main():
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

    corpus, refs = bench_overlap(max(50, a.runs), dev, emit)
    bench_step(max(50, a.runs), dev, emit, corpus, refs)


if __name__ == "__main__":
    main()
