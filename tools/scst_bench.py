"""CIDEr-D scoring and one SCST step on the MI355X.  HIP events, median of >= 50 timed runs after warm-up; one
JSON line per case.

  reward     gic_cider_d at B = 64 images x (n = 5 samples + 1 greedy caption), 5 references each, L = 20, V = 10 000, df table from a
             synthetic 20 000-image training corpus; next to the float64 host oracle (tests/cider_oracle.py) on the same input
  step       one SCST step at the cfg2 decoder shape (B = 64, L = 20, V = 10 000, E = H = 512, bf16, --conditional-gan 0), split into
             sample / greedy / reward / teacher-forced forward + backward / clip + Adam (events between the phases), and the whole
             SCSTStep call, whose host syncs are counted with torch's sync debug mode

python tools/scst_bench.py [--runs 50] [--out FILE]"""
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

B, N, L, V, E, H, REFS = 64, 5, 20, 10000, 512, 512, 5


def median_us(fn, runs, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def _zipf_caption(rng, weights, lo=8, hi=18):
    return rng.choices(range(4, V), weights=weights, k=rng.randrange(lo, hi + 1))


def bench_reward(runs, dev, emit):
    from tests import cider_oracle as O
    rng = random.Random(0)
    weights = [1.0 / (i + 1) for i in range(V - 4)]             # Zipf-like word frequencies: n-grams recur as in captions
    t0 = time.perf_counter()
    train = [[_zipf_caption(rng, weights) for _ in range(REFS)] for _ in range(20000)]
    refs = train[:B]
    scorer = CiderD(train, V, dev)
    t_table = time.perf_counter() - t0
    cands = [[_zipf_caption(rng, weights, 1, L - 1) + [2] for _ in range(N + 1)] for _ in range(B)]
    ids = torch.zeros(B * (N + 1), L, dtype=torch.int64)
    lens = torch.zeros(B * (N + 1), dtype=torch.int32)
    for i, c in enumerate(x for cs in cands for x in cs):
        ids[i, :len(c)] = torch.tensor(c)
        lens[i] = len(c)
    ids, lens = ids.to(dev), lens.to(dev)
    img = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(N + 1)
    rb = RefBatch.pack(refs).to(dev)
    us = median_us(lambda: scorer.score(ids, lens, rb, cand_img=img), runs)
    got = scorer.score(ids, lens, rb, cand_img=img).cpu().double()
    df, n_img = O.document_frequency(train)
    flat = [c for cs in cands for c in cs]
    t0 = time.perf_counter()
    want = [O.cider_d(c, refs[i // (N + 1)], df, n_img) for i, c in enumerate(flat)]
    host_us = (time.perf_counter() - t0) * 1e6
    err = float((got - torch.tensor(want, dtype=torch.float64)).abs().max())
    emit({"case": "gic_cider_d", "images": B, "candidates": B * (N + 1), "refs_per_image": REFS, "L": L, "V": V, "table_keys": int(scorer.keys.numel()),
          "kernel_us": round(us, 2), "host_oracle_us": round(host_us, 1), "speedup": round(host_us / us, 1), "max_abs_err_vs_oracle": err,
          "host_table_build_s": round(t_table, 2), "mean_score": float(got.mean())})
    return scorer, refs


def bench_step(runs, dev, emit, scorer, refs):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.scst import SCSTStep, _WeightedNLLFn
    from gan_image_captioning_amd.training import GANInstructor
    torch.manual_seed(0)
    args = default_args(device="cuda", log_file=None, model_dir=None, save_dir=None, compute_dtype="bf16", vocab_size=V, gen_embed_dim=E,
                        gen_hidden_dim=H, conditional_gan=0, max_seq_len=L)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    step = SCSTStep(inst, scorer, N, "greedy")
    rb = RefBatch.pack(refs).to(dev)
    dec = inst.gen.decoder
    phases = ["sample", "greedy", "reward", "tf_fwd_bwd", "adam"]
    times = {p: [] for p in phases}

    def one(record):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
        ev[0].record()
        feats = inst._features(None, B)
        ids, _, lengths = dec.sample_captions(feats, num_samples=N, temperature=1.0, max_caption_len=L)
        ev[1].record()
        g_ids, _, g_len = dec.beam_search(feats.detach(), beam_size=1, max_caption_len=L)
        ev[2].record()
        img = torch.arange(B, device=dev, dtype=torch.int32)
        sc = scorer.score(torch.cat([ids.reshape(B * N, L), g_ids]), torch.cat([lengths.reshape(-1), g_len]), rb,
                          cand_img=torch.cat([img.repeat_interleave(N), img]))
        adv = (sc[:B * N].view(B, N) - sc[B * N:].view(B, 1)).reshape(-1, 1)
        ev[3].record()
        flat = ids.reshape(B * N, L)
        pred = dec(feats.repeat_interleave(N, 0), flat[:, :-1], lengths.reshape(-1), pretrain=True, max_length=L)[0]
        live = torch.arange(L, device=dev)[None] < lengths.reshape(-1, 1)
        w = torch.where(live, (adv * L).expand(B * N, L), torch.zeros((), device=dev)).reshape(-1).contiguous()
        step.opt.zero_grad()
        _WeightedNLLFn.apply(pred.reshape(B * N * L, V), flat.reshape(-1), w).backward()
        ev[4].record()
        step.opt.step()
        ev[5].record()
        if record:
            ev[5].synchronize()
            for i, p in enumerate(phases):
                times[p].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)

    for _ in range(5):
        one(False)
    for _ in range(runs):
        one(True)
    split = {p: round(statistics.median(times[p]), 1) for p in phases}
    total = median_us(lambda: step(None, rb, L), runs)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step(None, rb, L)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message).splitlines()[0] for w in caught
             if "synchron" in str(w.message).lower() and "prototype" not in str(w.message)]         # (not the mode's own notice)
    emit({"case": "scst_step", "B": B, "n": N, "L": L, "V": V, "E": E, "H": H, "dtype": "bf16", "baseline": "greedy", "phase_us": split,
          "phase_sum_us": round(sum(split.values()), 1), "step_us": round(total, 1),
          "reward_share_of_step": round(split["reward"] / total, 4), "host_syncs_in_step": len(syncs), "sync_messages": syncs[:3]})


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

    scorer, refs = bench_reward(max(50, a.runs), dev, emit)
    bench_step(max(50, a.runs), dev, emit, scorer, refs)


if __name__ == "__main__":
    main()
