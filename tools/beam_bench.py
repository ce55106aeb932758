"""Beam-search decode at the cfg2 decoder shapes (B = 64, L = 20, V = 10000, E = H = 512, bf16) for k in {1, 3, 5, 8}, next to the
greedy ids-only roll-out (Decoder.sample's inference form).  HIP events, median of >= 50 timed runs after warm-up; prints one JSON
line per case (captions/s, us per step).  The weights give no early <E>, so every search runs all L steps.  The rows-matched cases
(k = 1 over B*k images, same rows as beam k) separate what grows with the rows from what grows with k (the top-k epilogues).
python tools/beam_bench.py [--runs 50]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H = 64, 20, 10000, 512, 512


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    eng = E.DecoderEngine(V, Em, H, 1, 1)
    P = [torch.empty(V, Em).uniform_(-0.05, 0.05, generator=g), torch.empty(4 * H, Em).uniform_(-0.05, 0.05, generator=g),
         torch.empty(4 * H, H).uniform_(-0.05, 0.05, generator=g), torch.zeros(4 * H), torch.zeros(4 * H),
         torch.empty(V, H).uniform_(-0.05, 0.05, generator=g), torch.zeros(V)]
    P = [p.to(dev) for p in P]
    feats = torch.randn(B, Em, device=dev) * 0.3
    st = eng.alloc_rollout_state(B, L, dev)
    ids = torch.empty(B, L, device=dev, dtype=torch.int64)
    greedy = median_us(lambda: eng.sample_fwd(P, feats, L, 1.0, pretrain=True, state=st, ids=ids, ids_only=True), a.runs)
    print(json.dumps({"case": "greedy", "us": round(greedy, 1), "us_per_step": round(greedy / L, 2), "captions_per_s": round(B / greedy * 1e6)}))
    for k, nb in ((1, B), (3, B), (5, B), (8, B), (1, 3 * B), (1, 5 * B), (1, 8 * B)):
        f = feats if nb == B else torch.randn(nb, Em, device=dev) * 0.3
        n = eng.beam_ws_bytes(nb, L, k)
        ws = torch.empty(n + 256, device=dev, dtype=torch.uint8)
        off = (-ws.data_ptr()) % 256
        w = ws[off:off + n]
        t = median_us(lambda: eng.beam_search(P, f, L, k, ws=w), a.runs)
        name = f"beam{k}" if nb == B else f"beam1_rows{nb}"
        print(json.dumps({"case": name, "images": nb, "rows": nb * k, "fused": eng.beam_fused(nb, k), "us": round(t, 1),
                          "us_per_step": round(t / L, 2), "captions_per_s": round(nb / t * 1e6), "vs_greedy_per_step": round(t / greedy, 3)}))


if __name__ == "__main__":
    main()
