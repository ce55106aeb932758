"""Attention-decoder beam search at cfg4's per-GPU decoder shapes (B = 32, L = 20, V = 10000, E = H = A = 512, a 7x7x2048 feature
map, bf16) for k in {1, 3, 5, 8}, next to the greedy attention roll-out (sample_fwd(pretrain=True)).  HIP events, median of >= 50
timed runs after warm-up; prints one JSON line per case (captions/s, us per step).  The weights give no early <E>, so every search
runs all L steps.  The rows-matched cases (k = 1 over B*k images, same rows as beam k) separate what grows with the rows from what
grows with k.   python tools/attn_beam_bench.py [--runs 50]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H, C, P, A = 32, 20, 10000, 512, 512, 2048, 49, 512


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
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    eng = E.AttnDecoderEngine(V, Em, H, C, P, A, 1)
    prm = [u(V, Em), u(4 * H, Em + C), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V),
           u(A, C), torch.zeros(A), u(A, H), u(A)]
    prm = [p.to(dev) for p in prm]

    def inputs(n):
        gi = torch.Generator().manual_seed(n)
        return (torch.randn(n, Em, generator=gi) * 0.3).to(dev), torch.relu(torch.randn(n, P, C, generator=gi)).to(dev).to(torch.bfloat16)

    feats, fmap = inputs(B)
    st = eng.alloc_state(B, L, dev)
    out = torch.empty(B, L, V, device=dev, dtype=torch.bfloat16)
    ids = torch.empty(B, L, device=dev, dtype=torch.int64)
    greedy = median_us(lambda: eng.sample_fwd(prm, feats, fmap, L, 1.0, pretrain=True, state=st, out=out, ids=ids), a.runs)
    print(json.dumps({"case": "greedy", "us": round(greedy, 1), "us_per_step": round(greedy / L, 2), "captions_per_s": round(B / greedy * 1e6)}))
    for k, nb in ((1, B), (3, B), (5, B), (8, B), (1, 3 * B), (1, 5 * B), (1, 8 * B)):
        f, m = (feats, fmap) if nb == B else inputs(nb)
        n = eng.beam_ws_bytes(nb, L, k)
        ws = torch.empty(n + 256, device=dev, dtype=torch.uint8)
        off = (-ws.data_ptr()) % 256
        w = ws[off:off + n]
        t = median_us(lambda: eng.beam_search(prm, f, m, L, k, ws=w), a.runs)
        name = f"beam{k}" if nb == B else f"beam1_rows{nb}"
        print(json.dumps({"case": name, "images": nb, "rows": nb * k, "us": round(t, 1), "us_per_step": round(t / L, 2),
                          "captions_per_s": round(nb / t * 1e6), "vs_greedy_per_step": round(t / greedy, 3)}))


if __name__ == "__main__":
    main()
