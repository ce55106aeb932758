"""Constrained decode (gic_*_constrained_beam_search / gic_decoder_constrained_sample_captions) at the cfg2 decoder shape (B = 64,
L = 20, V = 10000, E = H = 512, bf16): beam k in {1, 3, 5}, diverse beam k = 6 in G = 3 groups, sampling n = 5 (top-k / top-p off and
top_k = 50), each unconstrained and with no_repeat_ngram = 2, min_length = 5 and three suppressed ids.  The weights give no early <E>,
so every decode runs all L steps.  HIP events, median of >= 50 timed runs after warm-up; prints one JSON line per case (us per search
and per step, and the constrained case's ratio to the unconstrained one).  The unconstrained lines are the cases of tools/beam_bench.py,
tools/diverse_beam_bench.py and tools/sample_bench.py at the same shapes.
``--unconstrained-only`` times only the unconstrained halves (the form that also runs on a tree without the feature).
python tools/constrained_decode_bench.py [--runs 50] [--unconstrained-only]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H = 64, 20, 10000, 512, 512
CONS = dict(no_repeat_ngram=2, min_length=5, suppress_tokens=(1, 3, 4))


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


def ws_of(n, dev):
    ws = torch.empty(n + 256, device=dev, dtype=torch.uint8)
    off = (-ws.data_ptr()) % 256
    return ws[off:off + n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--unconstrained-only", action="store_true")
    a = ap.parse_args()
    runs = max(a.runs, 50)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    eng = E.DecoderEngine(V, Em, H, 1, 1)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    P = [u(V, Em), u(4 * H, Em), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V)]
    P = [p.to(dev) for p in P]
    feats = torch.randn(B, Em, device=dev) * 0.3
    cases = []
    for k in (1, 3, 5):
        w = ws_of(eng.beam_ws_bytes(B, L, k), dev)
        cases.append((f"beam{k}", k, lambda kw, k=k, w=w: eng.beam_search(P, feats, L, k, ws=w, **kw)))
    w6 = ws_of(eng.beam_ws_bytes(B, L, 6), dev)
    cases.append(("diverse6_g3", 6, lambda kw: eng.diverse_beam_search(P, feats, L, 6, 3, 0.5, ws=w6, **kw)))
    ws5 = ws_of(eng.sample_ws_bytes(B, L, 5), dev)
    for name, tk in (("off", 0), ("k50", 50)):
        cases.append((f"sample5_{name}", 5, lambda kw, tk=tk: eng.sample_captions(P, feats, L, 5, top_k=tk, seed=1, ws=ws5, **kw)))
    for name, k, fn in cases:
        free = median_us(lambda: fn({}), runs)
        if a.unconstrained_only:
            print(json.dumps({"case": name, "rows": B * k, "us": round(free, 1), "us_per_step": round(free / L, 2)}), flush=True)
            continue
        held = median_us(lambda: fn(CONS), runs)
        out = fn(CONS)
        torch.cuda.synchronize()
        assert int(out[2].min()) >= CONS["min_length"]
        print(json.dumps({"case": name, "rows": B * k, "us": round(free, 1), "us_per_step": round(free / L, 2), "constrained_us": round(held, 1),
                          "constrained_us_per_step": round(held / L, 2), "ratio": round(held / free, 3)}), flush=True)


if __name__ == "__main__":
    main()
