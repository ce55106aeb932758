"""Lexically constrained beam search (gic_decoder_forced_beam_search) at the cfg2 decoder shape (B = 64, L = 20, V = 10000,
E = H = 512, bf16): forced search for (C, K) = (1, 8), (2, 8), (3, 8) with D = 2 ids per constraint set, beside plain beam search K = 8
and diverse beam search K = 8 in G = 4 groups in the same session.  The weights give no early <E>, so every decode runs all L steps.
HIP events, median of >= 50 timed runs after warm-up; prints one JSON line per case (us per search and per step; the forced cases
also their ratio to plain beam search and the per-step difference, the cost of the hop bookkeeping and the per-state selection).
``--baseline-only`` times only plain and diverse beam search (the form that also runs on a tree without the feature).
``--tag key=value`` (repeatable) puts the pair in front of every line: profiles/forced_beam_bench.jsonl carries ``tree``, ``tool`` and
``run`` so that runs of two checkouts, alternating in one session, stay apart in one file.
python tools/forced_beam_bench.py [--runs 50] [--baseline-only] [--tag tree=this --tag tool=forced_beam_bench --tag run=1]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H, K, D = 64, 20, 10000, 512, 512, 8, 2


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
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--tag", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    tags = {}
    for kv in a.tag:
        k, _, v = kv.partition("=")
        tags[k] = int(v) if v.lstrip("-").isdigit() else v
    emit = lambda d: print(json.dumps({**tags, **d}), flush=True)   # noqa: E731
    runs = max(a.runs, 50)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    eng = E.DecoderEngine(V, Em, H, 1, 1)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    P = [u(V, Em), u(4 * H, Em), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V)]
    P = [p.to(dev) for p in P]
    feats = torch.randn(B, Em, device=dev) * 0.3
    w8 = ws_of(eng.beam_ws_bytes(B, L, K), dev)
    plain = median_us(lambda: eng.beam_search(P, feats, L, K, ws=w8), runs)
    emit({"case": "beam8", "rows": B * K, "us": round(plain, 1), "us_per_step": round(plain / L, 2)})
    div = median_us(lambda: eng.diverse_beam_search(P, feats, L, K, 4, 0.5, ws=w8), runs)
    emit({"case": "diverse8_g4", "rows": B * K, "us": round(div, 1), "us_per_step": round(div / L, 2)})
    if a.baseline_only:
        return
    wf = ws_of(eng.forced_beam_ws_bytes(B, L, K), dev)
    for Cn in (1, 2, 3):
        force = (torch.randperm(V - 5, generator=g)[:B * Cn * D] + 5).to(torch.int32).reshape(B, Cn, D).to(dev)
        t = median_us(lambda: eng.beam_search(P, feats, L, K, ws=wf, force_words=force), runs)
        out = eng.beam_search(P, feats, L, K, ws=wf, force_words=force)
        torch.cuda.synchronize()
        assert bool((out[3][:, 0] == (1 << Cn) - 1).all()) and int(out[2][:, 0].min()) == L
        emit({"case": f"forced_C{Cn}_K{K}", "rows": B * K, "D": D, "us": round(t, 1), "us_per_step": round(t / L, 2),
              "ratio_to_beam8": round(t / plain, 3), "extra_us_per_step": round((t - plain) / L, 2)})


if __name__ == "__main__":
    main()
