"""Diverse beam search against beam search of the same width, at cfg2's LSTM decoder shapes (B = 64, L = 20, V = 10000, E = H = 512,
bf16) and cfg4's attention decoder shapes (B = 32, a 7x7x2048 feature map, A = 512, otherwise as cfg2), for K in {4, 6, 8} and
G in {1, 2, K} (lambda = 0.5).  HIP events, median of >= 50 timed runs after warm-up, the two searches of a pair timed alternately so
that drift hits both; prints one JSON line per case (us, us per step, the ratio to beam search).  The weights give no early <E>, so
every search runs all L steps.  The select kernel alone is timed by a separate rocprofv3 pass over this script (--only selects the
searches to run), and --select-stats reads the trace back: the median duration of beam_select per instantiation and, for the
diverse one, per group count (the G = 2 searches of a width run before the G = K ones), as CSV lines:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/diverse_beam_bench.py --runs 20 --only lstm
    python tools/diverse_beam_bench.py --select-stats OUT/run_results.db
python tools/diverse_beam_bench.py [--runs 50] [--only lstm|attn]"""
import argparse
import collections
import json
import os
import re
import sqlite3
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H, C, P, A = 64, 20, 10000, 512, 512, 2048, 49, 512
BA = 32
LAM = 0.5


def events_us(fns, runs, warm=5):
    """Median HIP-event time of each callable, the callables timed in turn within every run."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def _ws(eng, nb, k, dev):
    n = eng.beam_ws_bytes(nb, L, k)
    ws = torch.empty(n + 256, device=dev, dtype=torch.uint8)
    off = (-ws.data_ptr()) % 256
    return ws[off:off + n]


def run(which, beam, dbs, runs):
    for k in (4, 6, 8):
        for G in sorted({1, 2, k}):
            tb, td = events_us([lambda: beam(k), lambda: dbs(k, G)], runs)
            print(json.dumps({"decoder": which, "K": k, "G": G, "diversity": LAM, "beam_us": round(tb, 1), "dbs_us": round(td, 1),
                              "dbs_us_per_step": round(td / L, 2), "dbs_vs_beam": round(td / tb, 3)}), flush=True)


def select_stats(db):
    """CSV lines (K, G, dispatches, median us) of beam_select from a rocprofv3 database of one --only run (G = 1: the plain
    instantiation, which beam search and the G = 1 searches share)."""
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    by = collections.defaultdict(list)
    for name, t0, t1 in rows:
        m = re.search(r"beam_select_kernel<(\d+), (true|false)>", name)
        if m:
            by[(int(m.group(1)), m.group(2) == "true")].append((t1 - t0) / 1e3)
    print("K,G,dispatches,median_us")
    for (k, diverse), ts in sorted(by.items()):
        parts = [(2, ts[:len(ts) // 2]), (k, ts[len(ts) // 2:])] if diverse else [(1, ts)]
        for G, t in parts:
            print(f"{k},{G},{len(t)},{statistics.median(t):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--only", choices=["lstm", "attn"], default=None)
    ap.add_argument("--select-stats", default=None, help="a rocprofv3 database of this tool: print beam_select's durations and exit")
    a = ap.parse_args()
    if a.select_stats:
        return select_stats(a.select_stats)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    if a.only in (None, "lstm"):
        eng = E.DecoderEngine(V, Em, H, 1, 1)
        prm = [p.to(dev) for p in (u(V, Em), u(4 * H, Em), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V))]
        feats = torch.randn(B, Em, device=dev) * 0.3
        ws = {k: _ws(eng, B, k, dev) for k in (4, 6, 8)}
        run("lstm", lambda k: eng.beam_search(prm, feats, L, k, ws=ws[k]),
            lambda k, G: eng.diverse_beam_search(prm, feats, L, k, G, LAM, ws=ws[k]), a.runs)
    if a.only in (None, "attn"):
        aeng = E.AttnDecoderEngine(V, Em, H, C, P, A, 1)
        prm = [p.to(dev) for p in (u(V, Em), u(4 * H, Em + C), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H),
                                   torch.zeros(V), u(A, C), torch.zeros(A), u(A, H), u(A))]
        gi = torch.Generator().manual_seed(BA)
        feats = (torch.randn(BA, Em, generator=gi) * 0.3).to(dev)
        fmap = torch.relu(torch.randn(BA, P, C, generator=gi)).to(dev).to(torch.bfloat16)
        ws = {k: _ws(aeng, BA, k, dev) for k in (4, 6, 8)}
        run("attn", lambda k: aeng.beam_search(prm, feats, fmap, L, k, ws=ws[k]),
            lambda k, G: aeng.diverse_beam_search(prm, feats, fmap, L, k, G, LAM, ws=ws[k]), a.runs)


if __name__ == "__main__":
    main()
