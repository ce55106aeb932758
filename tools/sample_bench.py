"""Caption sampling (gic_decoder_sample_captions / gic_attn_sample_captions) at the cfg2 LSTM decoder shape (B = 64 images, L = 20,
V = 10000, E = H = 512, bf16) and cfg4's per-GPU attention shape (B = 32, C = 2048, P = 49, A = 512), for n in {1, 5, 8} samples per
image, each with top-k / top-p off, top_k = 50 and top_p = 0.9.  Next to them: the ids-only greedy roll-out over the same B * n rows and
beam search with k = n.  The weights give no early <E>, so every decode runs all L steps.  HIP events, median of >= 50 timed runs after
warm-up; prints one JSON line per case (us, us per step, ratio to the rows-matched roll-out step).  ``--only-select`` times the
selection kernel alone (gic_sample_logits over B * n rows of V logits) and reports its bytes per step: B*n*V*4 read, plus the same
written by the vocabulary product before it.
python tools/sample_bench.py [--runs 50] [--which lstm,attn,select]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

L, V, Em, H = 20, 10000, 512, 512
B_LSTM, B_ATTN, C, P, A = 64, 32, 2048, 49, 512
OPTS = (("off", 0, 1.0), ("k50", 50, 1.0), ("p09", 0, 0.9))


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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def lstm(runs, dev):
    g = torch.Generator().manual_seed(0)
    eng = E.DecoderEngine(V, Em, H, 1, 1)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    prm = [u(V, Em), u(4 * H, Em), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V)]
    prm = [p.to(dev) for p in prm]
    for n in (1, 5, 8):
        R = B_LSTM * n
        feats = torch.randn(B_LSTM, Em, device=dev) * 0.3
        rfeats = torch.randn(R, Em, device=dev) * 0.3
        st = eng.alloc_rollout_state(R, L, dev)
        ids = torch.empty(R, L, device=dev, dtype=torch.int64)
        greedy = median_us(lambda: eng.sample_fwd(prm, rfeats, L, 1.0, pretrain=True, state=st, ids=ids, ids_only=True), runs)
        emit(decoder="lstm", case=f"greedy_rows{R}", rows=R, us=round(greedy, 1), us_per_step=round(greedy / L, 2))
        w = ws_of(eng.beam_ws_bytes(B_LSTM, L, n), dev)
        t = median_us(lambda: eng.beam_search(prm, feats, L, n, ws=w), runs)
        emit(decoder="lstm", case=f"beam{n}", rows=R, us=round(t, 1), us_per_step=round(t / L, 2), vs_greedy_rows=round(t / greedy, 3))
        w = ws_of(eng.sample_ws_bytes(B_LSTM, L, n), dev)
        for name, k, p in OPTS:
            t = median_us(lambda: eng.sample_captions(prm, feats, L, n, top_k=k, top_p=p, seed=1, ws=w), runs)
            emit(decoder="lstm", case=f"sample{n}_{name}", rows=R, fused=eng.beam_fused(B_LSTM, n), us=round(t, 1), us_per_step=round(t / L, 2),
                 vs_greedy_rows=round(t / greedy, 3))


def attn(runs, dev):
    g = torch.Generator().manual_seed(0)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g)   # noqa: E731
    eng = E.AttnDecoderEngine(V, Em, H, C, P, A, 1)
    prm = [u(V, Em), u(4 * H, Em + C), u(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H), u(V, H), torch.zeros(V),
           u(A, C), torch.zeros(A), u(A, H), u(A)]
    prm = [p.to(dev) for p in prm]

    def inputs(nb):
        gi = torch.Generator().manual_seed(nb)
        return (torch.randn(nb, Em, generator=gi) * 0.3).to(dev), torch.relu(torch.randn(nb, P, C, generator=gi)).to(dev).to(torch.bfloat16)

    feats, fmap = inputs(B_ATTN)
    for n in (1, 5, 8):
        R = B_ATTN * n
        rf, rm = inputs(R)
        st = eng.alloc_state(R, L, dev)
        out = torch.empty(R, L, V, device=dev, dtype=torch.bfloat16)
        ids = torch.empty(R, L, device=dev, dtype=torch.int64)
        greedy = median_us(lambda: eng.sample_fwd(prm, rf, rm, L, 1.0, pretrain=True, state=st, out=out, ids=ids), runs)
        emit(decoder="attn", case=f"greedy_rows{R}", rows=R, us=round(greedy, 1), us_per_step=round(greedy / L, 2))
        w = ws_of(eng.beam_ws_bytes(B_ATTN, L, n), dev)
        t = median_us(lambda: eng.beam_search(prm, feats, fmap, L, n, ws=w), runs)
        emit(decoder="attn", case=f"beam{n}", rows=R, us=round(t, 1), us_per_step=round(t / L, 2), vs_greedy_rows=round(t / greedy, 3))
        w = ws_of(eng.sample_ws_bytes(B_ATTN, L, n), dev)
        for name, k, p in OPTS:
            t = median_us(lambda: eng.sample_captions(prm, feats, fmap, L, n, top_k=k, top_p=p, seed=1, ws=w), runs)
            emit(decoder="attn", case=f"sample{n}_{name}", rows=R, us=round(t, 1), us_per_step=round(t / L, 2),
                 vs_greedy_rows=round(t / greedy, 3))


def select(runs, dev):
    for n in (1, 5, 8):
        R = B_LSTM * n
        logits = torch.randn(R, V, device=dev) * 3.0
        for name, k, p in OPTS:
            t = median_us(lambda: E.sample_logits(logits, k, p, 1.0, seed=1), runs)
            rd = R * V * 4
            emit(decoder="select", case=f"select_rows{R}_{name}", rows=R, us=round(t, 2), read_bytes=rd, vocab_write_bytes=rd,
                 floor_us_6p3TBs=round(rd / 6.3e12 * 1e6, 2), vs_floor=round(t / (rd / 6.3e12 * 1e6), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--which", default="lstm,attn,select")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    which = a.which.split(",")
    if "select" in which:
        select(max(a.runs, 50), dev)
    if "lstm" in which:
        lstm(max(a.runs, 50), dev)
    if "attn" in which:
        attn(max(a.runs, 50), dev)


if __name__ == "__main__":
    main()
