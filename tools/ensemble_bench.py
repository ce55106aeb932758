"""Ensemble caption decode at the cfg2 decoder shapes (B = 64, L = 20, V = 10000, E = H = 512, bf16): beam k in {3, 5} and sampling
n = 5 through the ensemble entry points for M in {1, 2, 3, 4} members, beside the single-model beam_search / sample_captions, and the
mix kernel alone.  All cases of a head run in ONE process, interleaved round-robin (case 0, case 1, ..., case 0, ...), HIP events,
median of >= 50 timed runs after warm-up, with the 10th / 90th percentiles as the spread.  The weights give no early <E>, so every
search runs all L steps.  Prints one JSON line per case and writes them all to profiles/ensemble_bench.json.
python tools/ensemble_bench.py [--runs 50] [--mix-only | --search-only]
(--mix-only: the kernel alone at M = 2, rows = 320; --search-only: the M = 2, k = 5 beam search alone; both for a rocprofv3
--kernel-trace --stats run of their own)"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_image_captioning_amd import engine as E  # noqa: E402

B, L, V, Em, H = 64, 20, 10000, 512, 512


def interleaved_us(fns, runs, warm=5):
    """{name: sorted times in us} of the callables in ``fns`` {name: fn}, timed round-robin."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3)
    return {name: sorted(v) for name, v in ts.items()}


def stats(v):
    return {"us": round(statistics.median(v), 1), "p10": round(v[len(v) // 10], 1), "p90": round(v[(9 * len(v)) // 10], 1)}


def make_params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    P = [torch.empty(V, Em).uniform_(-0.05, 0.05, generator=g), torch.empty(4 * H, Em).uniform_(-0.05, 0.05, generator=g),
         torch.empty(4 * H, H).uniform_(-0.05, 0.05, generator=g), torch.zeros(4 * H), torch.zeros(4 * H),
         torch.empty(V, H).uniform_(-0.05, 0.05, generator=g), torch.zeros(V)]
    return [p.to(dev) for p in P]


def aligned(n, dev):
    ws = torch.empty(n + 256, device=dev, dtype=torch.uint8)
    off = (-ws.data_ptr()) % 256
    return ws[off:off + n]


def mix_cases(dev, runs, out):
    for M in (1, 2, 3, 4):
        for rows in (3 * B, 5 * B):
            x = torch.randn(M, rows, V, device=dev) * 3.0
            for mode in ("prob", "logprob"):
                t = interleaved_us({"mix": lambda: E.ensemble_mix(x, None, mode)}, runs)["mix"]
                nbytes = (2 * M + 1) * rows * V * 4                 # two reads of every member's row, one write
                rec = {"case": f"mix_M{M}_rows{rows}_{mode}", "M": M, "rows": rows, "mode": mode, **stats(t), "bytes": nbytes,
                       "gbytes_per_s": round(nbytes / statistics.median(t) / 1e3, 1)}
                print(json.dumps(rec), flush=True)
                out.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--mix-only", action="store_true")
    ap.add_argument("--search-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    if a.mix_only:
        x = torch.randn(2, 5 * B, V, device=dev) * 3.0
        for _ in range(a.runs):
            E.ensemble_mix(x, None, "prob")
        torch.cuda.synchronize()
        return
    engs = [E.DecoderEngine(V, Em, H, 1, 1) for _ in range(4)]
    params = [make_params(dev, m) for m in range(4)]
    feats = [torch.randn(B, Em, device=dev) * 0.3 for _ in range(4)]
    if a.search_only:
        w = aligned(engs[0].ensemble_beam_ws_bytes(B, L, 2, 5), dev)
        for _ in range(a.runs):
            engs[0].ensemble_beam_search(list(zip(engs[:2], params[:2])), feats[:2], None, L, 5, ws=w)
        torch.cuda.synchronize()
        return
    for head, n in (("beam", 3), ("beam", 5), ("sample", 5)):
        fns = {}
        if head == "beam":
            w1 = aligned(engs[0].beam_ws_bytes(B, L, n), dev)
            fns["single"] = lambda w1=w1: engs[0].beam_search(params[0], feats[0], L, n, ws=w1)
        else:
            w1 = aligned(engs[0].sample_ws_bytes(B, L, n), dev)
            fns["single"] = lambda w1=w1: engs[0].sample_captions(params[0], feats[0], L, n, seed=1, ws=w1)
        for M in (1, 2, 3, 4):
            mem = list(zip(engs[:M], params[:M]))
            if head == "beam":
                w = aligned(engs[0].ensemble_beam_ws_bytes(B, L, M, n), dev)
                fns[f"M{M}"] = lambda mem=mem, M=M, w=w: engs[0].ensemble_beam_search(mem, feats[:M], None, L, n, ws=w)
            else:
                w = aligned(engs[0].ensemble_sample_ws_bytes(B, L, M, n), dev)
                fns[f"M{M}"] = lambda mem=mem, M=M, w=w: engs[0].ensemble_sample_captions(mem, feats[:M], None, L, n, seed=1, ws=w)
        ts = interleaved_us(fns, a.runs)
        t1 = statistics.median(ts["M1"])
        for name, v in ts.items():
            s = stats(v)
            rec = {"case": f"{head}{n}_{name}", "head": head, "n": n, "rows": B * n, **s, "us_per_step": round(s["us"] / L, 2),
                   "captions_per_s": round(B / s["us"] * 1e6)}
            if name == "single":
                rec["M1_over_single"] = round(t1 / s["us"], 3)
            else:
                M = int(name[1:])
                rec["M"] = M
                rec["over_M_times_M1"] = round(s["us"] / (M * t1), 3)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    mix_cases(dev, a.runs, out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ensemble_bench.json"), "w") as f:
        json.dump({"shape": {"B": B, "L": L, "V": V, "E": Em, "H": H, "dtype": "bf16"}, "runs": a.runs, "cases": out}, f, indent=1)


if __name__ == "__main__":
    main()
