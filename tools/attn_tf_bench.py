"""Teacher-forced decode with the attention decoder (gic_attn_forward_tf / _bwd) at cfg4's per-GPU decoder shapes (B = 32, T = 20,
V = 10000, E = H = A = 512, a 7x7x2048 feature map, bf16), next to the greedy attention roll-out (sample_fwd / sample_bwd with
pretrain=True) in the same process.  HIP events, median of >= 50 timed runs after warm-up; prints one JSON line per case.
   python tools/attn_tf_bench.py [--runs 50]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_image_captioning_amd import engine as E  # noqa: E402

B, T, V, Em, H, C, P, A = 32, 20, 10000, 512, 512, 2048, 49, 512


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
    feats = (torch.randn(B, Em, generator=g) * 0.3).to(dev)
    fmap = torch.relu(torch.randn(B, P, C, generator=g)).to(dev).to(torch.bfloat16)
    caps = torch.randint(4, V, (B, T - 1), generator=g).to(dev)
    spread = torch.randint(8, T + 1, (B,), generator=g).tolist()
    spread[0] = T

    st = eng.alloc_state(B, T, dev)
    out = torch.empty(B, T, V, device=dev, dtype=torch.bfloat16)
    ids = torch.empty(B, T, device=dev, dtype=torch.int64)
    greedy = median_us(lambda: eng.sample_fwd(prm, feats, fmap, T, 1.0, pretrain=True, state=st, out=out, ids=ids), a.runs)
    d_out = torch.randn(B, T, V, generator=g).to(dev).to(torch.bfloat16) * 1e-3
    ws = eng.alloc_bwd_ws(B, T, dev)
    grads = [torch.empty_like(p) for p in prm] + [torch.empty(B, Em, device=dev)]
    greedy_bwd = median_us(lambda: eng.sample_bwd(prm, dict(st, fmap=fmap), out, ids, d_out, 1.0, True, ws=ws, grads=grads), a.runs)
    rows = [{"case": "greedy_sample_fwd", "us": greedy}, {"case": "greedy_sample_bwd", "us": greedy_bwd}]
    for name, lens in (("tf_all20", [T] * B), ("tf_spread8_20", spread)):
        fwd = median_us(lambda: eng.forward_tf(prm, feats, fmap, caps, lens, 1.0, True), a.runs)
        pred, _, _, saved = eng.forward_tf(prm, feats, fmap, caps, lens, 1.0, True, keep_state=True)
        d = torch.randn(pred.shape, generator=g).to(dev).to(torch.bfloat16) * 1e-3
        bwd = median_us(lambda: eng.forward_tf_bwd(prm, saved, pred, d, 1.0, True, ws=ws, grads=grads), a.runs)
        rows.append({"case": name + "_fwd", "us": fwd, "vs_greedy": fwd / greedy, "mean_len": sum(lens) / B})
        rows.append({"case": name + "_bwd", "us": bwd, "vs_greedy": bwd / greedy_bwd, "mean_len": sum(lens) / B})
    for r in rows:
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in r.items()}))


if __name__ == "__main__":
    main()
