"""Teacher-forced decode, forward plus backward, with and without output dropout (dropout = 0 and 0.5) at the cfg2 (LSTM decoder, 64
captions) and cfg4 (visual-attention decoder, 32 captions, 7x7x2048 map) shapes, bf16: engine.forward_tf(keep_state=True) followed by
engine.forward_tf_bwd on a fixed d_pred.  Every configuration runs in a fresh child process (its own HIP context, caches and allocator);
a call pair is timed by wall clock between device synchronisations, median of --steps after --warmup.  Writes
profiles/gen_dropout_bench.json and prints one JSON line per configuration.
   python tools/gen_dropout_bench.py [--steps 30] [--warmup 5] [--tree DIR --label NAME]
--tree DIR: time the dropout = 0 pair of ANOTHER checkout of this project (built) with the same driver -- the parent commit's decode,
for the "dropout = 0 launches what the parent launches" comparison; the keyword is not passed there."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(w, p) for w in ("cfg2", "cfg4") for p in (0.0, 0.5)]


def child(a):
    sys.path.insert(0, a.tree or ROOT)
    import torch
    import bench
    from gan_image_captioning_amd import engine
    c = bench.CFG2
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1008)
    V, E, H, T = c["V"], c["E"], c["H"], c["L"] + 1
    batch = 64 if a.workload == "cfg2" else 32

    def w(*shape):
        return ((torch.rand(*shape, generator=g) - 0.5) * 0.1).to(dev)
    if a.workload == "cfg2":
        NL = c["NL"]
        eng = engine.DecoderEngine(V, E, H, NL, engine.parse_dtype("bf16"))
        params = [w(V, E)]
        for l in range(NL):
            params += [w(4 * H, E if l == 0 else H), w(4 * H, H), w(4 * H), w(4 * H)]
        params += [w(V, H), w(V)]
        maps = ()
    else:
        C, P, A = 2048, 49, 512
        eng = engine.AttnDecoderEngine(V, E, H, C, P, A, engine.parse_dtype("bf16"))
        params = [w(V, E), w(4 * H, E + C), w(4 * H, H), w(4 * H), w(4 * H), w(V, H), w(V), w(A, C), w(A), w(A, H), w(A)]
        maps = (torch.randn(batch, P, C, generator=g).to(dev),)
    feats = torch.randn(batch, E, generator=g).to(dev)
    caps = torch.randint(0, V, (batch, T - 1), generator=g).to(dev)
    lengths = torch.randint(8, T + 1, (batch,), generator=g).tolist()
    lengths[0] = T
    d_pred = (torch.randn(batch, T, V, generator=g) * 1e-3).to(dev).to(eng.act)
    kw = {"dropout": a.dropout, "dropout_seed": 7} if a.dropout > 0.0 else {}      # dropout = 0: the call as the parent commit takes it

    def step():
        res = eng.forward_tf(params, feats, *maps, caps, lengths, 1.0, pretrain=True, keep_state=True, **kw)
        eng.forward_tf_bwd(params, res[-1], res[0], d_pred, 1.0, True)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({"workload": a.workload, "dropout": a.dropout, "batch": batch, "T": T, "steps": a.steps,
                                  "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                                  "tree": a.label}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_dropout_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--dropout", type=float, default=0.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    if os.path.exists(a.out) and a.tree:                   # a second tree's rows join the file of the first
        with open(a.out) as f:
            rows = json.load(f)["rows"]
    for wl, p in CONFIGS:
        if a.tree and p > 0.0:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", wl, "--dropout", str(p), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--label", a.label] + (["--tree", a.tree] if a.tree else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{wl} dropout={p}: child exited with {r.returncode}")      # nothing more is started on the device
        rows.append(json.loads(line[-1][7:]))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "teacher-forced decode, forward + backward, ms (tools/gen_dropout_bench.py)", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
