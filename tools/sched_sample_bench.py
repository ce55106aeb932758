"""MLE pre-train step with scheduled sampling (--scheduled-sampling-prob) at the cfg2 (LSTM decoder, 64 captions) and cfg4
(visual-attention decoder, 32 captions) shapes: --pretrain-mode teacher with p = 0, 0.25 and 1, next to --pretrain-mode sample.  Every
configuration runs in a fresh child process (its own HIP context, caches and allocator); a step is timed by wall clock between device
synchronisations, median of --steps steps after --warmup.  Writes profiles/sched_sample_bench.json and prints one JSON line per
configuration.
   python tools/sched_sample_bench.py [--steps 30] [--warmup 5] [--tree DIR --label NAME]
--tree DIR: time the p = 0 teacher step and the sample step of ANOTHER checkout of this project (built) with the same driver -- the
parent commit's step, for the "p = 0 launches what the parent launches" comparison; its flags are left at that tree's defaults."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(w, mode, p) for w in ("cfg2", "cfg4") for mode, p in (("teacher", 0.0), ("teacher", 0.25), ("teacher", 1.0), ("sample", 0.0))]


def child(a):
    sys.path.insert(0, a.tree or ROOT)
    import torch
    import bench
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import synthetic_batch
    from gan_image_captioning_amd.training import GANInstructor
    c = bench.CFG2
    batch = 64 if a.workload == "cfg2" else 32
    extra = dict(decoder="attention", attn_dim=512) if a.workload == "cfg4" else {}
    if a.prob > 0.0:
        extra.update(scheduled_sampling_prob=a.prob, scheduled_sampling_pick=a.pick)
    args = default_args(vocab_size=c["V"], gen_embed_dim=c["E"], gen_hidden_dim=c["H"], gen_num_layers=c["NL"], conditional_gan=1,
                        encoder_arch="resnet50", compute_dtype="bf16", pretrain_mode=a.mode, image_size=c["S"], device="cuda",
                        log_file=None, model_dir=None, save_dir=None, **extra)
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    images, captions, _l, L = synthetic_batch(batch, c["V"], c["S"], c["L"], seed=1008, device=args.device, with_images=True)
    lengths = torch.full((batch,), L, dtype=torch.int32)

    def step():
        inst.pretrain_step(images, captions, L, train=True, next_images=images, lengths=lengths)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({"workload": a.workload, "pretrain_mode": a.mode, "p": a.prob, "pick": a.pick, "batch": batch, "L": L,
                                  "steps": a.steps, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                                  "ms_max": round(max(ms), 3), "tree": a.label}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pick", default="sample", choices=["sample", "argmax"])
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_sample_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--mode", default="teacher")
    ap.add_argument("--prob", type=float, default=0.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    if os.path.exists(a.out) and a.tree:                   # a second tree's rows join the file of the first
        with open(a.out) as f:
            rows = json.load(f)["rows"]
    for w, mode, p in CONFIGS:
        if a.tree and p > 0.0:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", w, "--mode", mode, "--prob", str(p), "--pick", a.pick,
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--label", a.label] + (["--tree", a.tree] if a.tree else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{w} {mode} p={p}: child exited with {r.returncode}")      # nothing more is started on the device
        rows.append(json.loads(line[-1][7:]))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "MLE pre-train step, ms (tools/sched_sample_bench.py)", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
