"""The image-conditioned discriminator on the MI355X: what --disc-cond projection costs per train step, and the two
match kernels of csrc/disc_cond.hip alone against their byte floors.

  step      the cfg2 train step as bench.py times it (B = 64, 224 x 224, L = 20, V = 10 000, E = H = 512, ResNet-50 trunk, bf16, device
            noise, trunk prefetch; wall time over --steps steps after --warmup): the flag off (twice: the run-to-run spread, and the line
            that must agree with bench.py's own figure), on at w = 0, on at w = 0.5 -- each in a fresh child process (a second instructor
            in one process measured 0.8 ms per step slower than the first, whatever its flags)
  kernels   gic_disc_match_fwd and the match backward inside gic_disc_bwd_cond at cfg2 (B = 64, R = 64, F = 900, Fp = 960, bf16), HIP
            events, median of --runs launches.  The backward kernel has no entry point of its own: its time is the difference between
            gic_disc_bwd_cond with q and with q = NULL (the same launches but this one, and the accumulate flag of one GEMM).  Floors:
            forward 7.9 MB read; backward 7.9 MB read + 15.7 MB written

python tools/disc_cond_bench.py [--steps 30] [--warmup 5] [--runs 200] [--out profiles/disc_cond_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(B=64, S=224, L=20, V=10000, E=512, H=512, NL=1)


def step_ms(cond, w, steps, warmup):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import synthetic_batch
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(vocab_size=CFG2["V"], gen_embed_dim=CFG2["E"], gen_hidden_dim=CFG2["H"], gen_num_layers=CFG2["NL"], conditional_gan=1,
                        encoder_arch="resnet50", compute_dtype="bf16", step_impl="fused", adv_train_batch_size=CFG2["B"], image_size=CFG2["S"],
                        disc_cond=cond, disc_mismatch_weight=w, device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.train()
    inst.disc.train()
    images, captions, _lengths, L = synthetic_batch(CFG2["B"], CFG2["V"], CFG2["S"], CFG2["L"], seed=1008, device=args.device, with_images=True)

    def step(k):
        losses = inst.adv_step(images, captions, L, train=True, next_images=images)
        inst.update_temperature(0 + (k + 1) / 50, args.adv_epochs)
        return losses

    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        losses = step(warmup + k)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert bool(torch.isfinite(losses).all()), "the step's losses are not finite"
    del inst
    torch.cuda.empty_cache()
    return ms


def median_us(fn, runs, warm=10):
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


def bench_kernels(runs, dev):
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    B, R, Lc, V = 64, 64, CFG2["L"], CFG2["V"]
    eng = engine.DiscEngine(V, 64, R, [3, 4, 5], [300, 300, 300], L.BF16)
    g = torch.Generator().manual_seed(0)
    shapes = [(64, V)] + [s for f in (3, 4, 5) for s in ((300, 1, f, 1), (300,))] + [(900, 900), (900,), (100, 900), (100,), (1, 100), (1,)]
    params = [(0.05 * torch.randn(*s, generator=g)).to(dev) for s in shapes]
    ids = torch.randint(0, V, (B, Lc), generator=g).to(dev)
    q = torch.randn(B, eng.F, generator=g).to(dev)
    gl = torch.randn(B * R, generator=g).to(dev)
    logits, st = eng.fwd(params, None, ids, True, None, seed=1)
    ws = eng.alloc_bwd_ws(B, Lc, dev)
    grads = [torch.zeros_like(p) for p in params]
    d_q = torch.empty(B, eng.F, device=dev)
    y_bytes = B * R * eng.Fp * 2
    fwd_bytes, bwd_bytes = y_bytes, y_bytes + B * R * eng.Fp * 4
    fwd_us = median_us(lambda: eng.match_logits(st, q, logits=logits, accumulate=True), runs)
    with_q = median_us(lambda: eng.bwd(params, st, None, ids, True, gl, True, False, grads=grads, accumulate=True, ws=ws, cond=q, d_q=d_q), runs)
    without = median_us(lambda: eng.bwd(params, st, None, ids, True, gl, True, False, grads=grads, accumulate=True, ws=ws, cond_entry=True), runs)
    bwd_us = with_q - without
    return {"shape": {"B": B, "R": R, "F": eng.F, "Fp": eng.Fp, "dtype": "bf16"},
            "match_fwd": {"us": round(fwd_us, 2), "bytes": fwd_bytes, "GBps": round(fwd_bytes / fwd_us / 1e3, 1)},
            "match_bwd": {"us": round(bwd_us, 2), "bytes": bwd_bytes, "GBps": round(bwd_bytes / max(bwd_us, 1e-3) / 1e3, 1),
                          "how": "gic_disc_bwd_cond with q minus with q = NULL", "bwd_cond_with_q_us": round(with_q, 2),
                          "bwd_cond_q_null_us": round(without, 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_cond_bench.json"))
    ap.add_argument("--one", default="", help="internal: COND,W -- time that one configuration in this process and print its ms per step")
    a = ap.parse_args()
    if a.one:
        cond, w = a.one.split(",")
        print(json.dumps({"ms": step_ms(cond, float(w), a.steps, a.warmup)}), flush=True)
        return

    def child(cond, w):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{cond},{w}", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the {cond}, w = {w} run failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])["ms"]
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/disc_cond_bench.py", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "runs": a.runs}
    rec["kernels"] = bench_kernels(a.runs, dev)
    off = [child("none", 0.5) for _ in range(2)]
    w0 = child("projection", 0.0)
    w5 = child("projection", 0.5)
    base = min(off)
    rec["step_ms"] = {"flag_off": [round(v, 4) for v in off], "flag_off_spread": round(abs(off[0] - off[1]), 4), "on_w0": round(w0, 4),
                      "on_w0.5": round(w5, 4), "cost_w0_ms": round(w0 - base, 4), "cost_w0.5_ms": round(w5 - base, 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
