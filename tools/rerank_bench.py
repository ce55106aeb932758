"""D-guided re-ranking and image-caption retrieval on the MI355X, at cfg2 shapes: B = 64 images of 224 x 224, L = 20,
V = 10 000, E = H = 512, ResNet-50 trunk, bf16; D with R = 64, filters (3, 4, 5) x 300 (F = 900, Fp = 960), --disc-cond projection.

  caption    Generator.caption at K = 5 without and with rerank_disc, for both decoders: wall time per call (host clock around --steps
             calls that end in a device synchronise, after --warmup), each configuration in a fresh child process (as
             tools/disc_cond_bench.py: a second model in one process does not time like the first)
  sample     Generator.sample_captions, best of 8, without and with rerank_disc (LSTM decoder)
  retrieval  GANInstructor.evaluate_retrieval at N = 1000 and 5000 (batches of 64, every batch the same device tensors: the trunk and D
             do the work of N distinct items), the median of --steps calls after --warmup; its three device phases from HIP events
             recorded where they begin: accumulation (trunk, img_proj, D forward, gic_disc_rep_mean per batch), the f32 GEMM
             S = F^-1/2 Ybar Q^T, and gic_match_ranks
  kernels    HIP events around single launches, median of --runs: gic_match_ranks against the bytes of S it reads once (4 N^2);
             gic_disc_match_fwd_grouped (identity index, and 5 captions per image) against gic_disc_match_fwd on the same 320 x 64 rows;
             gic_rerank and gic_disc_rep_mean.  A launch of a few microseconds is measured together with its launch gap.

python tools/rerank_bench.py [--steps 10] [--warmup 3] [--runs 200] [--out profiles/rerank_bench.json]"""
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
K_BEAMS, N_SAMPLES = 5, 8


def make_args(decoder, batch=CFG2["B"]):
    from gan_image_captioning_amd.args import default_args
    extra = dict(decoder="attention") if decoder == "attention" else dict(gen_num_layers=CFG2["NL"])
    return default_args(vocab_size=CFG2["V"], gen_embed_dim=CFG2["E"], gen_hidden_dim=CFG2["H"], conditional_gan=1, encoder_arch="resnet50",
                        compute_dtype="bf16", image_size=CFG2["S"], max_seq_len=CFG2["L"], adv_train_batch_size=batch, adv_eval_batch_size=batch,
                        disc_cond="projection", device="cuda", log_file=None, model_dir=None, save_dir=None, **extra)


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def decode_ms(what, decoder, rerank, steps, warmup):
    from gan_image_captioning_amd.discriminator import Discriminator
    from gan_image_captioning_amd.generator import Generator
    args = make_args(decoder)
    torch.manual_seed(1008)
    gen, disc = Generator(args).to(args.device).eval(), Discriminator(args).to(args.device).eval()
    images = torch.randn(CFG2["B"], 3, CFG2["S"], CFG2["S"], generator=torch.Generator().manual_seed(1008)).to(args.device)
    kw = dict(rerank_disc=disc, rerank_weight=1.0) if rerank else {}
    if what == "caption":
        return wall_ms(lambda: gen.caption(images, beam_size=K_BEAMS, max_caption_len=CFG2["L"], **kw), steps, warmup)
    return wall_ms(lambda: gen.sample_captions(images, num_samples=N_SAMPLES, max_caption_len=CFG2["L"], seed=5, **kw), steps, warmup)


class _SameBatch:
    """A loader of ``n`` items in batches of B that hands out the same device tensors every time."""

    def __init__(self, n, images, captions):
        self.dataset, self.images, self.captions = range(n), images, captions

    def __iter__(self):
        B = self.images.shape[0]
        for s in range(0, len(self.dataset), B):
            k = min(B, len(self.dataset) - s)
            yield self.images[:k], self.captions[:k]


def retrieval_ms(N, steps, warmup):
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.tasks import synthetic_batch
    from gan_image_captioning_amd.training import GANInstructor
    args = make_args("lstm")
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.eval()
    inst.disc.eval()
    images, captions, _, _ = synthetic_batch(CFG2["B"], CFG2["V"], CFG2["S"], CFG2["L"], seed=1008, device=args.device, with_images=True)
    inst.adv_eval_loader = _SameBatch(N, images, captions)
    inst.writer.add_scalar = lambda *a, **k: None
    ev = {}
    gemm, ranks = engine.gemm, engine.match_ranks

    def mark(name):
        ev[name] = torch.cuda.Event(enable_timing=True)
        ev[name].record()

    def gemm_marked(A, Bm, Cout, M, Nn, *a, **k):
        if M == N and Nn == N:
            mark("gemm")
        return gemm(A, Bm, Cout, M, Nn, *a, **k)

    def ranks_marked(*a, **k):
        mark("ranks")
        out = ranks(*a, **k)
        mark("end")
        return out
    engine.gemm, engine.match_ranks = gemm_marked, ranks_marked
    phases = {"accumulate_ms": [], "gemm_ms": [], "ranks_ms": []}
    walls = []
    try:
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mark("start")
            out = inst.evaluate_retrieval("val", max_items=N)
            torch.cuda.synchronize()
            if i >= warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
                phases["accumulate_ms"].append(ev["start"].elapsed_time(ev["gemm"]))
                phases["gemm_ms"].append(ev["gemm"].elapsed_time(ev["ranks"]))
                phases["ranks_ms"].append(ev["ranks"].elapsed_time(ev["end"]))
    finally:
        engine.gemm, engine.match_ranks = gemm, ranks
    assert out["n"] == N
    rec = {"N": N, "batches": -(-N // CFG2["B"]), "wall_ms": round(statistics.median(walls), 3)}
    rec.update({k: round(statistics.median(v), 4) for k, v in phases.items()})
    return rec


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
    B, K, R, V = CFG2["B"], K_BEAMS, 64, CFG2["V"]
    eng = engine.DiscEngine(V, 64, R, [3, 4, 5], [300, 300, 300], L.BF16)
    g = torch.Generator().manual_seed(0)
    caps = B * K
    y = torch.randn(caps * R, eng.Fp, generator=g).to(torch.bfloat16)
    y[:, eng.F:] = 0
    st = {"ydrop": y.to(dev)}
    q_rows = torch.randn(caps, eng.F, generator=g).to(dev)
    q_img = q_rows[:B].contiguous()
    logits = torch.zeros(caps * R, device=dev)
    ident = torch.arange(caps, dtype=torch.int32, device=dev)
    group = (torch.arange(caps, device=dev) // K).to(torch.int32)
    y_bytes = caps * R * eng.Fp * 2
    rec = {"match_shape": {"captions": caps, "R": R, "F": eng.F, "Fp": eng.Fp, "dtype": "bf16", "bytes": y_bytes}}
    for name, fn in (("match_fwd", lambda: eng.match_logits(st, q_rows, logits=logits)),
                     ("match_fwd_grouped_identity", lambda: eng.match_logits(st, q_rows, logits=logits, q_index=ident)),
                     ("match_fwd_grouped_5_per_image", lambda: eng.match_logits(st, q_img, logits=logits, q_index=group)),
                     ("match_fwd_again", lambda: eng.match_logits(st, q_rows, logits=logits))):
        us = median_us(fn, runs)
        rec[name] = {"us": round(us, 2), "GBps": round(y_bytes / us / 1e3, 1)}
    ybar, lbar = torch.empty(caps, eng.F, device=dev), torch.empty(caps, device=dev)
    us = median_us(lambda: eng.rep_mean(st, logits, ybar=ybar, lbar=lbar), runs)
    rec["rep_mean"] = {"us": round(us, 2), "bytes": y_bytes, "GBps": round(y_bytes / us / 1e3, 1)}
    lm = -torch.rand(B, K, generator=g).sort(1).values.to(dev)
    lengths = torch.randint(1, CFG2["L"] + 1, (B, K), generator=g, dtype=torch.int32).to(dev)
    ids = torch.randint(0, V, (B, K, CFG2["L"]), generator=g).to(dev)
    alphas = torch.rand(B, K, CFG2["L"], 49, generator=g).to(dev)
    rec["rerank_K5"] = {"us": round(median_us(lambda: engine.rerank(lm, lengths, logits, R, 1.0, 0.0, ids=ids), runs), 2)}
    rec["rerank_K5_alphas_P49"] = {"us": round(median_us(lambda: engine.rerank(lm, lengths, logits, R, 1.0, 0.0, ids=ids, alphas=alphas), runs), 2)}
    for N in (1000, 5000):
        S, bias = torch.randn(N, N, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
        us = median_us(lambda: engine.match_ranks(S, bias), runs)
        rec[f"match_ranks_N{N}"] = {"us": round(us, 2), "bytes": 4 * N * N, "GBps": round(4 * N * N / us / 1e3, 1)}
        Yb, Q = torch.randn(N, eng.F, generator=g).to(dev), torch.randn(N, eng.F, generator=g).to(dev)
        us = median_us(lambda: engine.gemm(Yb, Q, S, N, N, eng.F, eng.F, eng.F, N, True, True, alpha=eng.match_scale()), runs)
        rec[f"score_gemm_f32_N{N}"] = {"us": round(us, 2), "TFLOPs": round(2 * N * N * eng.F / us / 1e6, 2)}
    return rec


CHILDREN = [("caption", "lstm", 0), ("caption", "lstm", 1), ("caption", "attention", 0), ("caption", "attention", 1), ("sample", "lstm", 0),
            ("sample", "lstm", 1), ("retrieval", "1000", 0), ("retrieval", "5000", 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_bench.json"))
    ap.add_argument("--one", default="", help="internal: WHAT,ARG,RERANK -- time that one configuration in this process and print it")
    a = ap.parse_args()
    if a.one:
        what, arg, rr = a.one.split(",")
        if what == "retrieval":
            print(json.dumps(retrieval_ms(int(arg), a.steps, a.warmup)), flush=True)
        else:
            print(json.dumps({"ms": round(decode_ms(what, arg, bool(int(rr)), a.steps, a.warmup), 4)}), flush=True)
        return

    def child(what, arg, rr):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{what},{arg},{rr}", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the {what}, {arg}, rerank = {rr} run failed (status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/rerank_bench.py", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "runs": a.runs,
           "shapes": dict(CFG2, K=K_BEAMS, best_of=N_SAMPLES, R=64, F=900, dtype="bf16")}
    rec["kernels"] = bench_kernels(a.runs, dev)
    for what, arg, rr in CHILDREN:              # the first failing child ends the run: nothing more is started on the device after it
        out = child(what, arg, rr)
        if what == "retrieval":
            rec[f"retrieval_N{arg}"] = out
        else:
            rec.setdefault(f"{what}_{arg}_ms", {})["rerank" if rr else "plain"] = out["ms"]
    for k in ("caption_lstm_ms", "caption_attention_ms", "sample_lstm_ms"):
        rec[k]["cost_ms"] = round(rec[k]["rerank"] - rec[k]["plain"], 4)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
