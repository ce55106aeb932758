"""The optimizer step at the cfg2 generator and discriminator arena sizes (as GANInstructor lays them out: the modules' parameter lists
in padded 16-byte slots, --conditional-gan 1): gic_clip_adam; gic_clip_adamw with each feature alone (schedule, decay over the
arena's own decay ranges, EMA) and with all of them; and what a user would otherwise write for the EMA: gic_clip_adam followed by
shadow.lerp_(flat, 1 - d) in torch.

Every variant is two launches (three with the torch lerp_) on arenas of a few tens of MB, so a call is timed as the average of
--inner back-to-back calls between two device events on the launch stream (the arenas are re-read from HBM or the 256 MB last-level
cache exactly as in a train step that runs nothing else; the step's other kernels would evict them, which this does not model).  The
variants are interleaved --repeats times after --warmup calls each; the table gives the median and the spread (min .. max) of the
repeats, and bytes/s from the bytes the algorithm needs (28 B per element: p, m, v read and written, g read; + 8 B with the EMA; the
torch lerp_ adds 12 B: p and the shadow read, the shadow written).  Writes profiles/optim_bench.json and prints one JSON line per row.
   python tools/optim_bench.py [--repeats 15] [--inner 50] [--warmup 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arenas():
    """(name, numel, decay ranges) of the two arenas at cfg2, from the modules' parameter lists (built on the CPU: shapes only)."""
    import bench
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.discriminator import Discriminator
    from gan_image_captioning_amd.generator import Generator
    from gan_image_captioning_amd.optim import slot_ranges
    c = bench.CFG2
    args = default_args(vocab_size=c["V"], gen_embed_dim=c["E"], gen_hidden_dim=c["H"], gen_num_layers=c["NL"], conditional_gan=1,
                        image_size=c["S"], device="cpu")
    gen, disc = Generator(args), Discriminator(args)
    g = list(gen.decoder.parameters()) + list(gen.encoder.linear.parameters()) + list(gen.encoder.bn.parameters())
    out = []
    for name, params in (("G", g), ("D", list(disc.parameters()))):
        out.append((name, sum((p.numel() + 3) // 4 * 4 for p in params), slot_ranges(params)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    import torch
    from gan_image_captioning_amd import engine
    assert torch.cuda.is_available(), "optim_bench measures on the GPU: no device, no numbers"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    lr, d, wd = 1e-4, 0.999, 0.01
    rows = []
    for arena, n, ranges in arenas():
        gen = torch.Generator().manual_seed(1008)
        flat, grad = (0.05 * torch.randn(n, generator=gen)).to(dev), (1e-3 * torch.randn(n, generator=gen)).to(dev)
        m, v, shadow = torch.zeros_like(flat), torch.zeros_like(flat), flat.clone()
        step, count = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        norm, so = torch.zeros(1, device=dev), torch.zeros(2, device=dev)
        partials = torch.zeros(engine.clip_adam_partials(n), device=dev)
        fl = [x for r in ranges for x in r]
        rd = torch.tensor(fl, dtype=torch.int64, device=dev)
        base = (flat, grad, m, v, lr, 0.9, 0.999, 1e-8, 5.0, step, norm, partials)
        sched = dict(schedule="cosine", warmup_steps=1000, total_steps=100000, min_ratio=0.1)
        ema = dict(ema=shadow, ema_count=count, ema_decay=d, ema_warmup=True)
        opts = {"adamw neutral": engine.adamw_opts(sched_out=so),
                "adamw schedule": engine.adamw_opts(sched_out=so, **sched),
                "adamw decay": engine.adamw_opts(wd, fl, rd, sched_out=so),
                "adamw ema": engine.adamw_opts(sched_out=so, **ema),
                "adamw all": engine.adamw_opts(wd, fl, rd, sched_out=so, **sched, **ema)}

        def lerp():
            engine.clip_adam(*base)
            shadow.lerp_(flat, 1.0 - d)
        variants = {"clip_adam": lambda: engine.clip_adam(*base), "clip_adam + torch lerp_": lerp}
        for k, o in opts.items():
            variants[k] = (lambda o: lambda: engine.clip_adamw(*base, o))(o)
        bytes_per = {k: 28 + (8 if "ema" in k or "all" in k else 0) + (12 if "lerp_" in k else 0) for k in variants}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():             # interleaved: a drift of the machine hits every variant alike
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(a.inner):
                    fn()
                t1.record(stream)
                t1.synchronize()
                us[k].append(t0.elapsed_time(t1) * 1e3 / a.inner)
        assert bool(torch.isfinite(flat).all() and torch.isfinite(shadow).all())
        for k in variants:
            med = statistics.median(us[k])
            rows.append({"arena": arena, "numel": n, "decay_ranges": len(ranges), "variant": k, "launches": 3 if "lerp_" in k else 2,
                         "us_median": round(med, 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2),
                         "bytes_per_element": bytes_per[k], "GBps": round(n * bytes_per[k] / med * 1e-3, 1),
                         "repeats": a.repeats, "inner": a.inner})
            print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
