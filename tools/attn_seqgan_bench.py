"""SeqGAN step of the attention decoder at the benchmark shape (tools only; needs a GPU, no CPU fallback): B=32, L=20, V=10000,
E=H=512, C=2048, P=49, A=512, N=16 roll-outs per prefix (9728 roll-out rows), bf16.  HIP events, warm-up, medians of >= 20 timed
repetitions:
  rollout   the gic_attn_rollout call alone (engine.AttnDecoderEngine.rollout from a kept teacher-forced state)
  step      the whole step (--adv-mode seqgan --decoder attention --conditional-gan 1, ResNet-50 trunk at 224x224, look-ahead trunk pass)
and the workspace size.  python tools/attn_seqgan_bench.py [--reps 20] [--rollouts 16] [--only rollout|step]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, L, V, E, H, C, P, A = 32, 20, 10000, 512, 512, 2048, 49, 512


def timed_us(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def summary(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1), "reps": len(us)}


def bench_rollout(N, reps):
    from gan_image_captioning_amd import engine as Eg
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    u = lambda *s: torch.empty(*s).uniform_(-0.05, 0.05, generator=g).to(dev)          # noqa: E731
    params = [u(V, E), u(4 * H, E + C), u(4 * H, H), u(4 * H), u(4 * H), u(V, H), u(V), u(A, C), u(A), u(A, H), u(A)]
    eng = Eg.AttnDecoderEngine(V, E, H, C, P, A, 1)
    feats = (torch.randn(B, E, generator=g) * 0.3).to(dev)
    fmap = torch.relu(torch.randn(B, P, C, generator=g)).to(dev)
    _, Y, _ = eng.sample_fwd(params, feats, fmap, L, 1.0, seed=1)
    saved = eng.forward_tf(params, feats, fmap, Y[:, :-1], [L] * B, 1.0, pretrain=True, keep_state=True)[3]
    rows = (L - 1) * N * B
    nbytes = eng.rollout_ws_bytes(B, L, rows)
    ws = torch.empty(nbytes + 256, device=dev, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 256:][:nbytes]
    res = summary(timed_us(lambda: eng.rollout(params, saved, Y, N, seed=2, ws=ws), reps))
    res.update(rows=rows, ws_bytes=nbytes, row_steps=sum(s * N * B for s in range(1, L)))
    return res


def bench_step(N, reps):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, conditional_gan=1, encoder_arch="resnet50", decoder="attention",
                        attn_dim=A, adv_mode="seqgan", mc_rollouts=N, compute_dtype="bf16", adv_train_batch_size=B, image_size=224,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(1008)
    inst = GANInstructor(args, None, None)
    inst.gen.train(); inst.disc.train()
    dev = args.device
    g = torch.Generator().manual_seed(0)
    images = [torch.randn(B, 3, 224, 224, generator=g).to(dev) for _ in range(2)]
    caps = torch.randint(0, V, (B, L), generator=g).to(dev)
    k = [0]

    def step():
        k[0] += 1
        inst.adv_step(images[k[0] & 1], caps, L, train=True, next_images=images[(k[0] + 1) & 1])

    res = summary(timed_us(step, reps))
    res["rollout_rows"] = (L - 1) * N * B
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rollouts", type=int, default=16)
    ap.add_argument("--only", choices=["rollout", "step"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_seqgan_bench needs a GPU")
    reps = max(20, a.reps)
    out = {"shape": dict(B=B, L=L, V=V, E=E, H=H, C=C, P=P, A=A, N=a.rollouts, dtype="bf16")}
    if a.only != "step":
        out["rollout"] = bench_rollout(a.rollouts, reps)
        print(f"rollout: median {out['rollout']['median_us']:.0f} us over {reps} reps, workspace {out['rollout']['ws_bytes'] / 2**20:.1f} MiB, "
              f"{out['rollout']['rows']} rows")
    if a.only != "rollout":
        out["step"] = bench_step(a.rollouts, reps)
        print(f"step:    median {out['step']['median_us']:.0f} us over {reps} reps")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
