"""The trainer with LR schedules, weight decay and the weight EMA (--synthetic 1 at the tiny shapes of tests/test_gpu_training.py): the
defaults against checkpoints recorded from the commit before the feature, everything on for both decoders (logged rates, *_ema.ckpt and
*.train_state files, --resume / --resume-train-state, ema.swapped()), the step graphs under a schedule, and the deterministic mode."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_default_main.json")
TINY = ["--synthetic", "1", "--synthetic-batches", "3", "--synthetic-caption-len", "8", "--vocab-size", "64", "--adv-train-batch-size", "4",
        "--adv-eval-batch-size", "4", "--adv-epochs", "1", "--pretrain-epochs", "1", "--pre-train-batch-size", "4", "--pre-eval-batch-size", "4",
        "--gen-hidden-dim", "32", "--gen-embed-dim", "16", "--image-size", "32", "--encoder-arch", "resnet18", "--num-workers", "0"]
# the run behind tests/golden/optim_default_main.json: every optimizer flag at its default, deterministic mode, the seed main.py sets
DEFAULT_RUN = TINY + ["--conditional-gan", "1", "--compute-dtype", "bf16", "--deterministic", "1"]
ON = ["--pretrain-lr-schedule", "cosine", "--pretrain-lr-warmup-steps", "1", "--adv-lr-schedule", "linear", "--adv-lr-warmup-steps", "1",
      "--lr-min-ratio", "0.1", "--gen-weight-decay", "0.05", "--disc-weight-decay", "0.02", "--gen-ema-decay", "0.9", "--eval-ema", "1",
      "--eval-beam-size", "2", "--max-seq-len", "10"]


def digest(state_dict):
    """sha256 over the tensors of a (possibly nested) state dict, keys in sorted order."""
    h = hashlib.sha256()
    for k in sorted(state_dict):
        v = state_dict[k]
        if isinstance(v, dict):
            h.update(k.encode() + digest(v).encode())
        else:
            t = v.detach().cpu().contiguous().reshape(-1)
            h.update(k.encode() + str(t.dtype).encode() + str(tuple(v.shape)).encode() + t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@pytest.fixture
def det_off():
    from gan_image_captioning_amd import engine
    was = engine.deterministic()
    yield
    engine.set_deterministic(was)


def test_defaults_write_the_checkpoints_of_the_commit_before(tmp_path, det_off):
    """With every new flag at its default `main` writes what it wrote before the flags existed: the digests of pretrained_model.ckpt
    and adv_model.ckpt in deterministic mode at a fixed seed, recorded on an MI355X from commit a921b09 (the one before the optimizer
    features) with this file's `digest`.  The new files beside them (*.train_state) do not change them.  (A later change that alters
    the step's rounding on purpose records the digests again from its own parent commit, the same way.)"""
    from gan_image_captioning_amd.main import main
    from gan_image_captioning_amd.generator import SEEDS
    want = json.load(open(GOLDEN))
    SEEDS.reset(0)                     # the device-noise seed counter of a fresh process
    inst = main(DEFAULT_RUN + ["--save-dir", str(tmp_path), "--expt-name", "d"])
    torch.cuda.synchronize()
    assert inst.ema is None and inst.pretrain_opt._opts is None and inst.gen_opt._opts is None and inst.disc_opt._opts is None
    got = {name: digest(torch.load(os.path.join(inst.model_dir, name), map_location="cpu")) for name in want["digests"]}
    assert got == want["digests"]
    assert sorted(os.listdir(inst.model_dir)) == ["adv_model.ckpt", "adv_model.train_state", "pretrained_model.ckpt", "pretrained_model.train_state"]


def _lam(kind, W, T, r, s):
    from gan_image_captioning_amd.optim import LRSchedule
    return LRSchedule(kind, W, T, r).multiplier(s)


@pytest.mark.parametrize("decoder", ["lstm", "attention"])
def test_everything_on(tmp_path, monkeypatch, decoder):
    from gan_image_captioning_amd import training
    from gan_image_captioning_amd.main import main
    scalars = []
    monkeypatch.setattr(training._ScalarWriter, "add_scalar", lambda self, tag, value, step: scalars.append((tag, float(value), int(step))))
    base = TINY + ON + ["--conditional-gan", "1", "--compute-dtype", "bf16", "--decoder", decoder, "--save-dir", str(tmp_path)]
    scst = ["--scst-epochs", "1", "--scst-samples", "3"] if decoder == "lstm" else []
    first = main(base + scst + ["--expt-name", "a"])
    torch.cuda.synchronize()
    a = first.args
    n_scst = first.scst_steps
    assert (int(first.pretrain_opt.step_count), int(first.gen_opt.step_count), int(first.disc_opt.step_count)) == (3, 3, 3)
    assert int(first.ema.count) == 3 + n_scst + 3 and (n_scst > 0) == bool(scst)           # one EMA per arena: every G optimizer advances it
    # the logged rates follow the schedules: lr * lambda(s) against the number s of steps taken
    for tag, lr, (kind, r) in (("GenPreTraining_lr", a.pretrain_lr, ("cosine", 0.1)), ("Generator_lr", a.gen_lr, ("linear", 0.1)),
                               ("Discriminator_lr", a.disc_lr, ("linear", 0.1))):
        got = [(s, v) for t, v, s in scalars if t == tag]
        assert [s for s, _ in got] == [1, 2, 3], tag
        for s, v in got:
            assert v == lr * _lam(kind, 1, 3, r, s), (tag, s)
    assert _lam("cosine", 1, 3, 0.1, 1) == 1.0 and _lam("cosine", 1, 3, 0.1, 3) == pytest.approx(0.1)
    assert any(t == "BLEU4_val" for t, _, _ in scalars)                                    # --eval-beam-size ran (on the averaged weights)
    # the device agrees with the host's count: the last step's lr_t
    assert float(first.gen_opt.sched_out[0]) == pytest.approx(a.gen_lr * _lam("linear", 1, 3, 0.1, 2), rel=2e-7)
    # the files
    names = ["pretrained_model", "adv_model"] + (["scst_model"] if scst else [])
    for n in names:
        for suffix in (".ckpt", "_ema.ckpt", ".train_state"):
            assert os.path.exists(os.path.join(first.model_dir, n + suffix)), n + suffix
    live = torch.load(os.path.join(first.model_dir, "adv_model.ckpt"), map_location="cpu")
    ema_path = os.path.join(first.model_dir, "adv_model_ema.ckpt")
    avg = torch.load(ema_path, map_location="cpu")
    assert set(avg) == {"generator", "discriminator"} and set(avg["generator"]) == set(live["generator"])
    assert digest(avg["discriminator"]) == digest(live["discriminator"])
    arena_keys = {k for k, v in first.gen.state_dict().items()
                  if any(v.data_ptr() == p.data_ptr() for p in first.gen_arena.params)}
    assert arena_keys and any(k.startswith("encoder.bn.") for k in arena_keys) and any(k.startswith("decoder.") for k in arena_keys)
    for k in live["generator"]:
        same = torch.equal(avg["generator"][k], live["generator"][k])
        if k in arena_keys and live["generator"][k].dim() >= 2:          # (weight decay alone moves every matrix at every step)
            assert not same, f"{k}: the averaged checkpoint holds the live weights"
        elif k not in arena_keys:
            assert same, f"{k} is outside the arena: not averaged"
    state = torch.load(os.path.join(first.model_dir, "adv_model.train_state"), map_location="cpu")
    assert set(state) == {"pretrain_opt", "gen_opt", "disc_opt", "ema"} | ({"scst_opt"} if scst else set())
    # --resume takes the averaged checkpoint like any other, --resume-train-state restores the counters, the moments and the average
    second = main(base + ["--expt-name", "b", "--resume", ema_path, "--resume-train-state", os.path.join(first.model_dir, "adv_model.train_state"),
                          "--pretrain-epochs", "0", "--adv-epochs", "0", "--pretrain-lr-schedule", "none", "--adv-lr-schedule", "invsqrt"])
    torch.cuda.synchronize()
    for k, v in second.gen.state_dict().items():
        assert torch.equal(v.cpu(), avg["generator"][k]), k
    for name in ("pretrain_opt", "gen_opt", "disc_opt"):
        o2, sd = getattr(second, name), state[name]
        assert int(o2.step_count) == int(sd["step"]) == 3 and o2.steps == 3
        assert torch.equal(o2.exp_avg.cpu(), sd["exp_avg"]) and torch.equal(o2.exp_avg_sq.cpu(), sd["exp_avg_sq"])
    # (the train state was written with the best adversarial checkpoint; one validation pass later the live EMA is still that one)
    assert torch.equal(second.ema.shadow.cpu(), state["ema"]["shadow"]) and torch.equal(second.ema.shadow, first.ema.shadow)
    assert int(second.ema.count) == int(state["ema"]["count"]) == int(first.ema.count)
    assert second.gen_opt.current_lr() == a.gen_lr * _lam("invsqrt", 1, 0, 0.1, 3)
    # without a train state the average restarts from the loaded weights
    second.load_checkpoint(ema_path)
    assert int(second.ema.count) == 0 and torch.equal(second.ema.shadow, second.gen_arena.flat)
    # inside ema.swapped() the generator captions as one that loaded *_ema.ckpt; afterwards the live weights are back, bit for bit
    images = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(a.device)
    first.gen.eval(), second.gen.eval()
    before, shadow = first.gen_arena.flat.clone(), first.ema.shadow.clone()
    with first.ema.swapped():
        assert torch.equal(first.gen_arena.flat, shadow) and torch.equal(first.ema.shadow, before)
        got = first.gen.caption(images, beam_size=2, max_caption_len=10)
    want = second.gen.caption(images, beam_size=2, max_caption_len=10)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    own = first.gen.caption(images, beam_size=2, max_caption_len=10)
    assert torch.equal(first.gen_arena.flat, before) and torch.equal(first.ema.shadow, shadow)
    with pytest.raises(RuntimeError, match="inside"):
        with first.ema.swapped():
            raise RuntimeError("inside")
    assert torch.equal(first.gen_arena.flat, before) and torch.equal(first.ema.shadow, shadow)
    assert all(torch.equal(x, y) for x, y in zip(own, first.gen.caption(images, beam_size=2, max_caption_len=10)))


def _instructor(**kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.training import GANInstructor
    base = dict(vocab_size=64, gen_embed_dim=16, gen_hidden_dim=32, conditional_gan=0, adv_train_batch_size=4, compute_dtype="fp32",
                device="cuda", log_file=None, model_dir=None, save_dir=None, adv_lr_schedule="invsqrt", adv_lr_warmup_steps=2,
                pretrain_lr_schedule="step", pretrain_lr_warmup_steps=1, lr_step_size=2, lr_step_gamma=0.5, lr_min_ratio=0.1,
                gen_weight_decay=0.05, disc_weight_decay=0.02, gen_ema_decay=0.9)
    torch.manual_seed(1008)
    inst = GANInstructor(default_args(**dict(base, **kw)), None, None)
    inst.gen.train(), inst.disc.train()
    return inst


def test_step_graphs_are_captured_once_under_a_schedule(monkeypatch):
    """The schedule lives in the update kernel: `opt.lr` stays the base rate, so the step's graph key never changes and the graphs
    captured at step 2 are replayed from then on while the rate moves every step."""
    from gan_image_captioning_amd.tasks import synthetic_batch
    monkeypatch.setenv("GIC_STEP_GRAPH", "1")
    monkeypatch.delenv("GIC_NO_STEP_GRAPH", raising=False)
    monkeypatch.delenv("GIC_NO_GRAPH", raising=False)
    inst = _instructor()
    assert inst.fused.use_graph
    _, caps, _, L = synthetic_batch(4, 64, 32, 8, seed=3, device="cuda", with_images=False)
    keys, rates, ids = set(), [], []
    for s in range(6):
        inst.fused(None, caps, L, True)
        keys.add(inst.fused._graph_key(4, L))
        rates.append((float(inst.gen_opt.sched_out[0]), float(inst.disc_opt.sched_out[0])))
        ids.append({name: id(g) for name, g in next(iter(inst.fused._graphs.values()))["graphs"].items()} if inst.fused._graphs else None)
    assert len(keys) == 1 and len(inst.fused._warm) == 1 and len(inst.fused._graphs) == 1
    assert ids[0] is None and ids[1] and all(i == ids[1] for i in ids[2:])                  # eager, capture, four replays of the same graphs
    a = inst.args
    assert inst.gen_opt.lr == a.gen_lr and inst.disc_opt.lr == a.disc_lr
    for s, (g, d) in enumerate(rates):
        assert g == pytest.approx(a.gen_lr * _lam("invsqrt", 2, 0, 0.1, s), rel=2e-7) and d == pytest.approx(a.disc_lr * _lam("invsqrt", 2, 0, 0.1, s), rel=2e-7)
    assert len({g for g, _ in rates}) == 6 and int(inst.ema.count) == int(inst.gen_opt.step_count) == 6
    assert bool(torch.isfinite(inst.gen_arena.flat).all() and torch.isfinite(inst.ema.shadow).all())


def test_deterministic_mode_repeats_bit_for_bit_with_everything_on(det_off):
    """Two runs of 3 adversarial and 3 pre-training steps from the same seed: the new path has no atomics, nothing to switch."""
    from gan_image_captioning_amd.generator import SEEDS
    from gan_image_captioning_amd.tasks import synthetic_batch
    _, caps, _, L = synthetic_batch(4, 64, 32, 8, seed=3, device="cuda", with_images=False)
    runs = []
    for _ in range(2):
        inst = _instructor(deterministic=1)
        SEEDS.reset(77)
        for _s in range(3):
            inst.fused(None, caps, L, True)
            inst.pretrain_step(None, caps, L, train=True)
        torch.cuda.synchronize()
        assert int(inst.ema.count) == 6
        runs.append({"gen": inst.gen_arena.flat, "disc": inst.disc_arena.flat, "ema": inst.ema.shadow, "gm": inst.gen_opt.exp_avg,
                     "gv": inst.gen_opt.exp_avg_sq, "pm": inst.pretrain_opt.exp_avg, "dm": inst.disc_opt.exp_avg,
                     "so": torch.cat([inst.gen_opt.sched_out, inst.pretrain_opt.sched_out, inst.disc_opt.sched_out])})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert bool(torch.isfinite(runs[0][k]).all()), k
    assert not torch.equal(runs[0]["ema"], runs[0]["gen"])
