"""Command-line / config surface, drop-in for the reference's ``src/args.py``.

Every flag of the reference keeps its name, type and default (args.py:12-257); the parsed
Namespace doubles as the model-config object exactly as there.  ``get_args()`` keeps the
side effects too: a fresh ``<save-dir>/<expt-name>_<n>/`` with a ``models/`` sub-directory
(args.py:261-273) and ``args.device`` resolved to a ``torch.device`` (args.py:275-278).

New flags (all optional, defaults preserve the reference behaviour where one exists) select the
MI355X-specific knobs: compute dtype, synthetic data, fused step, data-parallel options.
"""
from __future__ import annotations

import argparse
import os

import torch

# (flag, type, default, help[, extra kwargs])  -- reference flags, args.py line numbers in comments
_MODEL = [
    ("--gen-hidden-dim", int, 512, "hidden dimension of generator"),                      # :12
    ("--gen-embed-dim", int, 32, "embedding dimension of generator"),                     # :17
    ("--gen-num-layers", int, 1, "number of layers in generator"),                        # :22
    ("--gen-init", str, "uniform", "Initialization strategy for generator weights"),      # :27
    ("--disc-embed-dim", int, 64, "embeddings dimension to use in discriminator"),        # :34
    ("--disc-num-rep", int, 64, "number of representations to use for CNN discriminator"),  # :39
    # the reference declares these two with type=list (args.py:44-52), which only works at the defaults;
    # here a comma-separated list is accepted as well
    ("--disc-filter-sizes", "intlist", [3, 4, 5], "Layer wise filter sizes to use in discriminator"),
    ("--disc-num-filters", "intlist", [300, 300, 300], "number of filters to use in discriminator per layer"),
    ("--disc-init", str, "uniform", "init strategy for discriminator weights"),            # :54
    ("--conditional-gan", int, 0, "is the gan conditional?", {"choices": [0, 1]}),         # :61
]
_DATA = [
    ("--vocab-size", int, -1, "vocab size for training"),                                  # :78
    ("--max-seq-len", int, 34, "maximum sequence length of captions"),                     # :83
    ("--padding-idx", int, 0, "index of padding token in vocab"),                          # :88
    ("--image-size", int, 256, "resize dim of images"),                                    # :96
    ("--captions-per-image", int, 1, "no of captions to use per image"),                   # :101
    ("--dataset_percent", float, 1.0, "percentage of dataset to use for training"),        # :108
]
_TRAIN = [
    ("--pretrain-lr", float, 1e-2, "learning rate for pretraining generator"),             # :123
    ("--pretrain-epochs", int, 0, "number of epochs for pretraining generator"),           # :128
    ("--pre-train-batch-size", int, 64, "batch size of pretrain training"),                # :133
    ("--pre-eval-batch-size", int, 64, "batch size of pretrain evaluation"),               # :138
    ("--gen-lr", float, 1e-4, "learning rate for adversarial training of generator"),      # :145
    ("--disc-lr", float, 1e-4, "learning rate for adversarial training of discriminator"),  # :150
    ("--disc-train-freq", int, 1, "ratio of training steps of disc vs gen (parsed, unused as in the reference)"),  # :155
    ("--adv-epochs", int, 30, "number of epochs for adversarial training"),                # :160
    ("--adv-train-batch-size", int, 64, "batch size of adversarial training"),             # :165
    ("--adv-eval-batch-size", int, 64, "batch size of adversarial evaluation"),            # :170
    ("--adv-loss-type", str, "standard", "Loss function to use for adversarial training"),  # :175
    ("--temperature", int, 100, "Temperature for rel gan training"),                       # :180
    ("--temp-adpt", str, "exp", "Temperature adoption strategy"),                          # :185
    ("--clip-norm", float, 5.0, "Gradient clipping threshold"),                            # :190
]
_GLOBAL = [
    ("--device", str, "cuda", "device to use for training (cpu|cuda)"),                    # :208
    ("--device-ids", int, 0, "device id (parsed, unused as in the reference)"),            # :213
    ("--expt-name", str, "debug", "Name of the experiment"),                               # :218
    ("--model-dir", str, "models", "directory to save models"),                            # :223
    ("--data-dir", str, "./data", "directory where data is stored"),                       # :228
    ("--save-dir", str, "./save", "directory to save the expt logs and tensorboard logs"),  # :233
    ("--adv-log-step", int, 1, "Log step frequency for adversarial training"),             # :238
    ("--pre-log-step", int, 1, "Log step frequency for pretraining"),                      # :243
    ("--test-log-step", int, 1, "Log step frequency for testing (parsed, unused)"),        # :248
    ("--log-file", str, "log", "Log file to save logs"),                                   # :253
]
# MI355X-native additions (no reference counterpart)
_NATIVE = [
    ("--compute-dtype", str, "bf16", "MFMA operand dtype: bf16 (perf) or fp32 (parity)", {"choices": ["bf16", "fp32"]}),
    ("--encoder-arch", str, "resnet18", "trunk shape: resnet18 (the reference's) or resnet50", {"choices": ["resnet18", "resnet50"]}),
    ("--step-impl", str, "fused", "adversarial step driver: fused (direct kernel sequence) or autograd (module API)",
     {"choices": ["fused", "autograd"]}),
    ("--adv-mode", str, "relgan", "generator update of the adversarial loop: relgan = Gumbel-softmax relaxation through D (the reference, "
                                  "training.py:144-169); seqgan = policy gradient with Monte-Carlo roll-outs scored by D (either --decoder)", {"choices": ["relgan", "seqgan"]}),
    ("--mc-rollouts", int, 16, "Monte-Carlo roll-outs per prefix (--adv-mode seqgan)"),
    ("--decoder", str, "lstm", "caption decoder: lstm (the reference, generator.py:27-96) or attention (visual attention over the trunk's "
                               "feature map, Show-Attend-Tell style; needs --conditional-gan 1; trains with either --adv-mode)", {"choices": ["lstm", "attention"]}),
    ("--attn-dim", int, 512, "width of the additive-attention hidden layer (--decoder attention)"),
    ("--real-as-ids", int, 1, "feed real captions to D as token ids (gather) instead of a dense one-hot", {"choices": [0, 1]}),
    ("--synthetic", int, 0, "use synthetic (image, caption) batches instead of COCO", {"choices": [0, 1]}),
    ("--synthetic-batches", int, 8, "batches per epoch of the synthetic dataset"),
    ("--synthetic-caption-len", int, 20, "caption length (incl. <S>/<E>) of synthetic batches"),
    ("--resume", str, "", "checkpoint to start from: adv_model.ckpt ({generator, discriminator}) or pretrained_model.ckpt "
                          "(generator state dict), in the reference's format (training.py:118,225-226); the reference cannot resume"),
    ("--seed", int, 1008, "RNG seed (src/main.py:14 fixes 1008)"),
    ("--deterministic", int, 0, "bit-reproducible train steps (the reference's cudnn.deterministic, src/main.py:22-23): fixed-order "
                                "reductions instead of f32 atomics; 0 leaves the process-wide mode as it is (GIC_DETERMINISTIC=1 sets it "
                                "at load)", {"choices": [0, 1]}),
    ("--num-workers", int, 4, "DataLoader workers (training.py:28-32 uses 4)"),
    ("--pretrain-mode", str, "sample", "MLE pre-training input: sample = the reference's free-running roll-out (sample(pretrain=True), "
                                       "training.py:66-83); teacher = teacher forcing, decoder.forward(features, captions[:, :-1], lengths)",
     {"choices": ["sample", "teacher"]}),
    ("--scheduled-sampling-prob", float, 0.0, "scheduled sampling (Bengio et al., 2015) in --pretrain-mode teacher: each input token of a "
                                              "training batch is the decoder's own pick from the previous step with this probability, "
                                              "else the ground truth; 0 = off (pure teacher forcing).  Validation is never mixed"),
    ("--scheduled-sampling-ramp-epochs", int, 0, "epoch e (0-based) trains with p_e = p * min(1, e / n); 0 = p throughout"),
    ("--scheduled-sampling-pick", str, "sample", "the replaced token: sample = a draw from the previous step's softmax, argmax = its mode",
     {"choices": ["sample", "argmax"]}),
    ("--gen-dropout", float, 0.0, "output dropout of the caption decoder in --pretrain-mode teacher: the LSTM output is dropped with this "
                                  "probability in front of the vocabulary projection, training batches only"),
    ("--attn-reg", float, 0.0, "weight of the doubly stochastic attention penalty mean_b sum_i (1 - sum_t alpha_bti)^2 added to the "
                               "pre-training loss (--decoder attention --pretrain-mode teacher only)"),
    ("--eval-beam-size", int, 0, "beam size of the BLEU-4 evaluation (GANInstructor.evaluate) after each adversarial epoch's validation; "
                                 "0 = off"),
    ("--eval-num-samples", int, 0, "sampled captions per image of the diversity evaluation (GANInstructor.evaluate_diversity: BLEU-4, "
                                   "mBLEU-4, distinct-1/2, vocabulary) after each adversarial epoch's validation; 0 = off"),
    ("--eval-top-k", int, 0, "top-k truncation of the diversity evaluation's sampling; 0 = off"),
    ("--eval-top-p", float, 1.0, "top-p (nucleus) truncation of the diversity evaluation's sampling; 1.0 = off"),
    ("--eval-sample-temperature", float, 1.0, "sampling temperature of the diversity evaluation (divides the logits; not --temperature)"),
    ("--scst-epochs", int, 0, "epochs of self-critical sequence training (CIDEr-D reward, scst.py) after MLE pre-training and before the "
                              "adversarial loop; 0 = off"),
    ("--scst-samples", int, 5, "sampled captions per image of an SCST step (1..8)"),
    ("--scst-baseline", str, "greedy", "SCST baseline: greedy = the CIDEr-D of the greedy caption; mean = the mean reward of the image's "
                                       "other samples (needs --scst-samples >= 2)", {"choices": ["greedy", "mean"]}),
    ("--scst-lr", float, 5e-5, "learning rate of SCST (its own clip + Adam over the generator's parameters)"),
    ("--scst-cider-weight", float, 1.0, "weight of CIDEr-D in the SCST reward (metrics.RewardMix; scores in their native units)"),
    ("--scst-bleu-weight", float, 0.0, "weight of the add-one smoothed sentence BLEU-4 in the SCST reward; with this and "
                                       "--scst-rouge-weight 0 and --scst-cider-weight 1 the reward is the plain CIDEr-D scorer"),
    ("--scst-rouge-weight", float, 0.0, "weight of ROUGE-L in the SCST reward"),
    # optimizer: LR schedules, decoupled weight decay and a weight EMA, all evaluated inside the update kernel (optim.py); every
    # default is off and leaves the optimizers on the plain clip + Adam entry point
    ("--pretrain-lr-schedule", str, "none", "LR schedule of MLE pre-training over pretrain_epochs * len(pre-train loader) steps, after "
                                            "--pretrain-lr-warmup-steps of linear warm-up", {"choices": ["none", "linear", "cosine", "invsqrt", "step"]}),
    ("--adv-lr-schedule", str, "none", "LR schedule of the generator's and the discriminator's adversarial optimizers over adv_epochs * "
                                       "len(adversarial train loader) steps", {"choices": ["none", "linear", "cosine", "invsqrt", "step"]}),
    ("--pretrain-lr-warmup-steps", int, 0, "linear LR warm-up steps of MLE pre-training"),
    ("--adv-lr-warmup-steps", int, 0, "linear LR warm-up steps of the adversarial optimizers"),
    ("--lr-min-ratio", float, 0.0, "floor of every LR schedule as a fraction of the base rate, in [0, 1]"),
    ("--lr-step-size", int, 0, "steps between two decays of the step schedule"),
    ("--lr-step-gamma", float, 0.1, "factor of one decay of the step schedule"),
    ("--gen-weight-decay", float, 0.0, "decoupled (AdamW) weight decay of the generator's matrices and embeddings (pre-training, SCST "
                                       "and adversarial optimizers); biases and BatchNorm affine parameters do not decay"),
    ("--disc-weight-decay", float, 0.0, "decoupled (AdamW) weight decay of the discriminator's embeddings, filters and matrices"),
    ("--gen-ema-decay", float, 0.0, "decay of an exponential moving average of the trainable generator parameters, advanced by every "
                                    "generator optimizer step; 0 = off"),
    ("--gen-ema-warmup", int, 1, "1: the EMA's k-th update uses min(decay, (1 + k) / (10 + k)); 0: the constant decay", {"choices": [0, 1]}),
    ("--eval-ema", int, 0, "1: every evaluate* method runs with the averaged generator (needs --gen-ema-decay > 0); validation losses "
                           "and best-checkpoint selection stay on the live weights", {"choices": [0, 1]}),
    ("--resume-train-state", str, "", "a <checkpoint>.train_state file written beside a model checkpoint: restores the optimizers' "
                                      "moments and step counts and the EMA (loop epoch counters are not restored)"),
    ("--eval-diverse-beam-size", int, 0, "beam size of the diverse-beam-search diversity evaluation (GANInstructor.evaluate_diverse_beam: "
                                         "BLEU-4, mBLEU-4, distinct-1/2, vocabulary) after each adversarial epoch's validation; 0 = off"),
    ("--eval-diverse-groups", int, 2, "groups of that evaluation's diverse beam search (must divide --eval-diverse-beam-size)"),
    ("--eval-diversity-strength", float, 0.5, "Hamming diversity penalty (lambda >= 0) of that evaluation's diverse beam search"),
    ("--eval-cider-beam-size", int, 0, "beam size of the CIDEr-D evaluation (GANInstructor.evaluate_cider) after each adversarial epoch's "
                                       "validation; 0 = off"),
    ("--eval-metrics-beam-size", int, 0, "beam size of the metrics-table evaluation (GANInstructor.evaluate_metrics: BLEU-1..4, ROUGE-L "
                                         "and CIDEr-D scored on the GPU from one decode) after each adversarial epoch's validation; 0 = off"),
    ("--disc-cond", str, "none", "image conditioning of the discriminator: none = D scores the caption alone (the reference); projection = D "
                                 "scores (image, caption) pairs, logits += F^-1/2 <highway output, img_proj(pooled trunk feature)> "
                                 "(needs --conditional-gan 1; not with --adv-mode seqgan)", {"choices": ["none", "projection"]}),
    ("--disc-mismatch-weight", float, 0.5, "w of d_loss = (1 - w) d(real, fake) + w d(real, wrong) under --disc-cond projection: wrong = the "
                                           "real captions against the batch's images rolled by one; 0 <= w < 1, 0 = no third D pass"),
    ("--eval-match", int, 0, "image-caption match evaluation (GANInstructor.evaluate_match: pair accuracy and margin of the match term, "
                             "--disc-cond projection) after each adversarial epoch's validation", {"choices": [0, 1]}),
    ("--eval-no-repeat-ngram", int, 0, "decode constraint of the evaluations (evaluate, evaluate_cider, evaluate_diversity, "
                                       "evaluate_diverse_beam): no n-gram of this size occurs twice in a caption; 0 = off"),
    ("--eval-min-length", int, 0, "decode constraint of the evaluations: <E> is not emitted before this many tokens; 0 = off"),
    ("--eval-suppress-tokens", "intlist", "", "decode constraint of the evaluations: comma-separated token ids (at most 16) that are "
                                              "never emitted, e.g. <S> and <UNK>; empty = none"),
    ("--eval-rerank-weight", float, 0.0, "weight of the discriminator's score in the beam evaluations (evaluate, evaluate_cider, "
                                         "evaluate_metrics): the beams are re-ranked by log-probability + weight * D score "
                                         "(Generator.caption rerank_disc); 0 = off"),
    ("--eval-retrieval", int, 0, "image-caption retrieval evaluation (GANInstructor.evaluate_retrieval: R@1/5/10, median and mean rank in "
                                 "both directions, --disc-cond projection) after each adversarial epoch's validation", {"choices": [0, 1]}),
    ("--eval-retrieval-items", int, 1000, "items of the retrieval evaluation (the first of the split; 1000 = the COCO 1k protocol; at most 8192)"),
    ("--pretrain-ignore-pad", int, 0, "1 = the pre-training loss is the mean over the tokens that are not --padding-idx (gic_xent_seq); "
                                      "0 = the reference's mean over all positions, <PAD> included", {"choices": [0, 1]}),
    ("--label-smoothing", float, 0.0, "label smoothing of the pre-training loss, in [0, 1): the target distribution is (1 - eps) onehot + "
                                      "eps / V (gic_xent_seq).  Training batches only: validation losses stay unsmoothed"),
    ("--eval-perplexity", int, 0, "teacher-forced per-token perplexity of the validation captions (GANInstructor.evaluate_perplexity) after "
                                  "each pre-training and adversarial epoch's validation", {"choices": [0, 1]}),
    ("--device-preprocess", int, 0, "1 = the datasets hand out the decoded uint8 images and one kernel (gic_image_preprocess) resizes, "
                                    "normalises and, under --augment, crops and flips them on the GPU; 0 = the host path (PIL resize + "
                                    "numpy per item)", {"choices": [0, 1]}),
    ("--augment", str, "none", "train-time image augmentation (needs --device-preprocess 1): flip = horizontal flip with p = 0.5, crop = "
                               "random resized crop (area fraction in --augment-crop-scale, aspect ratio in [3/4, 4/3]); validation and "
                               "evaluation never augment", {"choices": ["none", "flip", "crop", "crop-flip"]}),
    ("--augment-crop-scale", "floatpair", (0.5, 1.0), "lo,hi of the random resized crop's area fraction"),
    ("--eval-consensus-samples", int, 0, "sampled captions per image of the consensus evaluation (GANInstructor.evaluate_consensus: CIDEr-D of "
                                         "the first draw and of the consensus pick, Self-CIDEr of the samples; sampling as --eval-top-k / "
                                         "--eval-top-p / --eval-sample-temperature set it) after each adversarial epoch's validation; "
                                         "0 = off", {"choices": list(range(9))}),
    ("--eval-consensus-weight", float, 1.0, "weight of a sample's consensus (its mean CIDEr-D against the image's other samples) beside "
                                            "its log-probability in that evaluation's pick"),
    # decode-time ensemble of the evaluations (generator.Ensemble): members in the order live generator, checkpoints, EMA
    ("--eval-ensemble", "pathlist", "", "comma-separated generator checkpoints (pretrained_model.ckpt, scst_model.ckpt, adv_model.ckpt, "
                                        "*_ema.ckpt) that every evaluate* method ensembles with the live generator at decode time; "
                                        "empty = off"),
    ("--eval-ensemble-ema", int, 0, "1: the averaged generator joins the evaluations' ensemble as its last member (needs --gen-ema-decay "
                                    "> 0; not with --eval-ema 1)", {"choices": [0, 1]}),
    ("--eval-ensemble-weights", "floatlist", "", "comma-separated weights of the ensemble's members in the order live, checkpoints, EMA "
                                                 "(each > 0; normalised to sum 1); empty = uniform"),
    ("--eval-force-words", int, 0, "forced-words evaluation (GANInstructor.evaluate_forced, the oracle-tags protocol: per validation image "
                                   "the N reference tokens with the lowest document frequency among those in at least half of its "
                                   "references are forced into the caption by lexically constrained beam search; BLEU-4, CIDEr-D and the "
                                   "share of captions that hold their words, beside plain beam search's share) after each adversarial "
                                   "epoch's validation; N in 0..3, 0 = off", {"choices": [0, 1, 2, 3]}),
    ("--eval-force-beam-size", int, 8, "beam size of that evaluation (at most 8; 2^N must divide it)"),
    ("--eval-ensemble-mode", str, "prob", "how the members' next-token distributions are mixed: prob = the weighted arithmetic mean of the "
                                          "probabilities, logprob = the weighted geometric mean", {"choices": ["prob", "logprob"]}),
]

MAX_ENSEMBLE = 4          # gicap.h GIC_MAX_ENSEMBLE


def _pathlist(text):
    if isinstance(text, (list, tuple)):
        return [str(v) for v in text]
    return [v.strip() for v in str(text).split(",") if v.strip()]


def _floatlist(text):
    if isinstance(text, (list, tuple)):
        return [float(v) for v in text]
    try:
        return [float(v) for v in str(text).split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated numbers, got {text!r}")


def check_eval_ensemble(args):
    """The evaluations' ensemble as the flags ask for it: None with every flag at its default, else {"paths", "with_ema", "weights"
    (None: uniform), "mode"}.  Refused: --eval-ensemble* with --eval-ema 1, --eval-ensemble-ema 1 without an EMA, more than
    MAX_ENSEMBLE members, weights that are not one positive finite value per member, weights or a mode without any member to mix."""
    paths = _pathlist(getattr(args, "eval_ensemble", "") or "")
    with_ema = bool(int(getattr(args, "eval_ensemble_ema", 0) or 0))
    weights = _floatlist(getattr(args, "eval_ensemble_weights", "") or "")
    mode = getattr(args, "eval_ensemble_mode", "prob") or "prob"
    if mode not in ("prob", "logprob"):
        raise ValueError(f"--eval-ensemble-mode must be prob or logprob, got {mode!r}")
    if not paths and not with_ema:
        if weights or mode != "prob":
            raise ValueError("--eval-ensemble-weights / --eval-ensemble-mode need an ensemble: set --eval-ensemble or --eval-ensemble-ema 1")
        return None
    if int(getattr(args, "eval_ema", 0) or 0):
        raise ValueError("--eval-ensemble* with --eval-ema 1: the evaluations run either on the averaged generator alone (--eval-ema 1) or "
                         "on an ensemble that may hold it as a member (--eval-ensemble-ema 1); use one of the two")
    if with_ema and not float(getattr(args, "gen_ema_decay", 0.0) or 0.0) > 0.0:
        raise ValueError("--eval-ensemble-ema 1 puts the averaged generator into the ensemble: it needs --gen-ema-decay > 0")
    M = 1 + len(paths) + int(with_ema)
    if M > MAX_ENSEMBLE:
        raise ValueError(f"the evaluations' ensemble has {M} members (live, {len(paths)} checkpoints{', EMA' if with_ema else ''}); at most "
                         f"{MAX_ENSEMBLE}")
    if weights:
        if len(weights) != M:
            raise ValueError(f"--eval-ensemble-weights holds {len(weights)} values for {M} members (live, checkpoints, EMA)")
        if not all(0.0 < w < float("inf") for w in weights):
            raise ValueError("--eval-ensemble-weights must be finite and > 0")
    return {"paths": paths, "with_ema": with_ema, "weights": weights or None, "mode": mode}


def check_eval_forced(args):
    """The forced-words evaluation as the flags ask for it: None when --eval-force-words is 0, else (N, beam size).  Refused: N outside
    0..3, a beam size outside 1..8 or one that 2^N does not divide, and the combinations a forced search does not take -- an ensemble
    (--eval-ensemble*) and discriminator re-ranking (--eval-rerank-weight)."""
    n = int(getattr(args, "eval_force_words", 0) or 0)
    if n == 0:
        return None
    k = int(getattr(args, "eval_force_beam_size", 8) or 0)
    if not 1 <= n <= 3:
        raise ValueError(f"--eval-force-words must be 0..3, got {n}")
    if not 1 <= k <= 8 or k % (1 << n):
        raise ValueError(f"--eval-force-beam-size must be 1..8 and a multiple of 2^N = {1 << n} (--eval-force-words {n}), got {k}")
    if _pathlist(getattr(args, "eval_ensemble", "") or "") or int(getattr(args, "eval_ensemble_ema", 0) or 0):
        raise ValueError("--eval-force-words with --eval-ensemble*: the forced search runs one model")
    if float(getattr(args, "eval_rerank_weight", 0.0) or 0.0) != 0.0:
        raise ValueError("--eval-force-words with --eval-rerank-weight: a forced search keeps its own order (constraints met first)")
    return n, k


def _intlist(text):
    if isinstance(text, (list, tuple)):
        return [int(v) for v in text]
    return [int(v) for v in str(text).replace("[", "").replace("]", "").split(",") if v.strip()]


def _floatpair(text):
    if isinstance(text, (list, tuple)):
        vals = [float(v) for v in text]
    else:
        vals = [float(v) for v in str(text).replace("(", "").replace(")", "").split(",") if v.strip()]
    if len(vals) != 2 or not (0.0 < vals[0] <= vals[1] <= 1.0):
        raise argparse.ArgumentTypeError(f"expected lo,hi with 0 < lo <= hi <= 1, got {text!r}")
    return (vals[0], vals[1])


AUGMENT_NEEDS_DEVICE = "--augment {augment} needs --device-preprocess 1: crops and flips are applied by the device image pipeline"


def check_image_pipeline(args) -> None:
    """--augment without --device-preprocess 1 is refused: the host path has no augmentation."""
    augment = getattr(args, "augment", "none")
    if augment != "none" and not int(getattr(args, "device_preprocess", 0)):
        raise ValueError(AUGMENT_NEEDS_DEVICE.format(augment=augment))


def _add(parser, rows):
    for row in rows:
        flag, typ, default, helptext = row[:4]
        extra = dict(row[4]) if len(row) > 4 else {}
        if typ == "intlist":
            typ = _intlist
        elif typ == "floatpair":
            typ = _floatpair
        elif typ == "pathlist":
            typ = _pathlist
        elif typ == "floatlist":
            typ = _floatlist
        parser.add_argument(flag, type=typ, default=default, help=helptext, **extra)


def add_model_args(parser):
    _add(parser, _MODEL)


def add_data_args(parser):
    _add(parser, _DATA)


def add_training_args(parser):
    _add(parser, _TRAIN)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser("NLP GAN args")
    add_training_args(parser)
    add_data_args(parser)
    add_model_args(parser)
    _add(parser, _GLOBAL)
    _add(parser, _NATIVE)
    return parser


def resolve_device(args) -> None:
    """args.py:275-278: 'cuda' -> cuda:0 when available else cpu.  Under torchrun each rank takes
    cuda:LOCAL_RANK (one process per GPU)."""
    if str(args.device).startswith("cuda") and torch.cuda.is_available():
        args.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    else:
        args.device = torch.device("cpu")


def make_experiment_dirs(args) -> None:
    """args.py:261-273: first unused <save_dir>/<expt_name>_<n>, plus its model dir and log file path."""
    n = 1
    while os.path.exists(os.path.join(args.save_dir, f"{args.expt_name}_{n}")):
        n += 1
    args.expt_name = f"{args.expt_name}_{n}"
    args.save_dir = os.path.join(args.save_dir, args.expt_name)
    os.makedirs(args.save_dir)
    args.model_dir = os.path.join(args.save_dir, args.model_dir)
    os.mkdir(args.model_dir)
    args.log_file = os.path.join(args.save_dir, args.log_file)


def get_args(argv=None, make_dirs: bool = True):
    args = build_parser().parse_args(argv)
    check_image_pipeline(args)
    if make_dirs:
        make_experiment_dirs(args)
    resolve_device(args)
    return args


def default_args(**overrides):
    """Config object with every default, no directory side effects (for tests / bench / library use)."""
    args = build_parser().parse_args([])
    for k, v in overrides.items():
        if not hasattr(args, k):
            raise AttributeError(f"unknown config field {k}")
        setattr(args, k, v)
    if not isinstance(args.device, torch.device):
        resolve_device(args)
    return args
