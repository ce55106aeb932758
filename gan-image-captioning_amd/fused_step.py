"""The adversarial G+D train step as one direct kernel sequence (no autograd engine).

Same math and the same step order as ``GANInstructor._adv_step_autograd`` / SURVEY.md §8(c) -- body
of reference src/training.py:136-183 with both backward passes on pre-update weights, then both
optimizer steps -- but every buffer is allocated once per (batch, length) and gradients are written
straight into the flat arenas that the optimizer kernels and the RCCL all-reduce read.

Work that the reference executes and discards is skipped (results identical):
  * D's parameter gradients from g_loss (zeroed by the next zero_grad, training.py:195);
  * D(real) is evaluated on token ids (gather) rather than a dense one-hot (training.py:158), unless
    ``real_as_ids=0``;

The launches of the step are written once, as the pieces ``_d_real`` .. ``_d_bwd``: each takes the step's record (``_record``) and
enqueues on the current stream.  Two schedules run them: ``_call_eager`` on three streams behind events, with the phase markers and
the gradient reducer; ``_call_graph`` (opt-in) groups them into six captured sequences (``GRAPHS``) and replays those.
"""
from __future__ import annotations

import os
from typing import Dict

import torch

from . import engine
from .generator import SEEDS


class _Record(dict):
    """What the pieces of one step share, by attribute: the inputs, the parameter and gradient lists, and what one piece hands the next."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class FusedAdvStep:
    # The replayed step as LINEAR launch sequences, one per stretch between two cross-stream dependencies: each is captured as its own
    # hipGraph and replayed on its stream, with the events between them recorded / waited on eagerly.  (The whole step as ONE
    # multi-branch graph replays slower than eager launches on this runtime -- 3.49 against 2.67 ms per step, measured, round 3:
    # fork / join nodes inside a graph cost more than the stream events they replace -- while a linear graph replays at the
    # eager rate: the trunk pass has always been one.)
    GRAPHS = {"d_real": ("_d_prepare", "_d_real"),                     # s_real
              "rollout": ("_g_prepare", "_features", "_rollout"),      # main
              "d_fake": ("_d_fake", "_losses"),                        # main, behind D(real)
              "g_dgen": ("_g_dgen",),                                  # s_gen, behind the losses (reads D's weights)
              "g_bwd": ("_g_bwd",),                                    # s_gen
              "d_bwd": ("_d_bwd",)}                                    # main, behind the losses

    def __init__(self, gen, disc, gen_arena, disc_arena, args, reducer=None):
        self.gen, self.disc, self.args = gen, disc, args
        self.gen_arena, self.disc_arena = gen_arena, disc_arena
        self.reducer = reducer
        self.cgan = int(args.conditional_gan) == 1
        self.rsgan = args.adv_loss_type == "rsgan"       # utils.py:48: g_loss has no path to G
        # --disc-cond projection: every D pass also takes q = img_proj(pooled trunk features); w > 0 adds the mismatched-pair pass
        self.cond = getattr(disc, "cond", "none") == "projection"
        self.mismatch_w = float(getattr(args, "disc_mismatch_weight", 0.5)) if self.cond else 0.0
        self.attn = hasattr(gen.decoder, "attn")         # visual-attention decoder (cfg4): the roll-out also takes the trunk's feature map
        self.dec = gen.decoder.engine()
        self.den = disc.engine()
        self._buf: Dict[tuple, dict] = {}
        self._gen_grads = None
        self._disc_grads = None
        self.overlap = not os.environ.get("GIC_NO_STREAM_OVERLAP")
        self.trace = None
        # Replayed step graphs are opt-in.  LSTM step (GIC_STEP_GRAPH=1): at cfg2 (B=64, V=10000) the segments replayed on their three
        # streams left non-finite decoder gradients from the first replay on (the same kernels as eager launches give finite ones; the
        # replay test's cfg1 shapes do not show it), and eager launches measured 2.41 ms per step against 2.47 replayed.  (Observed at
        # cfg1 too, once the replayed step was compared bit for bit with an eager twin in the same process: sums added onto unzeroed
        # memory from the first pure replay on.  It went away when fill_zero, csrc/util.hip, captured kernel nodes for memset nodes; the
        # cause in the runtime is not identified, and whether this is cfg2's fault is not known: cfg2 has not been run again.)  Attention step
        # (GIC_STEP_GRAPH_ATTN=1): host enqueue 2.10 -> 0.43 ms per step, but 3.87 ms per step against 3.74 for eager launches at cfg4.
        want = os.environ.get("GIC_STEP_GRAPH_ATTN" if self.attn else "GIC_STEP_GRAPH")
        self.use_graph = bool(want) and not (os.environ.get("GIC_NO_STEP_GRAPH") or os.environ.get("GIC_NO_GRAPH"))
        if self.cond:
            self.use_graph = False               # the conditioned step is not captured: eager launches
        self._graphs: Dict[tuple, dict] = {}
        self._warm: set = set()

    # grads of the decoder parameters are views into the generator arena (order = Decoder.param_list())
    def _grad_lists(self):
        if self._gen_grads is None:
            by_param = {id(p): g for p, g in zip(self.gen_arena.params, self.gen_arena.grad_views())}
            self._gen_grads = [by_param[id(p)] for p in self.gen.decoder.param_list()]
            by_param = {id(p): g for p, g in zip(self.disc_arena.params, self.disc_arena.grad_views())}
            self._disc_grads = [by_param[id(p)] for p in self.disc.param_list()]
        return self._gen_grads, self._disc_grads

    def _buffers(self, B: int, L: int, dev) -> dict:
        key = (B, L)
        if key not in self._buf:
            dec, den = self.dec, self.den
            self._buf[key] = {
                "dec_state": dec.alloc_state(B, L, dev),
                "dec_ws": dec.alloc_bwd_ws(B, L, dev),
                "probs": torch.empty(B, L, dec.V, device=dev, dtype=dec.act),
                "ids": torch.empty(B, L, device=dev, dtype=torch.int64),
                "d_feat": torch.empty(B, dec.E, device=dev, dtype=torch.float32),
                "d_probs": torch.empty(B, L, dec.V, device=dev, dtype=dec.act),
                "st_rf": den.alloc_state(2 * B, L, dev),      # D(real) | D(fake) in the two halves: ONE backward over both
                "disc_ws": den.alloc_bwd_ws(2 * B, L, dev), "disc_ws_gen": den.alloc_bwd_ws(B, L, dev),
                "logits": torch.empty(3, B * den.R, device=dev, dtype=torch.float32),
                "ones": torch.ones(B, device=dev, dtype=torch.int64),
            }
            self._buf[key]["st_real"], self._buf[key]["st_fake"] = den.split_state(self._buf[key]["st_rf"])
            # D(gen) sees the same input as D(fake) (training.py:163-164): it shares everything up to the dropout draw
            self._buf[key]["st_gen"] = den.shared_state(self._buf[key]["st_fake"], B, L, dev)
            if self.cond:
                f32 = torch.float32
                self._buf[key]["logits"] = torch.empty(4, B * den.R, device=dev, dtype=f32)         # real, fake, gen, wrong
                self._buf[key]["q2"] = torch.empty(2 * B, den.F, device=dev, dtype=f32)             # [q; q] of the mixed real | fake batch
                self._buf[key]["d_q"] = torch.empty(3 * B, den.F, device=dev, dtype=f32)            # d_q of real | fake | wrong
                self._buf[key]["d_q_gen"] = torch.empty(B, den.F, device=dev, dtype=f32)
                if self.mismatch_w > 0.0:
                    self._buf[key]["st_wrong"] = den.alloc_state(B, L, dev)
                    self._buf[key]["disc_ws_wrong"] = den.alloc_bwd_ws(B, L, dev)
        return self._buf[key]

    def _early_bucket(self):
        """Arena span of decoder.linear's weight and bias (None if they are not adjacent in the arena)."""
        if not hasattr(self, "_early"):
            lin = self.gen.decoder.linear
            self._early = self.gen_arena.span([lin.weight, lin.bias])
        return self._early

    def _mark(self, name: str, stream) -> None:
        """Phase marker for tools/step_timeline.py (``self.trace`` is a list while tracing, else None)."""
        if self.trace is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream)
            self.trace.append((name, ev))

    def _streams(self, dev):
        if getattr(self, "_s_real", None) is None:
            self._s_real = torch.cuda.Stream(device=dev)     # D(real) forward: independent of the generator
            self._s_gen = torch.cuda.Stream(device=dev)      # the generator's path: D(gen) forward / backward, decoder backward
        return self._s_real, self._s_gen

    def __call__(self, images, captions, max_caption_len: int, train: bool = True, noise_u=None, keep_masks=None,
                 opt_step: bool = True, next_images=None, next_train=None) -> dict:
        """One step.  Returns device tensors: losses [g_loss, d_loss], ids, probs, logits (real, fake, gen).
        ``noise_u`` [L,B,V] / ``keep_masks`` (3 x [B*R,F]) make the step deterministic for parity runs.
        ``next_images``: the NEXT batch's images (same shape); its trunk forward is enqueued on a side stream under this
        step and picked up by the next call when it is passed the same tensor (results are identical either way).

        Independent branches of the step's dependency graph run on side HIP streams behind events:
          D(real) forward          || encoder head + roll-out         (and the NEXT batch's trunk forward under all of it)
          G path (D(gen) input-gradient, decoder / encoder-head backward)  ||  D path (backward real + fake, D's Adam)
        D's weights are not updated before the G path has finished reading them; both paths join before G's Adam.

        With GIC_STEP_GRAPH=1 (opt-in, see __init__), a training step with device-drawn noise is replayed as six linear hipGraphs from its
        third call on (``_call_graph``): everything behind the trunk features -- ~110 launches on three streams -- with the per-step
        scalars (temperature, noise seeds) read from device memory (engine.StepScalarsBuffer); GIC_NO_STEP_GRAPH=1 (or GIC_NO_GRAPH=1)
        keeps the eager launches either way.  Returned tensors
        of a replayed step live in the graphs' memory pools and are overwritten by the next step."""
        B, L = captions.shape[0], int(max_caption_len)
        if self.mismatch_w > 0.0 and B < 2:
            raise ValueError("--disc-mismatch-weight > 0 needs at least two captions per batch: the wrong pair is the next image of the batch")
        engine.require_gpu(captions, images)
        dev = captions.device
        main = torch.cuda.current_stream(dev)
        if (self.use_graph and train and opt_step and noise_u is None and keep_masks is None and self.reducer is None and self.overlap
                and self.trace is None):
            return self._call_graph(images, captions, B, L, main, next_images, next_train)
        # seeds in the order real, fake, gen, roll-out (the slots of a replayed step's device scalars), then the mismatched pass
        km = keep_masks if keep_masks is not None else (None, None, None)
        seeds = [0 if km[i] is not None else SEEDS.next() for i in range(3)]
        seeds.append(0 if noise_u is not None else SEEDS.next())
        if self.mismatch_w > 0.0:                # the mismatched-pair pass: a fourth keep mask / dropout seed
            km = tuple(km) + (None,) * (4 - len(km))
            seeds.append(0 if km[3] is not None else SEEDS.next())
        ev_start = main.record_event()
        self._mark("start", main)
        c = self._record(self._buffers(B, L, dev), captions, float(self.gen.decoder.temperature), train, noise_u, km, seeds, None)
        return self._call_eager(c, images, opt_step, main, ev_start, next_images, next_train)

    def _record(self, buf, caps, T, train, noise_u, km, seeds, scal) -> _Record:
        """``scal``: StepScalarsBuffer (a replayed step: temperature and seeds are read from device memory, ``T`` and ``seeds`` are
        zeros) or None (by value)."""
        c = _Record(buf=buf, caps=caps, T=T, train=bool(train), noise_u=noise_u, km=km, seeds=seeds, scal=scal,
                    trunk_feats=None, fmap=None, q=None)
        c.gparams = [p.detach() for p in self.gen.decoder.param_list()]
        c.dparams = [p.detach() for p in self.disc.param_list()]
        c.g_grads, c.d_grads = self._grad_lists()
        if self.cond:                    # the engine's parameters first, img_proj behind them (Discriminator.param_list)
            n_text = self.den.nparams()
            c.proj, c.proj_grads = c.dparams[n_text:], c.d_grads[n_text:]
            c.dparams, c.d_grads = c.dparams[:n_text], c.d_grads[:n_text]
        return c

    # ---- trunk look-ahead (Encoder.prefetch_trunk / take_trunk): the ResNet trunk is frozen (generator.py:21), so the trunk forward
    # of batch k+1 depends on nothing that step k updates; it runs on its own stream under this step's launch-bound phases.
    def _take_and_prefetch(self, images, train, main, ev_start, next_images, next_train):
        """This step's trunk features and feature map [B, P, C] (None without attention): the look-ahead pass of the previous step,
        or a pass now; then the NEXT batch's pass on its stream."""
        enc = self.gen.encoder
        feats, fmap = enc.take_trunk_with_map(images, train, main) if self.attn else (enc.take_trunk(images, train, main), None)
        if next_images is not None:          # the prefetched output is a private copy: the next trunk pass may start now
            enc.prefetch_trunk(next_images, train if next_train is None else next_train, ev_start, mark=self._mark, want_map=self.attn)
        return feats, (fmap.view(fmap.shape[0], -1, fmap.shape[-1]) if self.attn else None)

    # ---------------------------------------------------------------- the launches of the step, each on the current stream
    def _d_prepare(self, c):              # compute-dtype weight images: refreshed when the weights have changed
        self.den.prepare(c.dparams)

    def _g_prepare(self, c):
        self.dec.prepare(c.gparams)

    def _d_real(self, c):
        """D(real) (training.py:162)."""
        if int(getattr(self.args, "real_as_ids", 1)):
            c.real_soft, c.real_ids = None, c.caps
        else:
            c.real_soft, c.real_ids = self.den.soft_input(torch.nn.functional.one_hot(c.caps, self.den.V).float()), None
        self.den.fwd(c.dparams, c.real_soft, c.real_ids, c.train, c.km[0], c.seeds[0], state=c.buf["st_real"], logits=c.buf["logits"][0],
                     dev_scalars=c.scal, seed_slot=0)

    def _features(self, c):
        """training.py:144-147: the encoder head on the trunk features, or embed(<S>) broadcast."""
        if self.cgan:
            c.feats = self.gen.encoder.forward_fused(None, c.train, trunk_feats=c.trunk_feats)
        else:
            c.feats = engine.embedding_fwd(c.gparams[0], c.buf["ones"])

    def _rollout(self, c):
        """One roll-out (training.py:150).  (Measured: issuing it from a high-priority stream does not win it CU slots from the
        look-ahead trunk pass -- it finished only after the whole trunk pass -- so it stays on the main stream.)"""
        maps = (c.fmap,) if self.attn else ()
        c.probs, c.ids, c.dst = self.dec.sample_fwd(c.gparams, c.feats, *maps, c.caps.shape[1], c.T, False, c.noise_u, c.seeds[3],
                                                    state=c.buf["dec_state"], out=c.buf["probs"], ids=c.buf["ids"], dev_scalars=c.scal,
                                                    seed_slot=3)

    def _d_fake(self, c):
        """D(fake), D(gen) (training.py:163-164): one pass up to the highway layer, two dropout draws + heads."""
        buf, lg = c.buf, c.buf["logits"]
        if self.cond:                            # q = img_proj(pooled trunk features), detached: the step already owns them
            c.q, c.pooled = self.den.img_proj_fwd(*c.proj, c.trunk_feats)
        self.den.fwd(c.dparams, c.probs, None, c.train, c.km[1], c.seeds[1], state=buf["st_fake"], logits=lg[1], dev_scalars=c.scal,
                     seed_slot=1, cond=c.q)
        self.den.fwd_redrop(c.dparams, buf["st_fake"], buf["st_gen"], c.train, c.km[2], c.seeds[2], logits=lg[2], dev_scalars=c.scal,
                            seed_slot=2, cond=c.q)

    def _losses(self, c):
        a, buf, lg = self.args, c.buf, c.buf["logits"]
        if self.cond:                            # D(real)'s text path ran on its stream before the features existed: its match term now
            self.den.match_logits(buf["st_real"], c.q, logits=lg[0], accumulate=True)
        c.losses, c.lgrads = engine.gan_losses(a.adv_loss_type, lg[0], lg[1], lg[2], want_grads=c.train)
        c.lgrads_w = None
        if self.mismatch_w > 0.0:
            # mismatched pairs: the real captions against the batch's images rolled by one -- a third D pass with its own state and
            # dropout draw; d_loss = (1 - w) d(real, fake) + w d(real, wrong), g_loss as it was
            c.q_wrong = torch.roll(c.q, -1, 0)
            self.den.fwd(c.dparams, c.real_soft, c.real_ids, c.train, c.km[3], c.seeds[4], state=buf["st_wrong"], logits=lg[3], cond=c.q_wrong)
            losses_w, c.lgrads_w = engine.gan_losses(a.adv_loss_type, lg[0], lg[3], lg[2], want_grads=c.train)
            engine.gan_losses_mismatch(self.mismatch_w, c.losses, c.lgrads, losses_w, c.lgrads_w)

    def _g_dgen(self, c):
        """g_loss -> D(gen) input gradient: the last reader of D's weights on the G path."""
        if self.rsgan:
            self.gen_arena.grad.zero_()
        else:
            self.den.bwd(c.dparams, c.buf["st_gen"], c.probs, None, c.train, c.lgrads["dg_out"], False, True, ws=c.buf["disc_ws_gen"],
                         d_inp=c.buf["d_probs"], cond=c.q, d_q=c.buf.get("d_q_gen"))

    def _g_bwd(self, c, early=None):
        """Decoder BPTT + weight gradients, then the encoder head (training.py:169 minus the step).  ``early`` (data parallel, LSTM
        decoder): the vocabulary projection's span of G's arena (40 % of it) is complete before BPTT starts; its all-reduce runs
        under BPTT and the weight-gradient products instead of after them."""
        if self.rsgan:
            return

        def dec_bwd(**phases):
            self.dec.sample_bwd(c.gparams, c.dst, c.probs, c.ids, c.buf["d_probs"], c.T, False, ws=c.buf["dec_ws"],
                                grads=c.g_grads + [c.buf["d_feat"]], dev_scalars=c.scal, **phases)
        if early is None:
            dec_bwd()
        else:
            dec_bwd(phases=1)
            self.reducer.start(self.gen_arena.grad[early[0]:early[1]])
            dec_bwd(phases=2)
        if self.cgan:
            self.gen.encoder.backward_fused(c.buf["d_feat"])
        else:   # features = embed(<S>) broadcast: fold d_features into row 1 of the embedding gradient
            engine.embedding_bwd(c.buf["d_feat"], c.buf["ones"], self.dec.V, d_weight=c.g_grads[0], zero_first=False)

    def _d_bwd(self, c):
        """d_loss -> D parameters (training.py:168)."""
        buf, B = c.buf, c.caps.shape[0]
        self.disc_arena.grad.zero_()          # ONE fill; every pass accumulates (instead of a fill per small gradient tensor)
        into = dict(grads=c.d_grads, accumulate=True)
        if c.real_ids is None:                  # --real-as-ids 0: two dense passes
            half_ws = {k: v[:v.shape[0] // 2] for k, v in buf["disc_ws"].items()}
            for st, inp, d_logits in ((buf["st_real"], c.real_soft, c.lgrads["dd_real"]), (buf["st_fake"], c.probs, c.lgrads["dd_fake"])):
                self.den.bwd(c.dparams, st, inp, None, c.train, d_logits, True, False, ws=half_ws, **into)
            return
        # real (ids) and fake (soft) passes differentiated as one batch of 2B captions; the conditioned D (real ids only,
        # check_disc_cond) with [q; q], and d_q of its passes in one buffer: real | fake | wrong
        q2, d_q = (torch.cat([c.q, c.q], 0, out=buf["q2"]), buf["d_q"][:2 * B]) if self.cond else (None, None)
        self.den.bwd(c.dparams, buf["st_rf"], c.probs, c.real_ids, c.train, c.lgrads["dd_real_fake"], True, False, ws=buf["disc_ws"],
                     cond=q2, d_q=d_q, **into)
        if self.cond:                           # the wrong pass's own backward; d img_proj = d_q^T pooled over [pooled; pooled; rolled pooled]
            pooled = [c.pooled, c.pooled]
            if c.lgrads_w is not None:
                d_q = buf["d_q"]
                self.den.bwd(c.dparams, buf["st_wrong"], c.real_soft, c.real_ids, c.train, c.lgrads_w["dd_fake"], True, False,
                             ws=buf["disc_ws_wrong"], cond=c.q_wrong, d_q=d_q[2 * B:], **into)
                pooled.append(torch.roll(c.pooled, -1, 0))
            self.den.img_proj_bwd(d_q, torch.cat(pooled, 0), *c.proj_grads, accumulate=True)

    @staticmethod
    def _out(c) -> dict:
        return {"losses": c.losses, "ids": c.ids, "probs": c.probs, "logits": c.buf["logits"]}

    # ---------------------------------------------------------------- the step as eager launches on three streams
    def _call_eager(self, c, images, opt_step, main, ev_start, next_images, next_train) -> dict:
        red, mark = self.reducer, self._mark
        s_real, s_gen = self._streams(c.caps.device) if self.overlap else (main, main)
        with engine.on_stream(s_gen):            # the weight images are refreshed on the side streams, under the encoder
            s_gen.wait_event(ev_start)
            self._g_prepare(c)
            ev_gprep = s_gen.record_event()
        with engine.on_stream(s_real):           # D(real), concurrently with the generator's forward
            s_real.wait_event(ev_start)
            self._d_prepare(c)
            ev_dprep = s_real.record_event()
            self._d_real(c)
            ev_real = s_real.record_event()
            mark("D(real) fwd done [s_real]", s_real)
        if self.cgan:                            # the hand-over comes after D(real) and the weight images are under way
            c.trunk_feats, c.fmap = self._take_and_prefetch(images, c.train, main, ev_start, next_images, next_train)
        self._features(c)
        mark("encoder done", main)
        main.wait_event(ev_gprep)
        self._rollout(c)
        mark("roll-out done", main)
        main.wait_event(ev_dprep)
        self._d_fake(c)
        mark("D(fake), D(gen) fwd done", main)
        main.wait_event(ev_real)
        self._losses(c)
        out = self._out(c)
        if not c.train:
            return out
        ev_loss = main.record_event()
        mark("losses done", main)
        early = self._early_bucket() if (red is not None and not self.rsgan and not self.attn) else None
        with engine.on_stream(s_gen):            # the G path on its stream
            s_gen.wait_event(ev_loss)
            if self.overlap:
                c.lgrads["dg_out"].record_stream(s_gen)
            if self.cond and not self.rsgan:
                c.q.record_stream(s_gen)
            self._g_dgen(c)
            ev_dgen = s_gen.record_event()       # D's weights are free to change from here on
            if not self.rsgan:
                mark("D(gen) input-grad done [s_gen]", s_gen)
            self._g_bwd(c, early)
            ev_g = s_gen.record_event()
            mark("G path done [s_gen]", s_gen)
        self._d_bwd(c)                           # the D path on the main stream
        if red is not None:
            # collectives run one after the other on the reducer's stream, in the order they become ready:
            # G's early bucket (_g_bwd), D's arena (now), the rest of G's arena (when the G path is through)
            ev_dred = red.start(self.disc_arena.grad)
            numel = self.gen_arena.numel
            with engine.on_stream(s_gen):
                for lo, hi in ((0, numel),) if early is None else ((0, early[0]), (early[1], numel)):
                    if lo < hi:
                        red.start(self.gen_arena.grad[lo:hi])
        mark("D path done", main)
        main.wait_event(ev_dgen)                 # D's weights are no longer read by the G path
        if red is not None:
            red.wait(ev_dred)
        if opt_step:
            self.disc_opt.step()                 # D's clip + Adam runs under the rest of the G path
        main.wait_event(ev_g)
        if red is not None:
            red.wait_all()
        if opt_step:
            self.gen_opt.step()
        mark("optimizers done", main)
        return out

    # ---------------------------------------------------------------- the step as replayed hipGraphs
    def _graph_key(self, B: int, L: int) -> tuple:
        a = self.args
        return (B, L, engine.deterministic(), self.cgan, a.adv_loss_type, int(getattr(a, "real_as_ids", 1)), self.gen_arena.flat.data_ptr(), self.disc_arena.flat.data_ptr(),
                id(self.gen_opt), id(self.disc_opt), self.gen_opt.lr, self.gen_opt.clip_norm, self.disc_opt.lr, self.disc_opt.clip_norm,
                self.den.drop_p, bool(self.gen.training), bool(self.disc.training))

    def _call_graph(self, images, captions, B: int, L: int, main, next_images, next_train) -> dict:
        """Call 1 with a given key runs the sequences of ``GRAPHS`` eagerly (lazy code-object loads, LDS grants and buffer allocation
        are not capturable), call 2 captures each of them as it goes, later calls replay them.  Outside the graphs: the trunk look-ahead
        hand-over (its own replayed graph on its own stream), the copies of this batch's captions / trunk features into the step's
        static input buffers, the one-thread launch that writes temperature and seeds into device memory, the stream events and the
        optimizer steps (two launches each)."""
        dev = captions.device
        buf = self._buffers(B, L, dev)
        if "caps_in" not in buf:
            buf["caps_in"] = torch.empty(B, L, device=dev, dtype=torch.int64)
            buf["scal"] = engine.StepScalarsBuffer(dev)
            if self.cgan:
                buf["trunk_in"] = torch.empty(B, self.gen.encoder.resnet.out_features, device=dev, dtype=self.dec.act)
            if self.attn:
                buf["fmap_in"] = torch.empty(B, self.dec.P, self.dec.C, device=dev, dtype=self.dec.act)
        key = self._graph_key(B, L)
        g = self._graphs.get(key)
        if g is None:
            mode = "capture" if key in self._warm else "eager"
            self._warm.add(key)
            if mode == "capture":
                self._graphs.clear()             # at most one live set of step graphs (stale pointers never replay); dies here, outside capture
                self.dec._shadow_key = self.den._shadow_key = None      # the weight-image refresh is part of every replay
            c = self._record(buf, buf["caps_in"], 0.0, True, None, (None,) * 3, (0,) * 4, buf["scal"])
            c.trunk_feats, c.fmap = buf.get("trunk_in"), buf.get("fmap_in")
            g = {"ctx": c, "graphs": {}, "mode": mode}
            if mode == "capture":
                self._graphs[key] = g
        c = g["ctx"]
        s_real, s_gen = self._streams(dev)

        def run(name):
            """One sequence on the current stream: replay, or capture-then-replay, or eager."""
            gr = g["graphs"].get(name)
            if gr is None:
                pieces = [getattr(self, p) for p in self.GRAPHS[name]]
                if g["mode"] != "capture":
                    for piece in pieces:
                        piece(c)
                    return
                gr = torch.cuda.CUDAGraph()
                with engine.capture_guard(), torch.cuda.graph(gr, capture_error_mode="thread_local"):
                    for piece in pieces:
                        piece(c)
                g["graphs"][name] = gr
            gr.replay()

        try:
            buf["caps_in"].copy_(captions)
            buf["scal"].set(float(self.gen.decoder.temperature), [SEEDS.next() for _ in range(4)])
            ev_start = main.record_event()
            with engine.on_stream(s_real):
                s_real.wait_event(ev_start)
                run("d_real")
                ev_real = s_real.record_event()
            if self.cgan:
                feats, fmap = self._take_and_prefetch(images, True, main, ev_start, next_images, next_train)
                if self.attn:
                    buf["fmap_in"].copy_(fmap)
                buf["trunk_in"].copy_(feats)
            run("rollout")
            main.wait_event(ev_real)
            run("d_fake")
            ev_loss = main.record_event()
            with engine.on_stream(s_gen):
                s_gen.wait_event(ev_loss)
                run("g_dgen")
                ev_dgen = s_gen.record_event()       # D's weights are free to change from here on
                run("g_bwd")
                ev_g = s_gen.record_event()
            run("d_bwd")
            main.wait_event(ev_dgen)
            self.disc_opt.step()                     # D's clip + Adam runs under the rest of the G path
            main.wait_event(ev_g)
            self.gen_opt.step()
        except Exception as exc:
            if g["mode"] != "capture":
                raise
            import warnings                          # capture refused: eager launches from here on (same kernels, same results)
            warnings.warn(f"hipGraph capture of the train step failed ({exc}); falling back to eager launches")
            self.use_graph = False
            self._graphs.clear()
            torch.cuda.synchronize()
            self.dec._shadow_key = self.den._shadow_key = None
            return self(images, captions, L, True, next_images=next_images, next_train=next_train)
        g["mode"] = "replay" if g["mode"] == "capture" else g["mode"]
        return self._out(c)

    def bind_optimizers(self, gen_opt, disc_opt) -> "FusedAdvStep":
        self.gen_opt, self.disc_opt = gen_opt, disc_opt
        return self
