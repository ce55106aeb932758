"""The image-conditioned discriminator (--disc-cond projection, csrc/disc_cond.hip) on the CPU: there is no reference counterpart, the
oracle is this build's own PyTorch (fp64 where a test asks for it).  Nothing here touches the GPU.

  q = img_proj(pooled)                       [B, F], pooled = the frozen trunk's pooled features, detached
  logits[m] = base[m] + s sum_n y[m, n] q[b, n]     m = b R + r, s = F^-1/2, y = the dropped highway output feature2out consumes
  d_loss = (1 - w) d(real, fake) + w d(real, wrong)     wrong = the real captions against q[(b + 1) mod B]

`match_stage_*` are the element-wise stage checks in the manner of tests/disc_cases.py: fp64 references formed from the buffers the
kernels wrote upstream, bounds per element with u = 2^-24, none fitted."""
import torch

from oracle import cpu_step as O
from tests import disc_cases as D

LOSS_TYPES = ("standard", "JS", "KL", "hinge", "tv", "rsgan")


def scale(F):
    return float(F) ** -0.5


def roll(t):
    """Row b takes row (b + 1) mod B: the batch's images rolled by one."""
    return torch.roll(t, -1, 0)


def match_term(y, q, R):
    """s <y[m, :], q[m // R, :]> for y [B*R, F], q [B, F]."""
    B, F = q.shape
    return scale(F) * (y.view(B, R, F) * q[:, None, :]).sum(-1).reshape(-1)


def match_backward(y, q, g, R):
    """The hand-written gradients of the match term: (d_y [B*R, F], d_q [B, F]) for d_logits g [B*R]."""
    B, F = q.shape
    s = scale(F)
    d_y = s * g.view(B, R, 1) * q[:, None, :]
    d_q = s * (g.view(B, R, 1) * y.view(B, R, F)).sum(1)
    return d_y.reshape(B * R, F), d_q


def img_proj_backward(d_q, pooled):
    return d_q.t() @ pooled, d_q.sum(0)


def disc_forward(dp, inp, pooled, keep_mask, R, dropout_p=O.DROPOUT_P, q=None):
    """The conditioned Discriminator.forward: dp carries img_proj.weight / .bias; q overrides img_proj(pooled)."""
    base, st = O.disc_forward(dp, inp, keep_mask, R, return_stages=True, dropout_p=dropout_p)
    y = st["highway"] if keep_mask is None else st["highway"] * (keep_mask / (1.0 - dropout_p))
    if q is None:
        q = pooled.detach() @ dp["img_proj.weight"].t() + dp["img_proj.bias"]
    return base + match_term(y, q, R)


def d_loss_mix(d_real, d_fake, d_wrong, g_out, loss_type, w):
    g_loss, d1 = O.get_losses(d_real, d_fake, g_out, loss_type)
    if w <= 0.0:
        return g_loss, d1
    _, d2 = O.get_losses(d_real, d_wrong, g_out, loss_type)
    return g_loss, (1.0 - w) * d1 + w * d2


def d_loss_mix_grads(d_real, d_fake, d_wrong, g_out, loss_type, w):
    """The hand-written mix of gic_gan_losses_mismatch from two plain evaluations' gradients: (d_loss, dd_real, dd_fake, dd_wrong)."""
    def one(a, b):
        a, b = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        _, d = O.get_losses(a, b, g_out.detach(), loss_type)
        ga, gb = torch.autograd.grad(d, [a, b], allow_unused=True)
        z = torch.zeros_like(a)
        return d.detach(), (ga if ga is not None else z), (gb if gb is not None else z)
    la, ra, fa = one(d_real, d_fake)
    lb, rb, fb = one(d_real, d_wrong)
    return (1 - w) * la + w * lb, (1 - w) * ra + w * rb, (1 - w) * fa, w * fb


def adv_step(gp, dp, captions, us, masks, temperature, loss_type, trunk_feat, R, w, clip_norm=5.0, gen_opt=None, disc_opt=None,
             fmap=None, sample=None):
    """oracle.cpu_step.adv_step with the conditioned D and the mismatched-pair pass: masks = (real, fake, gen, wrong).  ``sample``: a
    callable (g_leaf, feats) -> (gen, ids) for another decoder (the attention decoder's oracle), default the LSTM roll-out."""
    bsz, seqlen = captions.shape
    vocab = dp["embeddings.weight"].shape[1]
    g_leaf = {k: v.detach().clone().requires_grad_(True) for k, v in gp.items()}
    d_leaf = {k: v.detach().clone().requires_grad_(True) for k, v in dp.items()}
    feats = O.encoder_head(g_leaf, trunk_feat, training=True)
    gen, ids = sample(g_leaf, feats) if sample is not None else O.decoder_sample(g_leaf, feats, seqlen, temperature, us)
    real = torch.nn.functional.one_hot(captions, vocab).to(gen.dtype)
    pooled = trunk_feat.detach()
    d_real = disc_forward(d_leaf, real, pooled, masks[0], R)
    d_fake = disc_forward(d_leaf, gen.detach(), pooled, masks[1], R)
    g_out = disc_forward(d_leaf, gen, pooled, masks[2], R)
    d_wrong = disc_forward(d_leaf, real, roll(pooled), masks[3], R) if w > 0.0 else None
    g_loss, d_loss = d_loss_mix(d_real, d_fake, d_wrong, g_out, loss_type, w)
    out = {"ids": ids, "g_loss": float(g_loss.detach()), "d_loss": float(d_loss.detach()), "d_real": d_real.detach(), "d_fake": d_fake.detach(),
           "g_out": g_out.detach(), "d_wrong": None if d_wrong is None else d_wrong.detach()}
    d_grads = dict(zip(d_leaf, torch.autograd.grad(d_loss, list(d_leaf.values()), retain_graph=True)))
    g_grads_t = torch.autograd.grad(g_loss, list(g_leaf.values()), allow_unused=True)
    g_grads = {k: g for k, g in zip(g_leaf, g_grads_t) if g is not None}
    out["d_grads_raw"], out["g_grads_raw"] = d_grads, g_grads
    d_grads, _ = O.clip_grad_norm(d_grads, clip_norm)
    g_grads, _ = O.clip_grad_norm(g_grads, clip_norm)
    if disc_opt is not None:
        disc_opt.step(dp, d_grads)
    if gen_opt is not None:
        gen_opt.step(gp, g_grads)
    return out


def evaluate_match(dp, batches, R):
    """{"pair_acc", "margin"} over batches of (pooled [B, C], captions [B, L]) in eval mode: ties are not wins."""
    V = dp["embeddings.weight"].shape[1]
    wins, total, n = 0, 0.0, 0
    for pooled, caps in batches:
        _, st = O.disc_forward(dp, torch.nn.functional.one_hot(caps, V).to(pooled.dtype), None, R, return_stages=True)
        q = pooled @ dp["img_proj.weight"].t() + dp["img_proj.bias"]
        own = match_term(st["highway"], q, R).view(-1, R).mean(1)
        other = match_term(st["highway"], roll(q), R).view(-1, R).mean(1)
        diff = own - other
        wins += int((diff > 0).sum())
        total += float(diff.double().sum())
        n += caps.shape[0]
    return {"pair_acc": wins / n, "margin": total / n}


# ------------------------------------------------------------------------------------------------ element-wise stage checks
def check_match_forward(case, P, buf, q, logits, rep):
    """logits = feat . w + b + s <ydrop, q> against the buffers upstream (feat, ydrop): (F + OUT + 4) u (sum |feat w| + |b| + s sum |y q|)."""
    F, R = case.F, case.R
    f, w, b = buf["feat"].double(), P[-2].double().reshape(-1), P[-1].double()
    y, qd = buf["ydrop"][:, :F].double(), q.double()
    ref = f @ w + b + match_term(y, qd, R)
    mag = f.abs() @ w.abs() + b.abs() + match_term(y.abs(), qd.abs(), R)
    rep.check("match logits", logits, ref, (F + D.OUT + 4) * D.U * mag)


def check_match_only(case, buf, q, term, rep):
    F, R = case.F, case.R
    y, qd = buf["ydrop"][:, :F].double(), q.double()
    rep.check("match term", term, match_term(y, qd, R), (F + 4) * D.U * match_term(y.abs(), qd.abs(), R))


def check_match_backward(case, img, st, ws, q, g, d_q, rep, det=False):
    """dydrop = dfeat W_f2o + s g q  ((OUT_PAD + 5) u (|dfeat| |W| + s |g q|)), pad columns exactly zero; d_q ((R + 4) u s sum_r |g y|).
    det: `dydrop` was scratch afterwards (deterministic mode), only d_q is checked."""
    F, R = case.F, case.R
    s = scale(F)
    gd, qd = g.double(), q.double()
    y = st["ydrop"][:, :F].double()
    d_y, d_q_ref = match_backward(y, qd, gd, R)
    if not det:
        dfe, W = ws["dfeat"].double(), img["f2o_w"].double()
        ref = dfe @ W
        ref[:, :F] += d_y
        mag = dfe.abs() @ W.abs()
        mag[:, :F] += d_y.abs()
        rep.check("cond dydrop", ws["dydrop"][:, :F], ref[:, :F], (D.OUT_PAD + 5) * D.U * mag[:, :F])
        if case.Fp > F:
            rep.exact("cond dydrop pad", ws["dydrop"][:, F:] == 0, "of the pad columns are not zero")
    _, mag_q = match_backward(y.abs(), qd.abs(), gd.abs(), R)
    rep.check("d_q", d_q, d_q_ref, (R + 4) * D.U * mag_q)
    return s
