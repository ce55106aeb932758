"""Shared helpers of the GPU parity tests (oracle <-> HIP library)."""
import torch

from oracle import cpu_step as O
from tests.disc_cases import SENTINEL

U8_SENTINEL = 0xA5


class Guarded:
    """[rows, ld] with sentinel guard rows on either side (whole 16-byte multiples, so the live part keeps the allocation's
    alignment); `off`: the live part starts that many elements later (a deliberately misaligned view)."""

    def __init__(self, rows, ld, dtype, dev, fill, off=0):
        esz = torch.empty((), dtype=dtype).element_size()
        g = 1
        while (g * ld * esz) % 16:
            g += 1
        self.sent = U8_SENTINEL if dtype == torch.uint8 else SENTINEL
        self.flat = torch.full(((rows + 2 * g) * ld + off,), self.sent, dtype=dtype, device=dev)
        self.lo = g * ld + off
        self.live = self.flat[self.lo:self.lo + rows * ld].view(rows, ld) if ld > 1 else self.flat[self.lo:self.lo + rows]
        self.live.fill_(fill)

    def guards_intact(self):
        n = self.live.numel()
        outside = torch.cat([self.flat[:self.lo], self.flat[self.lo + n:]])
        return bool((outside == self.sent).all())


def dec_param_names(nl):
    names = ["decoder.embed.weight"]
    for l in range(nl):
        names += [f"decoder.lstm.weight_ih_l{l}", f"decoder.lstm.weight_hh_l{l}",
                  f"decoder.lstm.bias_ih_l{l}", f"decoder.lstm.bias_hh_l{l}"]
    return names + ["decoder.linear.weight", "decoder.linear.bias"]


def disc_param_names(nconv):
    names = ["embeddings.weight"]
    for k in range(nconv):
        names += [f"convs.{k}.weight", f"convs.{k}.bias"]
    return names + ["highway.weight", "highway.bias", "feature2out.weight", "feature2out.bias",
                    "out2logits.weight", "out2logits.bias"]


def dec_params(gp, dev):
    nl = O.num_lstm_layers(gp)
    return [gp[n].to(dev).contiguous() for n in dec_param_names(nl)]


def disc_params(dp, dev):
    return [dp[n].to(dev).contiguous() for n in disc_param_names(O.disc_num_convs(dp))]


def close(got, want, rtol, atol_scale=1e-5, what="", atol_abs=1e-30):
    """assert_close with an absolute floor relative to the reference tensor's largest entry."""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    scale = float(want.abs().max()) if want.numel() else 0.0
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol_scale * scale + atol_abs, msg=lambda s: f"{what}: {s}")


def close_mostly(got, want, rtol, atol_scale, what, max_outlier_frac=5e-3, max_rel_l2=2e-3):
    """For tensors downstream of a discontinuous op (max-over-time argmax, relu gate): a near-tie
    resolved differently in fp32 re-routes one contribution, so allow a small fraction of entries
    outside the element-wise tolerance while bounding the relative L2 error of the whole tensor."""
    g = got.detach().double().cpu()
    w = want.detach().double().cpu()
    scale = float(w.abs().max()) if w.numel() else 0.0
    bad = (g - w).abs() > (atol_scale * scale + rtol * w.abs())
    frac = float(bad.double().mean()) if w.numel() else 0.0
    err = rel_l2(g, w)
    assert frac <= max_outlier_frac and err <= max_rel_l2, f"{what}: {frac:.2%} entries out of tolerance, rel L2 {err:.2e}"
    return frac, err


def rel_l2(got, want):
    got = got.detach().double().cpu().reshape(-1)
    want = want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / (want.norm() + 1e-30))
