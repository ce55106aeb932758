"""The masked, label-smoothed sequence loss without a GPU: the symbol is declared, bound and exported; every argument error of gic_xent_seq
returns its status with a message that names the argument, before any launch; the three flags and their checks; and the self-test of the
oracle the GPU tests compare with (tests/xent_seq_oracle.py) against F.cross_entropy in float64."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd.args import default_args
from tests import xent_seq_oracle as XO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [0x10000 * (i + 1) for i in range(16)]          # distinct non-null addresses, never dereferenced: the checks come first


def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gicap.h")).read(), flags=re.S)
    assert re.search(r"\bgic_xent_seq\s*\(", text)
    assert "gic_xent_seq" in L.EXPORTED_SYMBOLS
    lib = L.load()
    assert hasattr(lib, "gic_xent_seq") and lib.gic_abi_version() == L.ABI_VERSION == 5


def _args(**kw):
    a = dict(logits=FAKE[0], dtype=L.F32, rows=6, V=50, targets=FAKE[1], group=3, lengths=FAKE[2], ignore=-100, eps=0.1, w=FAKE[3], loss=FAKE[4],
             row_nll=FAKE[5], row_ws=FAKE[6], cap_nll=FAKE[7], cap_tokens=FAKE[8], dl=FAKE[9])
    a.update(kw)
    return [a[k] for k in ("logits", "dtype", "rows", "V", "targets", "group", "lengths", "ignore", "eps", "w", "loss", "row_nll", "row_ws",
                           "cap_nll", "cap_tokens", "dl")] + [None]


def _refused(status, *words, code=-1):
    assert status == code
    msg = L.load().gic_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_argument_checks():
    f = L.load().gic_xent_seq
    _refused(f(*_args(logits=None)), "logits")
    _refused(f(*_args(targets=None)), "targets")
    _refused(f(*_args(loss=None)), "loss")
    _refused(f(*_args(row_nll=None)), "row_nll")
    _refused(f(*_args(row_ws=None)), "row_ws")
    for rows in (0, -3):
        _refused(f(*_args(rows=rows)), f"rows={rows}")
    _refused(f(*_args(rows=1 << 24, group=1)), f"rows={1 << 24}", "2^24")      # a 256-thread workgroup per row: the grid's thread limit
    for V in (0, -1):
        _refused(f(*_args(V=V)), f"V={V}")
    for group in (0, -2):
        _refused(f(*_args(group=group)), f"group={group}")
    _refused(f(*_args(group=4)), "group=4", "rows=6")
    for eps in (1.0, -0.1, 1.5, float("nan")):
        _refused(f(*_args(eps=eps)), "smoothing")
    _refused(f(*_args(dtype=7)), "dtype 7", code=L.ERR_UNSUPPORTED)


def test_engine_checks_come_before_the_device():
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd._lib import GicError
    p = inspect.signature(engine.xent_seq).parameters
    assert list(p) == ["logits", "targets", "group", "lengths", "ignore_index", "smoothing", "row_weight", "want_grad"]
    assert (p["lengths"].default, p["ignore_index"].default, p["smoothing"].default, p["row_weight"].default, p["want_grad"].default) == \
        (None, -100, 0.0, None, True)
    with pytest.raises(GicError):
        engine.xent_seq(torch.zeros(6, 5), torch.zeros(6, dtype=torch.long), 3)


def test_flags_exist_with_their_defaults():
    a = default_args()
    assert (a.pretrain_ignore_pad, a.label_smoothing, a.eval_perplexity) == (0, 0.0, 0)


@pytest.mark.parametrize("eps", [1.0, -0.1, float("nan")])
def test_label_smoothing_outside_the_range_is_refused_at_construction(eps):
    from gan_image_captioning_amd.training import GANInstructor, check_seq_loss
    with pytest.raises(ValueError, match="--label-smoothing"):
        GANInstructor(default_args(vocab_size=50, label_smoothing=eps, device="cpu"), None, None)
    assert check_seq_loss(default_args(label_smoothing=0.1, pretrain_ignore_pad=1)) == (True, 0.1)


def test_module_signatures():
    from gan_image_captioning_amd.generator import AttnDecoder, Decoder, Generator
    from gan_image_captioning_amd.training import GANInstructor
    assert list(inspect.signature(Decoder.log_likelihood).parameters) == ["self", "features", "ids", "lengths"]
    assert list(inspect.signature(AttnDecoder.log_likelihood).parameters) == ["self", "features", "fmap", "ids", "lengths"]
    assert list(inspect.signature(Generator.score_captions).parameters) == ["self", "images", "ids", "lengths"]
    assert inspect.signature(GANInstructor.evaluate_perplexity).parameters["what"].default == "val"


def test_oracle_is_cross_entropy_with_ignore_index_and_label_smoothing():
    g = torch.Generator().manual_seed(5)
    B, Lc, V = 3, 5, 17
    x = torch.randn(B * Lc, V, generator=g, dtype=torch.float64, requires_grad=True)
    t = torch.randint(0, V, (B * Lc,), generator=g)
    t[[1, 4, 9, 14]] = 0                                  # some <PAD> = 0 targets
    for eps in (0.0, 0.1):
        for ignore in (0, -100):
            ref = F.cross_entropy(x, t, ignore_index=ignore, label_smoothing=eps)
            (grad,) = torch.autograd.grad(ref, x)
            got = XO.xent_seq(x, t, Lc, ignore_index=ignore, smoothing=eps)
            assert torch.allclose(got["loss"], ref.detach(), rtol=1e-12, atol=0)
            assert torch.allclose(got["d_logits"], grad, rtol=1e-10, atol=1e-15)
            assert got["count"] == int((t != ignore).sum())
            assert torch.allclose(got["row_nll"], F.cross_entropy(x.detach(), t, ignore_index=ignore, reduction="none"), rtol=1e-12, atol=0)


def test_oracle_masks_weights_empty_and_bad_targets():
    g = torch.Generator().manual_seed(6)
    B, Lc, V = 4, 7, 11
    x = torch.randn(B * Lc, V, generator=g)
    t = torch.randint(1, V, (B * Lc,), generator=g)
    lengths = torch.tensor([7, 4, 1, 0], dtype=torch.int32)
    w = torch.randn(B * Lc, generator=g)
    got = XO.xent_seq(x, t, Lc, lengths=lengths, smoothing=0.1, row_weight=w)
    assert got["cap_tokens"].tolist() == [7, 4, 1, 0] and got["count"] == 12 and float(got["cap_nll"][3]) == 0.0
    m = XO.counted_mask(t, Lc, lengths)
    lp = torch.log_softmax(x.double(), 1)
    row = 0.9 * -lp[torch.arange(B * Lc), t] + 0.1 * -lp.mean(1)
    assert torch.allclose(got["loss"], (w.double() * row)[m].sum() / 12, rtol=1e-12)
    assert bool((got["d_logits"][~m] == 0).all()) and bool((got["row_nll"][~m] == 0).all())
    empty = XO.xent_seq(x, t, Lc, lengths=torch.zeros(B, dtype=torch.int32))
    assert float(empty["loss"]) == 0.0 and empty["count"] == 0 and bool((empty["d_logits"] == 0).all())
    t[0] = V
    bad = XO.xent_seq(x, t, Lc, lengths=lengths)
    assert torch.isnan(bad["loss"]) and torch.isnan(bad["cap_nll"][0]) and not torch.isnan(bad["cap_nll"][1:]).any()
