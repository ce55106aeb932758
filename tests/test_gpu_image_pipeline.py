"""gic_image_preprocess on the GPU against the float64 oracle (tests/image_pipeline_oracle.py), element by element, on the smallest
shapes at which each thing can go wrong (IO.CASES), alone at each case's own S and together as one ragged batch in three layouts.

The bound, derived (U = 2^-24, the unit roundoff of f32; pixel values v <= 255):
  * the kernel takes its centres and the weight sums from float64 and forms a weight as max(0, 1 - |d0 + k| / fs) * norm with d0 the
    f32 rounding of (first - c + 0.5): a few roundings, each relative U, on weights that sum to 1 -- a constant number of U * 255;
  * a pass is an f32 sum of n products w * v with sum w = 1: at most n * U * 255 of accumulated rounding (the sum_bound form of
    tests/disc_cases.py); the horizontal pass has n_x terms, the vertical one n_y, and the vertical one carries the horizontal error
    through convex weights unchanged;
  so in pixel units |err| <= (n_x + n_y + 8) U 255, with 8 for the constant terms (disc_cases.sum_bound allows 4 per sum).  The output
  is (v / 255 - mean_c) / std_c: the pixel error divided by 255 std_c, plus the roundings of the two normalisation constants and of
  the final multiply-add, 4 U |ref|.  No term comes from a run of the kernel; a ratio above 1 is a bug.
"""
import numpy as np
import pytest
import torch

from tests import image_pipeline_oracle as IO
from tests.disc_cases import U
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

assert U == 2.0 ** -24
BATCH_S = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def refs():
    """Oracle outputs, computed once: per case at its own S, and at BATCH_S for the ragged batch."""
    own, batch = [], []
    for i, (name, h, w, c, S, box, flip) in enumerate(IO.CASES):
        img = IO.case_image(i)
        b = IO.f32_box(box, h, w)
        own.append(IO.preprocess(img, S, b, bool(flip)))
        batch.append(own[-1] if S == BATCH_S else IO.preprocess(img, BATCH_S, b, bool(flip)))
    return own, batch


def _pack(items, layout):
    """(pixels uint8 CPU tensor, descriptor rows, base offset of the live bytes) of ``items`` [(img, box, flip)].  ``aligned``: the
    collate's layout (tasks.RawImageBatch: offsets and strides padded to 16 bytes); ``awkward``: odd offsets, row_stride = W*C + 1,
    0xEE in every byte that is no pixel; ``bytes``: the awkward layout behind a base pointer that is not 4-byte aligned either."""
    from gan_image_captioning_amd.tasks import RawImageBatch
    if layout == "aligned":
        boxes = torch.tensor([it[1] for it in items], dtype=torch.float32)
        flips = torch.tensor([int(it[2]) for it in items])
        b = RawImageBatch.from_arrays([it[0] for it in items], 1, boxes, flips)
        return b.pixels, b.descs(), 0
    rows, at = [], 1
    for img, box, flip in items:
        h, w = img.shape[:2]
        c = 1 if img.ndim == 2 else 3
        stride = w * c + 1
        rows.append((at, h, w, c, stride, box, int(flip)))
        at += h * stride + (2 if (h * stride) % 2 == 0 else 1)           # keeps every offset odd
    base = 1 if layout == "bytes" else 0
    buf = np.full(base + at + 3, 0xEE, dtype=np.uint8)
    for (off, h, w, c, stride, _, _), (img, _, _) in zip(rows, items):
        assert off % 2 == 1
        buf[base + off:base + off + h * stride].reshape(h, stride)[:, :w * c] = img.reshape(h, w * c)
    return torch.from_numpy(buf), rows, base


def _run(dev, items, S, layout="aligned", stream=None):
    """One gic_image_preprocess call into a guarded buffer; returns (Guarded, the live [N,3,S,S] view)."""
    from gan_image_captioning_amd import engine
    pixels, descs, base = _pack(items, layout)
    px = pixels.to(dev)[base:]
    assert px.data_ptr() % 4 == (1 if layout == "bytes" else 0)
    g = Guarded(len(items), 3 * S * S, torch.float32, dev, float("nan"))
    out = g.live.view(len(items), 3, S, S)
    if stream is None:
        engine.image_preprocess(px, descs, S, out=out)
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            engine.image_preprocess(px, descs, S, out=out)
        px.record_stream(stream)
    return g, out


def _check(name, got, ref, taps):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / IO.error_bound(ref, taps)).max())
    print(f"{name}: taps {taps}, worst |err| / bound = {ratio:.4f}")
    assert np.isfinite(got).all(), name
    assert ratio <= 1.0, (name, ratio)


def _item(i):
    name, h, w, c, S, box, flip = IO.CASES[i]
    return IO.case_image(i), IO.f32_box(box, h, w), flip


@pytest.mark.parametrize("i", range(len(IO.CASES)), ids=[c[0] for c in IO.CASES])
def test_every_element_within_the_derived_bound(dev, refs, i):
    S = IO.CASES[i][4]
    g, out = _run(dev, [_item(i)], S)
    torch.cuda.synchronize()
    assert g.guards_intact()
    ref, taps = refs[0][i]
    _check(IO.CASES[i][0], out[0].cpu().numpy(), ref, taps)
    g2, out2 = _run(dev, [_item(i)], S)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))             # two runs, the same bits
    if IO.CASES[i][0] == "identity":
        # n = 1 on both axes: the output is the normalised pixels
        px = IO.case_image(i).astype(np.float64).transpose(2, 0, 1)
        want = (px / 255.0 - IO.MEAN[:, None, None]) / IO.STD[:, None, None]
        _check("identity vs pixels", out[0].cpu().numpy(), want, (1, 1))


def test_ragged_batch_in_three_layouts(dev, refs):
    items = [_item(i) for i in range(len(IO.CASES))]
    outs = {}
    for layout in ("aligned", "awkward", "bytes"):
        g, out = _run(dev, items, BATCH_S, layout)
        torch.cuda.synchronize()
        assert g.guards_intact(), layout
        outs[layout] = out
        got = out.cpu().numpy()
        for i, (ref, taps) in enumerate(refs[1]):
            _check(f"{layout}/{IO.CASES[i][0]}", got[i], ref, taps)
    bits = {k: v.view(torch.int32) for k, v in outs.items()}
    assert torch.equal(bits["aligned"], bits["awkward"]) and torch.equal(bits["aligned"], bits["bytes"])
    # more images than one descriptor-staging launch carries (64): the same bits, image for image
    _, big = _run(dev, items * 6, BATCH_S)
    assert torch.equal(big.view(torch.int32), bits["aligned"].repeat(6, 1, 1, 1))
    # an image alone and the same image inside the batch: the same bits (the stage is sized by the batch's widest row)
    for i, case in enumerate(IO.CASES):
        if case[4] == BATCH_S:
            _, alone = _run(dev, [items[i]], BATCH_S)
            assert torch.equal(alone[0].view(torch.int32), bits["aligned"][i]), case[0]


def test_flip_mirrors_and_grey_replicates_bit_for_bit(dev):
    img, box, _ = _item(7)
    _, out = _run(dev, [(img, box, 0), (img, box, 1)], 16)
    assert torch.equal(out[1].view(torch.int32), out[0].flip(-1).view(torch.int32))
    grey, gbox, _ = _item(10)
    rgb = np.repeat(grey[:, :, None], 3, axis=2)
    for layout in ("aligned", "awkward"):
        _, out = _run(dev, [(grey, gbox, 0), (rgb, gbox, 0)], 8, layout)
        # the same pixel values through the same weights; only the normalisation constants differ per plane
        assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


def test_wide_output_takes_the_twelve_item_kernel(dev):
    """S > 256: twelve (column, channel) items per thread; a down- and an up-scaled axis, a box and a flip, odd S with a partial last
    band."""
    S = 301
    img = IO.make_image(40, 700, 3, 9)
    box = IO.f32_box((10.25, 1.5, 690.5, 39.0), 40, 700)
    g, out = _run(dev, [(img, box, 1)], S, "awkward")
    torch.cuda.synchronize()
    assert g.guards_intact()
    ref, taps = IO.preprocess(img, S, box, True)
    _check("wide", out[0].cpu().numpy(), ref, taps)


def test_a_second_stream_leaves_the_first_result_alone(dev, refs):
    items = [_item(3), _item(11)]
    g1, out1 = _run(dev, items, 16)
    torch.cuda.synchronize()
    keep = out1.clone()
    side = torch.cuda.Stream(dev)
    g2, out2 = _run(dev, [_item(6), _item(9)], 16, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    assert g1.guards_intact() and g2.guards_intact()
    assert torch.equal(out1.view(torch.int32), keep.view(torch.int32))
    for k, i in enumerate((6, 9)):
        _check(f"side stream/{IO.CASES[i][0]}", out2[k].cpu().numpy(), *refs[1][i])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_synthetic_raw_batch_through_the_collate_matches_the_oracle(dev):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData, make_collate
    S, B = 64, 8
    ds = SyntheticCaptionData(B, 50, S, 10, seed=5, raw=True, augment="crop-flip")
    items = [ds[i] for i in range(B)]
    torch.manual_seed(3)
    images, caps, lengths, L = make_collate(ds)(items)
    out = images.to(dev)
    assert out.shape == images.shape == (B, 3, S, S) and out.dtype == torch.float32 and out.is_cuda
    got = out.cpu().numpy()
    assert images.flips.sum() > 0
    for i, (img, _) in enumerate(items):
        ref, taps = IO.preprocess(img, S, tuple(images.boxes[i].tolist()), bool(images.flips[i]))
        _check(f"synthetic {img.shape}", got[i], ref, taps)
    # whole images, no augmentation: the validation path
    val = make_collate(SyntheticCaptionData(B, 50, S, 10, seed=5, raw=True))(items)[0]
    got = val.to(dev).cpu().numpy()
    for i, (img, _) in enumerate(items):
        _check(f"synthetic whole {img.shape}", got[i], *IO.preprocess(img, S))


def test_main_trains_and_evaluates_on_device_preprocessed_images(dev, tmp_path):
    """cfg1's shape (ResNet-18 at 64x64, B = 8, L = 10): one pre-training epoch, one adversarial epoch, one evaluate; the first training
    batch of two passes with the same seed is bit-identical."""
    from gan_image_captioning_amd.main import main
    argv = ["--synthetic", "1", "--synthetic-batches", "2", "--synthetic-caption-len", "10", "--vocab-size", "64",
            "--adv-train-batch-size", "8", "--adv-eval-batch-size", "8", "--pre-train-batch-size", "8", "--pre-eval-batch-size", "8",
            "--adv-epochs", "1", "--pretrain-epochs", "1", "--gen-hidden-dim", "32", "--gen-embed-dim", "16", "--image-size", "64",
            "--conditional-gan", "1", "--encoder-arch", "resnet18", "--save-dir", str(tmp_path), "--expt-name", "p", "--num-workers", "0",
            "--compute-dtype", "bf16", "--device-preprocess", "1", "--augment", "crop-flip", "--eval-beam-size", "2"]
    inst = main(argv)
    torch.cuda.synchronize()
    assert inst.train_dataset.raw and inst.train_dataset.augment == "crop-flip" and inst.dev_dataset.augment == "none"
    assert int(inst.pretrain_opt.step_count) == 2 and int(inst.gen_opt.step_count) == 2
    for p in list(inst.gen.parameters()) + list(inst.disc.parameters()):
        assert bool(torch.isfinite(p).all())
    assert np.isfinite(np.asarray(inst.genpretrain_loop("val"), dtype=np.float64)).all()
    assert np.isfinite(np.asarray(inst.adv_loop("val"), dtype=np.float64)).all()
    assert np.isfinite(float(inst.evaluate("val", beam_size=2)))
    first = []
    for _ in range(2):
        torch.manual_seed(77)
        batch = next(iter(inst.adv_train_loader))
        first.append((batch[0].to(dev), batch[1]))
    assert first[0][0].shape == (8, 3, 64, 64)
    assert torch.equal(first[0][0].view(torch.int32), first[1][0].view(torch.int32)) and torch.equal(first[0][1], first[1][1])
