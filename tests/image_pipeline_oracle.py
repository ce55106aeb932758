"""float64 restatement of the image pipeline's filter (gicap.h, gic_image_preprocess), with numpy loops, and the case list its tests
share.

Per axis (source length n, box [b0, b1), S outputs):
    scale = (b1 - b0) / S        fs = max(scale, 1)        c_i = b0 + (i + 0.5) scale
    first = max(int(c_i - fs + 0.5), 0)     last = min(int(c_i + fs + 0.5), n)         taps first .. last-1: clipped to the image
    w_x = max(0, 1 - |x - c_i + 0.5| / fs), normalised to sum 1 over the taps
separable, horizontal pass first, no rounding between the passes; flip reverses the output x index; one channel feeds all three;
out = (v / 255 - mean_c) / std_c.  The box is taken as the f32 values the descriptor carries."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).astype(np.float64)     # tasks.IMAGENET_MEAN / _STD, the f32 constants
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).astype(np.float64)


def axis_weights(n, S, b0, b1):
    """[(first, weights float64 [taps])] per output index, and the largest tap count."""
    b0, b1 = float(np.float32(b0)), float(np.float32(b1))
    scale = (b1 - b0) / S
    fs = max(scale, 1.0)
    out, most = [], 0
    for i in range(S):
        c = b0 + (i + 0.5) * scale
        first = max(int(c - fs + 0.5), 0)
        last = min(int(c + fs + 0.5), n)
        x = np.arange(first, last, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs(x - c + 0.5) / fs)
        out.append((first, w / w.sum()))
        most = max(most, last - first)
    return out, most


def resize_pixels(img, S, box=None, flip=False):
    """uint8 [H,W] or [H,W,C] -> float64 [S,S,3] in PIXEL units (0..255), plus (n_x, n_y) = the largest tap counts."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    x0, y0, x1, y1 = (0.0, 0.0, float(W), float(H)) if box is None else box
    wx, n_x = axis_weights(W, S, x0, x1)
    wy, n_y = axis_weights(H, S, y0, y1)
    src = img.astype(np.float64)
    hor = np.zeros((H, S, C))
    for i, (first, w) in enumerate(wx):
        hor[:, i, :] = (src[:, first:first + len(w), :] * w[None, :, None]).sum(axis=1)
    out = np.zeros((S, S, C))
    for r, (first, w) in enumerate(wy):
        out[r] = (hor[first:first + len(w)] * w[:, None, None]).sum(axis=0)
    if flip:
        out = out[:, ::-1, :]
    if C == 1:
        out = np.repeat(out, 3, axis=2)
    return np.ascontiguousarray(out), (n_x, n_y)


def preprocess(img, S, box=None, flip=False):
    """float64 [3,S,S] normalised as the kernel's output, plus (n_x, n_y)."""
    px, taps = resize_pixels(img, S, box, flip)
    return np.ascontiguousarray(((px / 255.0 - MEAN) / STD).transpose(2, 0, 1)), taps


def error_bound(ref, taps):
    """|kernel - oracle| allowed per element of ``ref`` [3,S,S] (derivation: tests/test_gpu_image_pipeline.py)."""
    U = 2.0 ** -24
    n_x, n_y = taps
    px = (n_x + n_y + 8) * U * 255.0
    return px / (255.0 * STD)[:, None, None] + 4 * U * np.abs(ref)


def make_image(h, w, c, seed):
    """A seeded mix of noise and a smooth ramp, uint8 [h,w] (c = 1) or [h,w,3]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = 255.0 * (0.6 * xx / max(w - 1, 1) + 0.4 * yy / max(h - 1, 1))
    chans = []
    for k in range(c):
        noise = rng.randint(0, 256, size=(h, w)).astype(np.float64)
        mix = np.where(rng.rand(h, w) < 0.5, noise, np.roll(ramp, 7 * k, axis=1))
        chans.append(np.clip(np.rint(mix), 0, 255).astype(np.uint8))
    return chans[0] if c == 1 else np.stack(chans, axis=2)


FRACTIONAL = (4.3, 2.6, 41.9, 30.2)
# (name, H, W, C, S, box or None, flip): the smallest shapes at which each thing can go wrong
CASES = [
    ("one-pixel", 1, 1, 3, 8, None, 0),                   # one tap, everything clipped
    ("upscale", 3, 5, 3, 8, None, 0),                     # 2 taps, borders
    ("identity", 16, 16, 3, 16, None, 0),                 # the output is the normalised pixels
    ("down", 37, 53, 3, 16, None, 0),                     # non-integer downscale on both axes
    ("down-up", 64, 7, 3, 16, None, 0),                   # down on one axis, up on the other
    ("wide", 3, 640, 3, 8, None, 0),                      # 80:1, 160 taps
    ("many-taps", 480, 640, 3, 16, None, 0),              # many taps on both axes
    ("box", 37, 53, 3, 16, FRACTIONAL, 0),                # fractional box: taps leave the box, stay in the image
    ("edge-box", 37, 53, 3, 16, (0.0, 0.0, 20.5, 37.0), 0),
    ("far", 8, 3000, 3, 16, (2900.3, 0.0, 2990.7, 8.0), 0),   # coordinates far from the origin
    ("grey", 20, 30, 1, 8, None, 0),
    ("flip", 37, 53, 3, 16, FRACTIONAL, 1),
    ("bands", 33, 45, 3, 224, None, 0),                   # the workload's S, several row bands
]


def case_image(i):
    name, h, w, c, S, box, flip = CASES[i]
    return make_image(h, w, c, 100 + i)


def f32_box(box, h, w):
    """The box as the f32 values a descriptor carries (whole image when None)."""
    b = (0.0, 0.0, float(w), float(h)) if box is None else box
    return tuple(float(np.float32(v)) for v in b)
