"""Data side of the trainer: the reference's ``COCO_data`` / ``collate_fn`` contract
(src/tasks.py:18-158) plus a synthetic dataset of the same batch shape.

Batch contract (tasks.py:138-158): ``(images f32[B,3,S,S], captions i64[B,Lmax], lengths i32[B],
max_caption_len)`` with caption rows ``[<S>=1] + tokens + [<E>=2] + [<PAD>=0]*`` and
``max_caption_len = longest caption + 2``.  Specials: <PAD>=0, <S>=1, <E>=2, <UNK>=3 (tasks.py:42-45).

Image decoding is host work outside the timed hot path; torchvision is not required (the resize /
to-tensor / normalise pipeline of tasks.py:92-100 is restated with PIL + numpy).

``device_preprocess``: the datasets hand out the decoded uint8 arrays instead (``load_image_raw``), the collate packs them into a
``RawImageBatch`` and draws the train-time crop boxes / flips, and ``RawImageBatch.to(device)`` uploads the bytes and runs
gic_image_preprocess -- crop, flip, antialiased resize, grey -> 3 channels, normalisation in one kernel -- returning the f32
[B,3,S,S] tensor every consumer takes.  Only the JPEG decode stays on the host.
"""
from __future__ import annotations

import functools
import json
import math
import os
import pickle
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .args import AUGMENT_NEEDS_DEVICE

SPECIALS = ("<PAD>", "<S>", "<E>", "<UNK>")
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def load_image(path: str, size: int) -> torch.Tensor:
    """Resize((S,S), bilinear) -> [0,1] CHW -> grey to 3 channels -> ImageNet normalise (tasks.py:92-100)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "L"):
            im = im.convert("RGB")
        im = im.resize((size, size), resample=Image.BILINEAR)
        arr = np.asarray(im, dtype=np.float32) / 255.0
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    arr = (arr - IMAGENET_MEAN) / IMAGENET_STD
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def load_image_raw(path: str) -> np.ndarray:
    """The decoded image as it is: uint8 [H,W,3] (RGB) or [H,W] (L); any other mode is converted to RGB.  No resize, no float work."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "L"):
            im = im.convert("RGB")
        return np.array(im, dtype=np.uint8)


AUGMENTS = ("none", "flip", "crop", "crop-flip")
CROP_RATIO = (3.0 / 4.0, 4.0 / 3.0)


def check_augment(augment: str, crop_scale) -> Tuple[float, float]:
    if augment not in AUGMENTS:
        raise ValueError(f"unknown augment {augment!r} (use one of {', '.join(AUGMENTS)})")
    lo, hi = (float(v) for v in crop_scale)
    if not (0.0 < lo <= hi <= 1.0):
        raise ValueError(f"crop scale ({lo}, {hi}) must satisfy 0 < lo <= hi <= 1")
    return lo, hi


def random_resized_crop_box(height: int, width: int, scale=(0.5, 1.0), ratio=CROP_RATIO) -> Tuple[float, float, float, float]:
    """(x0, y0, x1, y1) by torchvision's RandomResizedCrop rule: area fraction uniform in ``scale``, aspect ratio log-uniform in
    ``ratio``, ten tries, then the centred fallback (the whole image where its own ratio is in range).  The box keeps its fractional
    size and position -- the resize takes any box -- so area and ratio are exactly the drawn ones.  Draws come from ``torch.rand``."""
    area = float(height) * float(width)
    u = torch.rand(10, 4).tolist()
    for a, r, ux, uy in u:
        target = area * (scale[0] + a * (scale[1] - scale[0]))
        aspect = math.exp(math.log(ratio[0]) + r * (math.log(ratio[1]) - math.log(ratio[0])))
        w, h = math.sqrt(target * aspect), math.sqrt(target / aspect)
        if 0.0 < w <= width and 0.0 < h <= height:
            x0, y0 = ux * (width - w), uy * (height - h)
            return x0, y0, min(x0 + w, float(width)), min(y0 + h, float(height))
    in_ratio = float(width) / float(height)
    if in_ratio < ratio[0]:
        w, h = float(width), float(width) / ratio[0]
    elif in_ratio > ratio[1]:
        w, h = float(height) * ratio[1], float(height)
    else:
        w, h = float(width), float(height)
    x0, y0 = (width - w) / 2.0, (height - h) / 2.0
    return x0, y0, x0 + w, y0 + h


def draw_augmentation(shapes, augment: str = "none", crop_scale=(0.5, 1.0)):
    """(boxes f32 [B,4], flips int64 [B]) for images of ``shapes`` [(H, W)]: whole-image boxes and no flips under ``none``."""
    lo, hi = check_augment(augment, crop_scale)
    boxes = torch.tensor([[0.0, 0.0, float(w), float(h)] for h, w in shapes], dtype=torch.float32).reshape(len(shapes), 4)
    flips = torch.zeros(len(shapes), dtype=torch.int64)
    if augment in ("crop", "crop-flip"):
        for i, (h, w) in enumerate(shapes):
            x0, y0, x1, y1 = random_resized_crop_box(h, w, (lo, hi))
            b = torch.tensor([x0, y0, x1, y1], dtype=torch.float32)
            # f32 rounding must not push the box out of the image or empty it
            b[2:] = torch.minimum(b[2:], torch.tensor([float(w), float(h)]))
            b[:2] = b[:2].clamp_(min=0.0)
            if bool(b[0] < b[2]) and bool(b[1] < b[3]):
                boxes[i] = b
    if augment in ("flip", "crop-flip"):
        flips = (torch.rand(len(shapes)) < 0.5).to(torch.int64)
    return boxes, flips


class RawImageBatch:
    """A ragged batch of decoded uint8 images waiting for the device: ``pixels`` is ONE flat uint8 tensor (each image's offset and row
    stride padded to 16 bytes), ``table`` int64 [B,6] = (offset, height, width, channels, row_stride, flip), ``boxes`` f32 [B,4] =
    (x0, y0, x1, y1) in source pixels, ``size`` the target S.  It stands where the f32 [B,3,S,S] image tensor stood: ``len``,
    ``.shape``, ``.pin_memory()`` (DataLoader(pin_memory=True) pins it), pickling across loader workers, and ``.to(device)``, which
    uploads the bytes, runs gic_image_preprocess and RETURNS THE f32 [B,3,S,S] DEVICE TENSOR."""

    ALIGN = 16

    def __init__(self, pixels: torch.Tensor, table: torch.Tensor, boxes: torch.Tensor, size: int):
        self.pixels, self.table, self.boxes, self.size = pixels, table, boxes, int(size)

    @classmethod
    def from_arrays(cls, arrays, size: int, boxes: Optional[torch.Tensor] = None, flips: Optional[torch.Tensor] = None):
        al = cls.ALIGN
        rows, total = [], 0
        for a in arrays:
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
                raise ValueError(f"raw image must be a non-empty uint8 [H,W], [H,W,1] or [H,W,3] array, got {a.dtype} {a.shape}")
            h, w = a.shape[:2]
            c = 1 if a.ndim == 2 else a.shape[2]
            stride = (w * c + al - 1) // al * al
            rows.append((total, h, w, c, stride, a.reshape(h, w * c)))
            total += h * stride
        buf = np.zeros(total, dtype=np.uint8)
        for off, h, w, c, stride, a in rows:
            buf[off:off + h * stride].reshape(h, stride)[:, :w * c] = a
        B = len(rows)
        if boxes is None:
            boxes = torch.tensor([[0.0, 0.0, float(r[2]), float(r[1])] for r in rows], dtype=torch.float32).reshape(B, 4)
        if flips is None:
            flips = torch.zeros(B, dtype=torch.int64)
        table = torch.tensor([[r[0], r[1], r[2], r[3], r[4], int(f)] for r, f in zip(rows, flips.tolist())],
                             dtype=torch.int64).reshape(B, 6)
        return cls(torch.from_numpy(buf), table, boxes.to(torch.float32).reshape(B, 4).clone(), size)

    def __len__(self):
        return int(self.table.shape[0])

    def __getitem__(self, index):
        """A sub-batch (slice or index list) over the same bytes, as ``images[:k]`` of a tensor."""
        if isinstance(index, int):
            index = [index]
        return RawImageBatch(self.pixels, self.table[index], self.boxes[index], self.size)

    @property
    def shape(self):
        return torch.Size((len(self), 3, self.size, self.size))

    @property
    def flips(self) -> torch.Tensor:
        return self.table[:, 5]

    def descs(self):
        """The descriptor rows ``engine.image_preprocess`` takes."""
        return [(o, h, w, c, s, box, f) for (o, h, w, c, s, f), box in zip(self.table.tolist(), self.boxes.tolist())]

    def pin_memory(self):
        self.pixels = self.pixels.pin_memory()
        return self

    def to(self, device, non_blocking: bool = True) -> torch.Tensor:
        from . import engine
        dev = torch.device(device)
        if dev.type != "cuda":
            engine.require_gpu(self.pixels)                # refuses: there is no host implementation of the kernel
        return engine.image_preprocess(self.pixels.to(dev, non_blocking=non_blocking), self.descs(), self.size)


def stack_images(items, image_size: Optional[int] = None, augment: str = "none", crop_scale=(0.5, 1.0)):
    """The images of a batch as one object: f32 [B,3,S,S] for tensors (what the host path's datasets return), a ``RawImageBatch`` for
    raw uint8 arrays (``device_preprocess``), with the crop boxes / flips of ``augment`` drawn here."""
    items = list(items)
    if isinstance(items[0], torch.Tensor):
        return torch.stack(items)
    if image_size is None:
        raise ValueError("stack_images: raw images need the target image_size")
    boxes, flips = draw_augmentation([np.asarray(a).shape[:2] for a in items], augment, crop_scale)
    return RawImageBatch.from_arrays(items, image_size, boxes, flips)


class COCO_data(Dataset):
    """Karpathy-split COCO captions (dataset_coco.json); vocabulary built from the training split."""

    def __init__(self, captions_path, image_path, split, image_size=256, captions_per_image=5, vocab_dicts=None,
                 dataset_percent=1.0, device_preprocess=False, augment="none", crop_scale=(0.5, 1.0)):
        assert split in {"train", "val", "test"}
        self.split, self.image_path, self.image_size = split, image_path, image_size
        # device_preprocess: items carry the decoded uint8 array; the collate (make_collate) draws this dataset's augmentation.
        # Only the training split ever augments
        self.device_preprocess = bool(device_preprocess)
        self.crop_scale = check_augment(augment, crop_scale)
        if augment != "none" and not self.device_preprocess:
            raise ValueError(AUGMENT_NEEDS_DEVICE.format(augment=augment))
        self.augment = augment if split == "train" else "none"
        self.dataset_percent = dataset_percent
        cache = os.path.join(image_path, f"{split}_{captions_per_image}.pkl")      # tasks.py:30,88
        if os.path.exists(cache):
            print("Loading from saved dict")
            with open(cache, "rb") as fh:
                saved = pickle.load(fh)
            self.captions, self.word_to_index, self.index_to_word = saved["captions"], saved["w2i"], saved["i2w"]
        else:
            print("Creating and saving dict")
            with open(captions_path, "r") as fh:
                entries = json.load(fh)["images"]
            if vocab_dicts is None:
                self.word_to_index = {w: i for i, w in enumerate(SPECIALS)}
                self.index_to_word = {i: w for i, w in enumerate(SPECIALS)}
            else:
                self.word_to_index, self.index_to_word = vocab_dicts
            self.captions = []
            for row in entries:
                if split not in row["filepath"]:                                    # tasks.py:60
                    continue
                meta = {k: v for k, v in row.items() if not isinstance(v, list)}
                for sent in row["sentences"][:captions_per_image]:
                    self.captions.append({**meta, **sent})
                    if vocab_dicts is None:
                        for word in sent["tokens"]:
                            if word not in self.word_to_index:
                                idx = len(self.word_to_index)
                                self.word_to_index[word] = idx
                                self.index_to_word[idx] = word
            with open(cache, "wb+") as fh:
                pickle.dump({"captions": self.captions, "w2i": self.word_to_index, "i2w": self.index_to_word}, fh)
        self.vocab_size = len(self.word_to_index)

    def __len__(self):
        return int(self.dataset_percent * len(self.captions))

    def __getitem__(self, index):
        entry = self.captions[index]
        path = os.path.join(self.image_path, entry["filepath"], entry["filename"])
        image = load_image_raw(path) if self.device_preprocess else load_image(path, self.image_size)
        unk = self.word_to_index["<UNK>"]
        tokens = [t if isinstance(t, int) else self.word_to_index.get(t, unk) for t in entry["tokens"]]
        return image, tokens


class SyntheticCaptionData(Dataset):
    """Deterministic stand-in for COCO: normal-distributed "normalised pixels" and random token ids in
    [4, V) (no specials inside a caption), every caption the same length so max_caption_len is exact
    (SURVEY.md §8(d))."""

    def __init__(self, num_items: int, vocab_size: int, image_size: int = 224, caption_len: int = 20, seed: int = 1008,
                 ragged: bool = False, raw: bool = False, augment: str = "none", crop_scale=(0.5, 1.0)):
        self.vocab_size, self.image_size, self.n = vocab_size, image_size, num_items
        # raw: seeded uint8 "decoded images" of seeded sizes (S/2 .. 3S per side, one in four grey) for the device image pipeline
        self.device_preprocess = self.raw = bool(raw)
        self.crop_scale = check_augment(augment, crop_scale)
        if augment != "none" and not self.raw:
            raise ValueError(AUGMENT_NEEDS_DEVICE.format(augment=augment))
        self.augment = augment
        g = torch.Generator().manual_seed(seed)
        self.seeds = torch.randint(0, 2 ** 31 - 1, (num_items,), generator=g).tolist()
        self.body_len = caption_len - 2
        self.ragged = ragged
        self.word_to_index = {w: i for i, w in enumerate(SPECIALS)}
        self.index_to_word = {i: w for i, w in enumerate(SPECIALS)}

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seeds[index])
        if self.raw:
            S = self.image_size
            h, w, grey = (int(v) for v in torch.randint(0, 2 ** 20, (3,), generator=g))
            lo, span = max(1, S // 2), 3 * S - max(1, S // 2) + 1
            h, w = lo + h % span, lo + w % span
            image = torch.randint(0, 256, (h, w) if grey % 4 == 0 else (h, w, 3), generator=g, dtype=torch.uint8).numpy()
        else:
            image = torch.randn(3, self.image_size, self.image_size, generator=g)
        n = self.body_len if not self.ragged else int(torch.randint(1, self.body_len + 1, (1,), generator=g))
        tokens = torch.randint(4, self.vocab_size, (n,), generator=g).tolist()
        return image, tokens


def collate_fn(batch: Sequence[Tuple[torch.Tensor, List[int]]], image_size: Optional[int] = None, augment: str = "none",
               crop_scale=(0.5, 1.0)):
    """tasks.py:138-158.  Raw uint8 images (``device_preprocess``) come back as a ``RawImageBatch`` in the images' place."""
    images = stack_images([image for image, _ in batch], image_size, augment, crop_scale)
    max_caption_len = max(len(tokens) for _, tokens in batch) + 2
    captions = torch.zeros(len(batch), max_caption_len, dtype=torch.long)
    lengths = torch.zeros(len(batch), dtype=torch.int)
    for i, (image, tokens) in enumerate(batch):
        row = [1] + list(tokens) + [2]
        captions[i, :len(row)] = torch.tensor(row, dtype=torch.long)
        lengths[i] = len(row)
    return images, captions, lengths, max_caption_len


def synthetic_batch(batch: int, vocab_size: int, image_size: int, caption_len: int, seed: int = 1008, device=None,
                    with_images: bool = True):
    """One fixed batch straight on the device (bench / smoke): (images|None, captions, lengths, L)."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(batch, 3, image_size, image_size, generator=g) if with_images else None
    body = torch.randint(4, vocab_size, (batch, caption_len - 2), generator=g)
    captions = torch.cat([torch.ones(batch, 1, dtype=torch.long), body, torch.full((batch, 1), 2, dtype=torch.long)], 1)
    lengths = torch.full((batch,), caption_len, dtype=torch.int)
    if device is not None:
        images = images.to(device) if images is not None else None
        captions, lengths = captions.to(device), lengths.to(device)
    return images, captions, lengths, caption_len


def group_by_image(ds) -> Tuple[dict, list]:
    """The items of ``ds`` grouped by image: ``filepath`` + ``filename`` for COCO_data, one image per item otherwise.  Returns
    (groups {key: [item index]}, keys in first-seen order)."""
    groups, order = {}, []
    for i in range(len(ds)):
        if isinstance(ds, COCO_data):
            e = ds.captions[i]
            key = (e["filepath"], e["filename"])
        else:
            key = i
        if key not in groups:
            groups[key] = []
            order.append(key)
        groups[key].append(i)
    return groups, order


class ImageGroups(Dataset):
    """Image-grouped view of a caption dataset (the grouping of ``group_by_image``): item k = (image, [reference token lists]) of the
    k-th image; the image is loaded once per image.  ``references()`` gives every image's token lists without loading images (COCO)."""

    def __init__(self, ds):
        self.ds = ds
        self.groups, self.order = group_by_image(ds)
        self.coco = isinstance(ds, COCO_data)

    def __len__(self):
        return len(self.order)

    def _tokens(self, i):
        unk = self.ds.word_to_index.get("<UNK>", 3)
        return [t if isinstance(t, int) else self.ds.word_to_index.get(t, unk) for t in self.ds.captions[i]["tokens"]]

    def __getitem__(self, k):
        items = self.groups[self.order[k]]
        image, first = self.ds[items[0]]
        return image, [self._tokens(i) for i in items] if self.coco else [first]

    def references(self) -> List[List[List[int]]]:
        if self.coco:
            return [[self._tokens(i) for i in self.groups[k]] for k in self.order]
        return [[self.ds[self.groups[k][0]][1]] for k in self.order]


def make_collate(ds, groups: bool = False):
    """The collate of a loader over ``ds``: ``collate_fn`` / ``collate_groups`` themselves for the host path, and bound to the
    dataset's image size and augmentation where it hands out raw images."""
    fn = collate_groups if groups else collate_fn
    if not getattr(ds, "device_preprocess", False):
        return fn
    return functools.partial(fn, image_size=ds.image_size, augment=getattr(ds, "augment", "none"),
                             crop_scale=tuple(getattr(ds, "crop_scale", (0.5, 1.0))))


def collate_groups(batch: Sequence[Tuple[torch.Tensor, List[List[int]]]], image_size: Optional[int] = None, augment: str = "none",
                   crop_scale=(0.5, 1.0)):
    """(images f32 [B,3,S,S], refs) with refs = (ids int64 [n_ref, Lr] zero-padded, lengths int32 [n_ref], offsets int32 [B+1],
    max references per image): the references packed for gic_cider_d (cider.RefBatch.pack)."""
    from .cider import RefBatch
    images = stack_images([image for image, _ in batch], image_size, augment, crop_scale)
    r = RefBatch.pack([refs for _, refs in batch])
    return images, (r.ids, r.lengths, r.offsets, r.max_refs)
