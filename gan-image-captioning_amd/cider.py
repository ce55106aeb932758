"""CIDEr-D (Vedantam et al. 2015; the coco-caption ``CiderScorer``) on token ids, scored on the GPU by ``gic_cider_d`` (csrc/cider.hip).
No reference counterpart: the reference reports no caption metric.  Definition: gicap.h and DESIGN.md section 13.

The document-frequency table is built once on the host (numpy, vectorised) from a reference corpus -- lists of token lists grouped by
image -- and uploaded as sorted unique n-gram keys with their idf; ``CiderD.score`` then reads candidate ids already on the device and
returns device f32 scores without a host sync.  Only dataset tokens are scored: there is no PTB tokenizer.

Key of an n-gram (n = 1..4, token ids < 32768): ``(n - 1) << 60 | t_0 << 45 | t_1 << 30 | t_2 << 15 | t_3`` with the unused slots 0.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, engine

SPECIAL_IDS = (0, 1, 2)            # <PAD>, <S>, <E>: not part of a caption's tokens (evaluate()'s words())
MAX_N = 4


def strip(tokens) -> List[int]:
    return [int(t) for t in tokens if int(t) not in SPECIAL_IDS]


def _check_vocab(V: int) -> None:
    if V > _lib.CIDER_MAX_VOCAB:
        raise ValueError(f"CIDEr-D keys hold 15-bit token ids: vocabulary size {V} > {_lib.CIDER_MAX_VOCAB} is not supported")


def pack_keys(tokens: np.ndarray, n: int) -> np.ndarray:
    """uint64 keys of the n-grams whose tokens are the rows of ``tokens`` int [rows, n]."""
    tokens = np.asarray(tokens, dtype=np.uint64).reshape(-1, n)
    key = np.full(tokens.shape[0], np.uint64(n - 1) << np.uint64(60), dtype=np.uint64)
    for j in range(n):
        key |= tokens[:, j] << np.uint64(15 * (3 - j))
    return key


def unpack_key(key: int) -> Tuple[int, ...]:
    """The token ids of one key (the inverse of ``pack_keys``)."""
    key = int(key)
    n = (key >> 60) + 1
    return tuple((key >> (15 * (3 - j))) & 0x7FFF for j in range(n))


def unigram_df(keys: np.ndarray, df: np.ndarray) -> dict:
    """{token id: document frequency} of the 1-gram keys among ``keys`` uint64 / ``df`` (``document_frequency``'s outputs)."""
    keys = np.asarray(keys, dtype=np.uint64)
    one = (keys >> np.uint64(60)) == 0
    tok = (keys[one] >> np.uint64(45)) & np.uint64(0x7FFF)
    return dict(zip(tok.tolist(), np.asarray(df)[one].tolist()))


def _pad(captions: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """Stripped captions as a zero-padded int64 matrix [rows, Lmax] and their lengths."""
    rows = [strip(c) for c in captions]
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    out = np.zeros((len(rows), max(1, int(lens.max()) if len(rows) else 1)), dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, lens


def corpus_ngram_keys(corpus: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray]:
    """Every n-gram occurrence of the corpus's references: (keys uint64, image index int64), one entry per occurrence."""
    caps = [c for refs in corpus for c in refs]
    img = np.repeat(np.arange(len(corpus)), [len(refs) for refs in corpus])
    if not caps:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    tok, lens = _pad(caps)
    if tok.size and int(tok.max()) >= _lib.CIDER_MAX_VOCAB:
        raise ValueError(f"a reference token id is >= {_lib.CIDER_MAX_VOCAB}: CIDEr-D keys hold 15-bit token ids")
    keys, owners = [], []
    for n in range(1, MAX_N + 1):
        m = tok.shape[1] - n + 1
        if m <= 0:
            continue
        win = np.stack([tok[:, j:j + m] for j in range(n)], -1)                  # [rows, m, n]
        valid = np.arange(m)[None, :] + n <= lens[:, None]
        keys.append(pack_keys(win[valid], n))
        owners.append(np.broadcast_to(img[:, None], valid.shape)[valid])
    return np.concatenate(keys), np.concatenate(owners)


def document_frequency(corpus: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray]:
    """(keys uint64 [K] sorted unique, df int64 [K]): df(g) = the number of images whose reference set contains g."""
    keys, owner = corpus_ngram_keys(corpus)
    if keys.size == 0:
        return keys, np.zeros(0, np.int64)
    order = np.lexsort((owner, keys))                   # by key, then image
    keys, owner = keys[order], owner[order]
    first = np.ones(keys.size, dtype=bool)
    first[1:] = (keys[1:] != keys[:-1]) | (owner[1:] != owner[:-1])
    return np.unique(keys[first], return_counts=True)


class RefBatch:
    """References of B images packed for gic_cider_d: ids int64 [n_ref, Lr] (zero-padded), lengths int32 [n_ref], offsets int32
    [B+1] (image b owns rows off[b] .. off[b+1]), and the largest per-image count."""

    def __init__(self, ids: torch.Tensor, lengths: torch.Tensor, offsets: torch.Tensor, max_refs: int):
        self.ids, self.lengths, self.offsets, self.max_refs = ids, lengths, offsets, int(max_refs)

    @property
    def num_images(self) -> int:
        return self.offsets.numel() - 1

    @classmethod
    def pack(cls, groups: Sequence[Sequence[Sequence[int]]]) -> "RefBatch":
        """From per-image lists of token lists (host tensors; ``to(device)`` moves them)."""
        caps = [list(map(int, c)) for refs in groups for c in refs]
        Lr = max([len(c) for c in caps] + [1])
        if Lr > _lib.CIDER_MAX_LEN:
            raise ValueError(f"a reference has {Lr} tokens: CIDEr-D scores references of at most {_lib.CIDER_MAX_LEN}")
        counts = [len(refs) for refs in groups]
        if counts and max(counts) > _lib.CIDER_MAX_REFS:
            raise ValueError(f"an image has {max(counts)} references: CIDEr-D takes at most {_lib.CIDER_MAX_REFS}")
        ids = torch.zeros(len(caps), Lr, dtype=torch.int64)
        for i, c in enumerate(caps):
            ids[i, :len(c)] = torch.tensor(c, dtype=torch.int64)
        lengths = torch.tensor([len(c) for c in caps], dtype=torch.int32)
        offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)
        return cls(ids, lengths, offsets, max(counts + [0]))

    def to(self, device) -> "RefBatch":
        return RefBatch(self.ids.to(device, non_blocking=True), self.lengths.to(device, non_blocking=True),
                        self.offsets.to(device, non_blocking=True), self.max_refs)


def flat_candidates(cand_ids: torch.Tensor, refs: RefBatch, cand_img: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two candidate shapes of the scorers as (ids [rows, L], image index int32 [rows]): [B, n, L] (n per image, image-major), or
    [rows, L] with ``cand_img`` (None with rows = B: one per image)."""
    dev = cand_ids.device
    B = refs.num_images
    if cand_ids.dim() == 3:
        if cand_ids.shape[0] != B:
            raise ValueError(f"candidates for {cand_ids.shape[0]} images, references for {B}")
        n = cand_ids.shape[1]
        return cand_ids.reshape(B * n, cand_ids.shape[2]), torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(n)
    return cand_ids, (torch.arange(cand_ids.shape[0], device=dev, dtype=torch.int32) if cand_img is None else cand_img)


class CiderD:
    """CIDEr-D scorer whose document frequencies come from ``corpus`` (per-image lists of reference token lists); holds the table on
    ``device``.  ``vocab_size`` above 32768 is refused (15-bit keys)."""

    def __init__(self, corpus: Sequence[Sequence[Sequence[int]]], vocab_size: int, device):
        _check_vocab(int(vocab_size))
        self.V = int(vocab_size)
        keys, df = document_frequency(corpus)
        self.num_images = len(corpus)
        self.log_n = math.log(float(self.num_images)) if self.num_images else 0.0
        idf = self.log_n - np.log(np.maximum(1.0, df.astype(np.float64)))
        self.keys = torch.from_numpy(keys.view(np.int64).copy()).to(device)     # all keys < 2^62: int64 order = uint64 order
        self.idf = torch.from_numpy(idf.astype(np.float32)).to(device)
        self.df = df
        self.keys_host = keys                                 # the table's keys on the host (unigram_df: no device read)

    def score(self, cand_ids: torch.Tensor, cand_lengths: torch.Tensor, refs: RefBatch, cand_img: torch.Tensor = None) -> torch.Tensor:
        """CIDEr-D of candidates int64 [B, n, L] (n per image, image-major) or [rows, L] with ``cand_img`` int [rows] (None with
        rows = B: one per image) against ``refs`` (a RefBatch on the device, B images).  ``cand_lengths``: the ids before each length
        are the caption (specials are dropped).  Returns device f32 scores of ``cand_lengths``'s shape; no host sync."""
        flat, img = flat_candidates(cand_ids, refs, cand_img)
        if flat.shape[1] > _lib.CIDER_MAX_LEN:
            raise ValueError(f"candidates of {flat.shape[1]} ids: CIDEr-D scores at most {_lib.CIDER_MAX_LEN}")
        out = engine.cider_d(flat, cand_lengths.reshape(-1), img, refs.ids, refs.lengths, refs.offsets, refs.max_refs, self.keys, self.idf,
                             self.log_n, self.V)
        return out.view(cand_lengths.shape)

    def pairwise(self, ids: torch.Tensor, lengths: torch.Tensor, want_matrix: bool = True, want_consensus: bool = True,
                 want_self_cider: bool = True) -> dict:
        """CIDEr-D among the K captions of each image (gic_cider_pairwise; gicap.h): ``ids`` int64 [B, K, L],
        ``lengths`` [B, K], K <= 32.  Returns {"matrix": f32 [B, K, K] -- caption i as the candidate against caption j as the single
        reference, in CIDEr-D units --, "consensus": f32 [B, K], each caption's mean score against the K - 1 others (the
        minimum-Bayes-risk pick is its argmax), "self_cider": f32 [B], the Self-CIDEr diversity of each set (Wang & Chan 2019; 0 =
        all alike, 1 = nothing shared)}; an output that is not wanted is None.  One launch, no host sync."""
        if ids.dim() != 3:
            raise ValueError(f"pairwise takes ids [B, K, L], got {tuple(ids.shape)}")
        if not 1 <= ids.shape[1] <= _lib.CIDER_PAIR_MAX_K:
            raise ValueError(f"pairwise CIDEr-D compares 1..{_lib.CIDER_PAIR_MAX_K} captions per image, got {ids.shape[1]}")
        if not 1 <= ids.shape[2] <= _lib.CIDER_MAX_LEN:
            raise ValueError(f"captions of {ids.shape[2]} ids: CIDEr-D scores 1..{_lib.CIDER_MAX_LEN}")
        return engine.cider_pairwise(ids, lengths, self.keys, self.idf, self.log_n, self.V, want_matrix=want_matrix,
                                     want_consensus=want_consensus, want_self_cider=want_self_cider)

    def self_cider(self, ids: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """The Self-CIDEr diversity f32 [B] of the caption sets ``ids`` [B, K, L] (``pairwise`` with that output alone)."""
        return self.pairwise(ids, lengths, want_matrix=False, want_consensus=False)["self_cider"]
