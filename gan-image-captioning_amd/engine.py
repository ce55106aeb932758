"""Tensor-level host wrappers around the C ABI: buffer planning + ctypes calls.

``DecoderEngine`` / ``DiscEngine`` own nothing but the derived compute-dtype weight
images; every other buffer (outputs, saved-for-backward state, workspaces, grads) is a
torch tensor allocated here through PyTorch's caching allocator and handed to the
library as a raw device pointer.  All launches go to the current PyTorch HIP stream.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L

TORCH_DTYPE = {L.F32: torch.float32, L.BF16: torch.bfloat16}
DTYPE_BY_NAME = {"fp32": L.F32, "f32": L.F32, "float32": L.F32, "bf16": L.BF16, "bfloat16": L.BF16}

_param_epoch = 0   # bumped by optimizers that update weights through raw pointers


def set_deterministic(on: bool) -> None:
    """Process-wide deterministic mode (gic_set_deterministic): with it on, the same inputs, weights, seeds, shapes, library
    build and device model give bit-identical results; no f32 sum has a run-to-run order.  Cached trunk and step graphs key on
    the mode, so a change takes effect at the next call.  GIC_DETERMINISTIC=1 turns it on when the library is loaded."""
    L.check(L.load().gic_set_deterministic(int(bool(on))), "gic_set_deterministic")


def deterministic() -> bool:
    return bool(L.load().gic_get_deterministic())


def bump_param_epoch() -> None:
    global _param_epoch
    _param_epoch += 1


class capture_guard:
    """Bracket for a hipGraph capture region: no cyclic garbage collection may run inside it.

    A generational collection that fires between two captured launches finalises whatever HIP-owning garbage the process has
    accumulated (stale ``CUDAGraph``s with their private pools, streams, events of dropped plans): a destructor that frees device
    memory or destroys a graph while a capture is open throws inside a C++ destructor -> ``std::terminate`` (the rc=134 abort of
    round 2).  torch >= 2.6 no longer collects before a capture (``force_cudagraph_gc`` is off), so this
    does: collect BEFORE the region (the garbage dies outside it), disable the collector inside, restore it afterwards."""

    def __enter__(self):
        import gc
        self._gc = gc
        self._was_enabled = gc.isenabled()
        gc.collect()
        gc.disable()
        return self

    def __exit__(self, *exc):
        if self._was_enabled:
            self._gc.enable()
        return False


class route_only:
    """Route-only mode of the calling thread (gicap.h gic_debug_route_only): inside, the library's GEMM / convolution entry points select
    their kernel and return without touching the GPU; ``last()`` is the selection as one line.  Always cleared on exit."""

    def __enter__(self):
        L.load().gic_debug_route_only(1)
        return self

    def __exit__(self, *exc):
        L.load().gic_debug_route_only(0)
        return False

    @staticmethod
    def last() -> str:
        return L.load().gic_debug_last_route().decode()


class on_stream:
    """``with torch.cuda.stream(s)`` without its per-entry device query (torch's StreamContext asks the runtime for the device count
    on every construction: ~20 us, a dozen times per step).  Single device per process (one process per GPU)."""
    __slots__ = ("s", "prev")

    def __init__(self, stream):
        self.s = stream

    def __enter__(self):
        self.prev = torch.cuda.current_stream(self.s.device)
        torch.cuda.set_stream(self.s)
        return self.s

    def __exit__(self, *exc):
        torch.cuda.set_stream(self.prev)
        return False


def parse_dtype(x) -> int:
    if isinstance(x, int):
        return x
    try:
        return DTYPE_BY_NAME[str(x).lower()]
    except KeyError:
        raise ValueError(f"unknown compute dtype {x!r} (use 'bf16' or 'fp32')")


def require_gpu(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise L.GicError("tensor is not on a GPU: the hot path runs only through the HIP library "
                             "(libgicap.so) on an AMD GPU and has no CPU fallback")


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _arr(ctype, n, values):
    a = (ctype * n)()
    for i, v in enumerate(values):
        a[i] = v
    return a


def _key(params: Sequence[torch.Tensor]):
    return tuple((p.data_ptr(), p._version) for p in params) + (_param_epoch,)


class StepScalarsBuffer:
    """Device-resident gic_step_scalars (gicap.h): the decoder's temperature and the seeds of the step's device noise streams, read
    by the kernels from device memory so that a captured step graph replays with unchanged launch arguments."""

    def __init__(self, device):
        self.buf = torch.zeros(C.sizeof(L.StepScalars), dtype=torch.uint8, device=device)
        self.ptr = self.buf.data_ptr()

    def set(self, temperature: float, seeds) -> None:
        """Enqueue the update on the current stream (values travel as kernel arguments)."""
        v = L.StepScalars()
        v.temperature = float(temperature)
        for i, sd in enumerate(seeds):
            v.seed[i] = int(sd) & (2 ** 64 - 1)
        L.check(L.load().gic_step_scalars_set(self.ptr, C.byref(v), stream_ptr()), "gic_step_scalars_set")


# ------------------------------------------------------------------------------------------ generic ops
def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, accumulate=False, alpha=1.0):
    require_gpu(A, B, Cout)
    in_dt = L.F32 if A.dtype == torch.float32 else L.BF16
    out_dt = L.F32 if Cout.dtype == torch.float32 else L.BF16
    L.check(L.load().gic_gemm(ptr(A), ptr(B), ptr(Cout), M, N, K, lda, ldb, ldc, int(a_kc), int(b_kc), in_dt, out_dt,
                              ptr(bias), int(accumulate), float(alpha), stream_ptr()), "gic_gemm")
    return Cout


def gemm_desc(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, accumulate=False, alpha=1.0, c_zeroed=False,
              no_split=False, wgrad=False, a_sum=None, a_sum2=None, C2=None, ldc2=0, n_split=0):
    """``gemm`` with the descriptor fields only the library's own call sites set (gicap.h gic_debug_gemm_desc): tests run them through it."""
    require_gpu(A, B, Cout, a_sum, a_sum2, C2)
    in_dt = L.F32 if A.dtype == torch.float32 else L.BF16
    out_dt = L.F32 if Cout.dtype == torch.float32 else L.BF16
    L.check(L.load().gic_debug_gemm_desc(ptr(A), ptr(B), ptr(Cout), M, N, K, lda, ldb, ldc, int(a_kc), int(b_kc), in_dt, out_dt, ptr(bias),
                                         int(accumulate), float(alpha), int(c_zeroed), int(no_split), int(wgrad), ptr(a_sum), ptr(a_sum2),
                                         ptr(C2), ldc2, n_split, stream_ptr()), "gic_debug_gemm_desc")
    return Cout


def cast2d(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, lds: int, ldd: int):
    require_gpu(src, dst)
    sd = L.F32 if src.dtype == torch.float32 else L.BF16
    dd = L.F32 if dst.dtype == torch.float32 else L.BF16
    L.check(L.load().gic_cast2d(ptr(src), sd, lds, ptr(dst), dd, ldd, rows, cols, stream_ptr()), "gic_cast2d")
    return dst


def _to_act(t: torch.Tensor, act: torch.dtype) -> torch.Tensor:
    """``t`` contiguous in the compute dtype ``act`` (cast on the GPU where it differs)."""
    t = t.contiguous()
    if t.dtype == act:
        return t
    n = t.shape[-1]
    return cast2d(t, torch.empty(t.shape, device=t.device, dtype=act), t.numel() // n, n, n, n)


def embedding_fwd(weight: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    require_gpu(weight, ids)
    ids = ids.contiguous()
    out = torch.empty(ids.numel(), weight.shape[1], device=weight.device, dtype=torch.float32)
    L.check(L.load().gic_embedding_fwd(ptr(weight), ptr(ids), ptr(out), ids.numel(), weight.shape[0], weight.shape[1],
                                       stream_ptr()), "gic_embedding_fwd")
    return out.view(*ids.shape, weight.shape[1])


def embedding_bwd(d_out: torch.Tensor, ids: torch.Tensor, V: int, d_weight: Optional[torch.Tensor] = None,
                  zero_first: bool = True) -> torch.Tensor:
    require_gpu(d_out, ids)
    E = d_out.shape[-1]
    d_out = d_out.contiguous()
    ids = ids.contiguous()
    if d_weight is None:
        d_weight = torch.empty(V, E, device=d_out.device, dtype=torch.float32)
    L.check(L.load().gic_embedding_bwd(ptr(d_out), ptr(ids), ptr(d_weight), ids.numel(), V, E, int(zero_first), stream_ptr()),
            "gic_embedding_bwd")
    return d_weight


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # tasks.IMAGENET_MEAN / _STD


def image_srcs(descs):
    """``(gic_image_src * N)`` from an iterable of ``(offset, height, width, channels, row_stride, (x0, y0, x1, y1), flip)`` rows (a
    ctypes array of ``_lib.ImageSrc`` passes through)."""
    if isinstance(descs, C.Array) and getattr(descs, "_type_", None) is L.ImageSrc:
        return descs
    rows = list(descs)
    arr = (L.ImageSrc * max(1, len(rows)))()
    for s, (offset, h, w, c, stride, box, flip) in zip(arr, rows):
        s.offset, s.height, s.width, s.channels, s.row_stride, s.flip = int(offset), int(h), int(w), int(c), int(stride), int(flip)
        for k in range(4):
            s.box[k] = float(box[k])
    return arr


def image_preprocess_ws_bytes(N: int, S: int) -> int:
    """Host-only size query of gic_image_preprocess's scratch."""
    out = C.c_uint64(0)
    L.check(L.load().gic_image_preprocess_ws_bytes(int(N), int(S), C.byref(out)), "gic_image_preprocess_ws_bytes")
    return int(out.value)


def image_preprocess(pixels_u8: torch.Tensor, descs, S: int, out: Optional[torch.Tensor] = None, mean=IMAGENET_MEAN,
                     std=IMAGENET_STD) -> torch.Tensor:
    """gic_image_preprocess on the current stream: a flat uint8 device tensor holding a ragged batch of HWC / HW images + their
    descriptors (``image_srcs``) -> f32 [N,3,S,S]: crop box, flip, antialiased bilinear resize, grey -> 3 channels, normalisation."""
    require_gpu(pixels_u8, out)
    if pixels_u8.dtype != torch.uint8 or pixels_u8.dim() != 1 or not pixels_u8.is_contiguous():
        raise ValueError("image_preprocess: pixels must be a flat contiguous uint8 tensor")
    src = image_srcs(descs)
    N = len(descs) if hasattr(descs, "__len__") else len(src)
    if out is None:
        out = torch.empty(max(N, 0), 3, int(S), int(S), device=pixels_u8.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, 3, int(S), int(S)) or not out.is_contiguous():
        raise ValueError(f"image_preprocess: out must be a contiguous f32 [{N},3,{S},{S}] tensor")
    ws = torch.empty(image_preprocess_ws_bytes(N, S), device=pixels_u8.device, dtype=torch.uint8)
    L.check(L.load().gic_image_preprocess(ptr(pixels_u8), pixels_u8.numel(), src, N, int(S), _arr(C.c_float, 3, mean),
                                          _arr(C.c_float, 3, std), ptr(out), ptr(ws), stream_ptr()), "gic_image_preprocess")
    return out


def sample_opts(num_samples: int = 1, top_k: int = 0, top_p: float = 1.0, temperature: float = 1.0, eos_id: int = 2,
                pad_id: int = 0) -> L.SampleOpts:
    """gic_sample_opts (h0 / c0 unset); the library checks the values."""
    o = L.SampleOpts()
    o.num_samples, o.top_k, o.top_p, o.temperature = int(num_samples), int(top_k), float(top_p), float(temperature)
    o.eos_id, o.pad_id = int(eos_id), int(pad_id)
    return o


def sample_logits(logits: torch.Tensor, top_k: int = 0, top_p: float = 1.0, temperature: float = 1.0,
                  noise_u: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0):
    """gic_sample_logits: one temperature / top-k / top-p draw per row of f32 logits [rows, V] (rows may be strided).  ``noise_u``
    f32 [rows, V] or None = Philox(seed, stream_id, row).  Returns (ids int64 [rows], logp f32 [rows] = l_tok - logsumexp(l),
    kept int32 [rows] = the size of the kept set)."""
    require_gpu(logits, noise_u)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be float32 [rows, V] with unit column stride")
    rows, V = logits.shape
    if noise_u is not None:
        if tuple(noise_u.shape) != (rows, V) or noise_u.dtype != torch.float32:
            raise ValueError(f"noise_u must be float32 [{rows}, {V}]")
        noise_u = noise_u.contiguous()
    dev = logits.device
    ids = torch.empty(rows, device=dev, dtype=torch.int64)
    logp = torch.empty(rows, device=dev, dtype=torch.float32)
    kept = torch.empty(rows, device=dev, dtype=torch.int32)
    o = sample_opts(1, top_k, top_p, temperature)
    L.check(L.load().gic_sample_logits(ptr(logits), int(logits.stride(0)), int(rows), int(V), C.byref(o), ptr(noise_u),
                                       int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), ptr(ids), ptr(logp), ptr(kept),
                                       stream_ptr()), "gic_sample_logits")
    return ids, logp, kept


def _aligned_ws(ws: Optional[torch.Tensor], nbytes: int, dev) -> torch.Tensor:
    if ws is None or ws.numel() < nbytes or ws.data_ptr() % 256:
        ws = torch.empty(nbytes + 256, device=dev, dtype=torch.uint8)
        off = (-ws.data_ptr()) % 256
        ws = ws[off:off + nbytes]
    return ws


def _decode_features(features: torch.Tensor, E: int) -> torch.Tensor:
    """The decode methods' features: float32 [B, E], contiguous."""
    if tuple(features.shape) != (features.shape[0], E) or features.dtype != torch.float32:
        raise ValueError(f"features must be float32 [B,{E}], got {tuple(features.shape)} {features.dtype}")
    return features.contiguous()


def _decode_states(opts, states, shape, err: str):
    """(h0, c0), each f32 of ``shape``, into opts.h0 / opts.c0 (None: zeros).  Returns the tensors the call reads."""
    if states is None:
        return ()
    h0, c0 = (t.detach().to(torch.float32).contiguous() for t in states)
    if tuple(h0.shape) != shape or tuple(c0.shape) != shape:
        raise ValueError(err)
    require_gpu(h0, c0)
    opts.h0, opts.c0 = ptr(h0), ptr(c0)
    return h0, c0


def _decode_outputs(B: int, n: int, Lc: int, dev):
    """ids int64 [B, n, Lc], scores f32 [B, n], lengths int32 [B, n]."""
    return (torch.empty(B, n, Lc, device=dev, dtype=torch.int64), torch.empty(B, n, device=dev, dtype=torch.float32),
            torch.empty(B, n, device=dev, dtype=torch.int32))


def _diverse_opts(beam_opts, groups: int, diversity: float):
    """gic_diverse_beam_opts around filled gic_decoder_beam_opts (a copy: the library reads h0 / c0 from it)."""
    o = L.DiverseBeamOpts()
    o.beam, o.groups, o.diversity = beam_opts, int(groups), float(diversity)
    return o


def decode_constraints(no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
    """gic_decode_constraints, or None when every constraint is at its default (the caller then runs the unconstrained entry point);
    the library checks the values against the decode's L, V and eos_id."""
    if suppress_tokens is None:
        raise ValueError("suppress_tokens must be a sequence of token ids (empty: none), got None")
    sup = [int(v) for v in suppress_tokens]
    if not int(no_repeat_ngram) and not int(min_length) and not sup:
        return None
    if len(sup) > L.MAX_SUPPRESS:
        raise ValueError(f"suppress_tokens holds {len(sup)} ids, at most {L.MAX_SUPPRESS} (num_suppress)")
    c = L.DecodeConstraints()
    c.no_repeat_ngram, c.min_length, c.num_suppress = int(no_repeat_ngram), int(min_length), len(sup)
    for i, v in enumerate(sup):
        c.suppress[i] = v
    return c


def _constraints_ws(c, rows: int, Lc: int, dev) -> torch.Tensor:
    """The 256-byte aligned workspace of the per-row ban lists (gic_decode_constraints_ws_bytes)."""
    out = C.c_uint64(0)
    L.check(L.load().gic_decode_constraints_ws_bytes(int(rows), int(Lc), C.byref(c), C.byref(out)), "gic_decode_constraints_ws_bytes")
    return _aligned_ws(None, int(out.value), dev)


FORCE_MAX_SETS, FORCE_MAX_IDS = 3, 4          # gic_forced_words: C <= 3 constraint sets per image of D <= 4 ids


def pack_force_words(force_words, B: int) -> torch.Tensor:
    """``force_words`` as the int32 [B, C, D] tensor of gic_forced_words, padded with -1.  Either that tensor already (any device), or
    a list per image of constraints, each an int (one id) or a tuple of ints (a disjunctive set): C = the most constraints of any
    image (at least 1), D = the largest set.  The list form is packed on the host."""
    if isinstance(force_words, torch.Tensor):
        if force_words.dim() != 3 or force_words.shape[0] != B or force_words.dtype != torch.int32:
            raise ValueError(f"force_words must be int32 [B={B}, C, D], got {tuple(force_words.shape)} {force_words.dtype}")
        t = force_words
    else:
        one = lambda c: isinstance(c, numbers.Integral) or (isinstance(c, torch.Tensor) and c.dim() == 0)     # noqa: E731
        per = [[(int(c),) if one(c) else tuple(int(v) for v in c) for c in img] for img in force_words]
        if len(per) != B:
            raise ValueError(f"force_words must hold one list of constraints per image ({B}), got {len(per)}")
        Cn = max([len(img) for img in per] + [1])
        Dn = max([len(c) for img in per for c in img] + [1])
        t = torch.full((B, Cn, Dn), -1, dtype=torch.int32)
        for b, img in enumerate(per):
            for c, ids in enumerate(img):
                if any(v < 0 for v in ids):
                    raise ValueError(f"force_words: image {b}, constraint {c}: id outside [0, V)")
                t[b, c, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    if t.shape[1] > FORCE_MAX_SETS:
        raise ValueError(f"force_words: at most {FORCE_MAX_SETS} constraints per image (C), got {t.shape[1]}")
    if t.shape[2] > FORCE_MAX_IDS:
        raise ValueError(f"force_words: at most {FORCE_MAX_IDS} ids per constraint (D), got {t.shape[2]}")
    if t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError("force_words: C and D must be at least 1")
    return t


_FORCE_CHECKED = [None]      # the last device tensor check_force_words passed, as (storage, version, shape, the check's arguments)


def check_force_words(t: torch.Tensor, V: int, beam: int, eos_id: int, pad_id: int, suppress_tokens=()) -> None:
    """The refusals of a forced search that the library cannot make (the ids live on the device): run on a host copy of the packed
    tensor before anything is launched.  A device tensor costs one blocking device-to-host copy; the same tensor, unmodified since
    (torch's version counter), passed again with the same arguments is not read a second time, so a decode loop that reuses its
    constraint tensor syncs once."""
    key = None
    if t.device.type != "cpu":
        key = (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), int(V), int(beam), int(eos_id), int(pad_id),
               tuple(int(v) for v in suppress_tokens))
        if _FORCE_CHECKED[0] is not None and _FORCE_CHECKED[0][0] is t and _FORCE_CHECKED[0][1] == key:
            return
    _check_force_words_host(t.detach().cpu(), V, beam, eos_id, pad_id, suppress_tokens)
    if key is not None:
        _FORCE_CHECKED[0] = (t, key)


def _check_force_words_host(h: torch.Tensor, V: int, beam: int, eos_id: int, pad_id: int, suppress_tokens=()) -> None:
    B, Cn, Dn = h.shape
    if int(beam) % (1 << Cn):
        raise ValueError(f"force_words: 2^C = {1 << Cn} must divide the beam size {int(beam)}")
    if bool((h < -1).any()) or bool((h >= V).any()):
        raise ValueError(f"force_words: id outside [0, {V}) (-1 pads a set)")
    live = h[h >= 0]
    if live.numel() == 0:
        raise ValueError("force_words: every constraint of every image is absent; use the plain beam search")
    if bool((live == pad_id).any()):
        raise ValueError(f"force_words: <PAD> ({pad_id}) in a constraint")
    if bool((live == eos_id).any()):
        raise ValueError(f"force_words: <E> ({eos_id}) in a constraint")
    sup = set(int(v) for v in suppress_tokens)
    if sup and any(int(v) in sup for v in live.tolist()):
        raise ValueError("force_words: a suppressed id (suppress_tokens) in a constraint")
    s = h.sort(dim=-1).values
    if bool(((s[..., 1:] == s[..., :-1]) & (s[..., 1:] >= 0)).any()):
        raise ValueError("force_words: duplicate id within a constraint")


def _sample_noise(noise_u: Optional[torch.Tensor], Lc: int, rows: int, V: int) -> Optional[torch.Tensor]:
    if noise_u is None:
        return None
    require_gpu(noise_u)
    if tuple(noise_u.shape) != (Lc, rows, V) or noise_u.dtype != torch.float32:
        raise ValueError(f"noise_u must be float32 [L={Lc}, B*n={rows}, V={V}]")
    return noise_u.contiguous()


class _CaptionDecodes:
    """Beam search, diverse beam search and caption sampling of both decoder engines (csrc/decode.hip).  The engine gives the symbol
    prefix and its ``_states``; the attention engine also overrides the two methods through which the feature map and the alphas
    enter a call."""

    _PREFIX = ""                 # gic_decoder / gic_attn

    def _decode_maps(self, fmap, B: int):
        """The inputs a call takes after ``features``."""
        return ()

    def _beam_alphas(self, want: bool, B: int, beam, Lc: int, dev):
        """The outputs a beam search takes after ``lengths`` (a tensor or None each)."""
        return ()

    def _ws_bytes(self, head: str, B: int, Lc: int, n: int) -> int:
        name = f"{self._PREFIX}_{head}_ws_bytes"
        out = C.c_uint64(0)
        L.check(getattr(L.load(), name)(C.byref(self.dims(B, Lc)), int(n), C.byref(out)), name)
        return int(out.value)

    def _decode_call(self, what: str, params, B: int, Lc: int, opts, cons, rows: int, ws, ins, outs, draw=()):
        """<prefix>_<what> of the library, looked up by name at call time.  ``cons`` (set with the constrained forms alone) and its
        workspace follow the options; ``ins``: features and the maps, ``draw``: the sampler's (noise_u pointer, seed), ``outs``: ids to
        lengths / alphas."""
        name = f"{self._PREFIX}_{what}"
        args = [C.byref(self.dims(B, Lc)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(opts)]
        if cons is not None:
            cws = _constraints_ws(cons, rows, Lc, ws.device)
            args += [C.byref(cons), ptr(ws), ptr(cws)]
        else:
            args += [ptr(ws)]
        L.check(getattr(L.load(), name)(*args, *map(ptr, ins), *draw, *map(ptr, outs), stream_ptr()), name)

    def _beam(self, params, features, fmap, Lc, beam, eos_id, pad_id, length_penalty, states, ws, want_alphas, diverse, cons):
        self.check_params(params)
        require_gpu(features, fmap)
        features = _decode_features(features, self.E)
        B, dev = features.shape[0], features.device
        maps = self._decode_maps(fmap, B)
        self.prepare(params)
        ws = _aligned_ws(ws, self.beam_ws_bytes(B, Lc, beam), dev)
        opts = L.DecoderBeamOpts()
        opts.beam, opts.eos_id, opts.pad_id, opts.length_penalty = int(beam), int(eos_id), int(pad_id), float(length_penalty)
        keep = self._states(opts, states, B)                         # (h0, c0): referenced until the call has returned
        outs = _decode_outputs(B, beam, Lc, dev) + self._beam_alphas(want_alphas, B, beam, Lc, dev)
        if cons is not None:
            what, o = "constrained_beam_search", _diverse_opts(opts, *(diverse or (1, 0.0)))
        elif diverse is not None:
            what, o = "diverse_beam_search", _diverse_opts(opts, *diverse)
        else:
            what, o = "beam_search", opts
        self._decode_call(what, params, B, Lc, o, cons, B * int(beam), ws, (features, *maps), outs)
        return outs if want_alphas else outs[:3]

    def forced_beam_ws_bytes(self, B: int, Lc: int, beam: int) -> int:
        """Bytes of gic_*_forced_beam_search's workspace (host-only query)."""
        return self._ws_bytes("forced_beam", B, Lc, beam)

    def _forced_beam(self, params, features, fmap, Lc, beam, eos_id, pad_id, length_penalty, states, ws, want_alphas, force_words, cons,
                     suppress_tokens):
        """gic_*_forced_beam_search (lexically constrained beam search): _beam's outputs plus met int32 [B, beam], the mask of
        constraints each returned beam has met (absent ones set)."""
        self.check_params(params)
        require_gpu(features, fmap)
        features = _decode_features(features, self.E)
        B, dev = features.shape[0], features.device
        force = pack_force_words(force_words, B)
        check_force_words(force, self.V, beam, eos_id, pad_id, suppress_tokens)
        force = force.to(dev).contiguous()
        maps = self._decode_maps(fmap, B)
        self.prepare(params)
        ws = _aligned_ws(ws, self.forced_beam_ws_bytes(B, Lc, beam), dev)
        opts = L.DecoderBeamOpts()
        opts.beam, opts.eos_id, opts.pad_id, opts.length_penalty = int(beam), int(eos_id), int(pad_id), float(length_penalty)
        keep = self._states(opts, states, B)                         # (h0, c0): referenced until the call has returned
        outs = _decode_outputs(B, beam, Lc, dev) + self._beam_alphas(want_alphas, B, beam, Lc, dev)
        met = torch.empty(B, int(beam), device=dev, dtype=torch.int32)
        fw = L.ForcedWords()
        fw.C, fw.D, fw.ids = int(force.shape[1]), int(force.shape[2]), ptr(force)
        name = f"{self._PREFIX}_forced_beam_search"
        cws = _constraints_ws(cons, B * int(beam), Lc, dev) if cons is not None else None
        o = _diverse_opts(opts, 1, 0.0)
        L.check(getattr(L.load(), name)(C.byref(self.dims(B, Lc)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)),
                                        C.byref(o), C.byref(fw), C.byref(cons) if cons is not None else None, ptr(ws), ptr(cws),
                                        *map(ptr, (features, *maps)), *map(ptr, outs), ptr(met), stream_ptr()), name)
        return (outs if want_alphas else outs[:3]) + (met,)

    def _sample(self, params, features, fmap, Lc, num_samples, top_k, top_p, temperature, eos_id, pad_id, seed, noise_u, states, ws, cons):
        self.check_params(params)
        require_gpu(features, fmap)
        features = _decode_features(features, self.E)
        B, dev = features.shape[0], features.device
        n = int(num_samples)
        noise_u = _sample_noise(noise_u, Lc, B * n, self.V)
        opts = sample_opts(n, top_k, top_p, temperature, eos_id, pad_id)
        nbytes = self.sample_ws_bytes(B, Lc, n)          # (checks the dims and n before anything runs)
        maps = self._decode_maps(fmap, B)
        self.prepare(params)
        ws = _aligned_ws(ws, nbytes, dev)
        keep = self._states(opts, states, B)                         # (h0, c0): referenced until the call has returned
        outs = _decode_outputs(B, n, Lc, dev)
        what = "sample_captions" if cons is None else "constrained_sample_captions"
        self._decode_call(what, params, B, Lc, opts, cons, B * n, ws, (features, *maps), outs, (ptr(noise_u), int(seed) & (2 ** 64 - 1)))
        return outs


    # ---- ensemble searches (gic_*_ensemble_*): M members of one decoder kind and dims around one search state
    def _ensemble_ws_bytes(self, head: str, B: int, Lc: int, M: int, n: int) -> int:
        name = f"{self._PREFIX}_ensemble_{head}_ws_bytes"
        out = C.c_uint64(0)
        L.check(getattr(L.load(), name)(C.byref(self.dims(B, Lc)), int(M), int(n), C.byref(out)), name)
        return int(out.value)

    def ensemble_beam_ws_bytes(self, B: int, Lc: int, M: int, beam: int) -> int:
        """Bytes of the ensemble beam search's workspace for M members (host-only query)."""
        return self._ensemble_ws_bytes("beam", B, Lc, M, beam)

    def ensemble_sample_ws_bytes(self, B: int, Lc: int, M: int, num_samples: int) -> int:
        """Bytes of the ensemble sampling decode's workspace for M members (host-only query)."""
        return self._ensemble_ws_bytes("sample", B, Lc, M, num_samples)

    def _ensemble_members(self, members, features, fmaps):
        """Checks the members [(engine, params)] against this engine (member 0's) and prepares them.  Returns (B, dev, the arrays of
        M params / shadow structs / feature / map pointers, everything they point to)."""
        members = list(members)
        M = len(members)
        if not 1 <= M <= L.MAX_ENSEMBLE:
            raise ValueError(f"an ensemble has 1..{L.MAX_ENSEMBLE} members, got {M}")
        if len(features) != M or (fmaps is not None and len(fmaps) != M):
            raise ValueError(f"an ensemble of {M} members needs {M} feature tensors (and feature maps)")
        if members[0][0] is not self:
            raise ValueError("the ensemble's first member must be the engine the search is called on")
        mine = bytes(self.dims(1, 1))
        seen = {}
        for m, (eng, _) in enumerate(members):
            if type(eng) is not type(self) or bytes(eng.dims(1, 1)) != mine:
                raise ValueError(f"ensemble member {m} differs from member 0 in decoder kind, dims or compute dtype")
        for m, (eng, params) in enumerate(members):
            eng.check_params(params)
            if seen.setdefault(id(eng), _key(params)) != _key(params):
                raise ValueError(f"ensemble member {m} shares its engine with another member but not its weights: one engine holds one "
                                 "set of weight images")
        feats = [_decode_features(f, self.E) for f in features]
        B, dev = feats[0].shape[0], feats[0].device
        if any(f.shape[0] != B for f in feats):
            raise ValueError("the members' features differ in batch size")
        require_gpu(*feats, *(fmaps or ()))
        maps = [] if fmaps is None else [self._decode_maps(f, B)[0] for f in fmaps]
        keep = []
        for eng, params in members:
            eng.prepare(params)
            keep.append((eng._pstruct(params), eng._shadow_struct(params)))
        parr = (C.c_void_p * M)(*[C.addressof(p) for p, _ in keep])
        sarr = (C.c_void_p * M)(*[C.addressof(s) for _, s in keep])
        farr = (C.c_void_p * M)(*[ptr(f) for f in feats])
        ins = [farr] + ([(C.c_void_p * M)(*[ptr(f) for f in maps])] if maps else [])
        return M, B, dev, parr, sarr, ins, (keep, feats, maps)

    def _ensemble_call(self, what: str, B, Lc, M, parr, sarr, eopts, opts, cons, rows, ws, ins, outs, draw=()):
        name = f"{self._PREFIX}_ensemble_{what}"
        cws = None if cons is None else _constraints_ws(cons, rows, Lc, ws.device)
        L.check(getattr(L.load(), name)(C.byref(self.dims(B, Lc)), M, parr, sarr, C.byref(eopts), C.byref(opts),
                                        None if cons is None else C.byref(cons), ptr(ws), ptr(cws), *ins, *draw, *map(ptr, outs),
                                        stream_ptr()), name)

    def ensemble_beam_search(self, members, features, fmaps, Lc: int, beam: int, weights=None, mode: str = "prob", groups: int = 1,
                             diversity: float = 0.0, eos_id: int = 2, pad_id: int = 0, length_penalty: float = 0.0,
                             ws: Optional[torch.Tensor] = None, no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
        """gic_*_ensemble_beam_search on this engine (member 0's): ``members`` = [(engine, params)] of one decoder kind, dims and compute
        dtype, ``features`` a list of M f32 [B, E] tensors (``fmaps``: M [B, P, C] tensors for the attention decoder, else None).
        ``weights`` (None: uniform) / ``mode`` ("prob" / "logprob"): ensemble_opts.  Returns (ids int64 [B, beam, Lc], scores f32
        [B, beam], lengths int32 [B, beam]) as beam_search / diverse_beam_search (``groups``, ``diversity``) do; the decode constraints
        as for beam_search."""
        M, B, dev, parr, sarr, ins, keep = self._ensemble_members(members, features, fmaps)
        eopts = ensemble_opts(M, weights, mode)
        cons = decode_constraints(no_repeat_ngram, min_length, suppress_tokens)
        opts = L.DecoderBeamOpts()
        opts.beam, opts.eos_id, opts.pad_id, opts.length_penalty = int(beam), int(eos_id), int(pad_id), float(length_penalty)
        ws = _aligned_ws(ws, self.ensemble_beam_ws_bytes(B, Lc, M, beam), dev)
        outs = _decode_outputs(B, beam, Lc, dev)
        self._ensemble_call("beam_search", B, Lc, M, parr, sarr, eopts, _diverse_opts(opts, groups, diversity), cons, B * int(beam), ws, ins,
                            outs)
        return outs

    def ensemble_sample_captions(self, members, features, fmaps, Lc: int, num_samples: int, weights=None, mode: str = "prob", top_k: int = 0,
                                 top_p: float = 1.0, temperature: float = 1.0, eos_id: int = 2, pad_id: int = 0, seed: int = 0,
                                 noise_u: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, no_repeat_ngram: int = 0,
                                 min_length: int = 0, suppress_tokens=()):
        """gic_*_ensemble_sample_captions: ensemble_beam_search's members, sample_captions' draw on the mixed logits.  Returns (ids int64
        [B, n, Lc], scores f32 [B, n], lengths int32 [B, n]) in row order."""
        M, B, dev, parr, sarr, ins, keep = self._ensemble_members(members, features, fmaps)
        eopts = ensemble_opts(M, weights, mode)
        cons = decode_constraints(no_repeat_ngram, min_length, suppress_tokens)
        n = int(num_samples)
        noise_u = _sample_noise(noise_u, Lc, B * n, self.V)
        opts = sample_opts(n, top_k, top_p, temperature, eos_id, pad_id)
        ws = _aligned_ws(ws, self.ensemble_sample_ws_bytes(B, Lc, M, n), dev)
        outs = _decode_outputs(B, n, Lc, dev)
        self._ensemble_call("sample_captions", B, Lc, M, parr, sarr, eopts, opts, cons, B * n, ws, ins, outs,
                            (ptr(noise_u), int(seed) & (2 ** 64 - 1)))
        return outs


def ensemble_opts(M: int, weights=None, mode: str = "prob") -> L.EnsembleOpts:
    """gic_ensemble_opts: ``weights`` None = uniform, else M finite values > 0 (the library normalises them); ``mode`` "prob" (the
    arithmetic mean of the members' probabilities) or "logprob" (the geometric mean)."""
    if mode not in L.ENSEMBLE_MODES:
        raise ValueError(f"ensemble mode must be one of {sorted(L.ENSEMBLE_MODES)}, got {mode!r}")
    if not 1 <= int(M) <= L.MAX_ENSEMBLE:
        raise ValueError(f"an ensemble has 1..{L.MAX_ENSEMBLE} members, got {M}")
    w = [1.0] * int(M) if weights is None else [float(v) for v in weights]
    if len(w) != int(M):
        raise ValueError(f"ensemble weights: {len(w)} values for {M} members")
    if not all(0.0 < v < float("inf") for v in w):
        raise ValueError("ensemble weights must be finite and > 0")
    o = L.EnsembleOpts()
    o.M, o.mode = int(M), L.ENSEMBLE_MODES[mode]
    for i, v in enumerate(w):
        o.weights[i] = v
    return o


def ensemble_mix(logits: torch.Tensor, weights=None, mode: str = "prob") -> torch.Tensor:
    """gic_ensemble_mix: the members' f32 logits [M, rows, V] -> the ensemble's logits z f32 [rows, V].  With lp_m = log_softmax(l_m),
    "prob": z = log sum_m w_m exp(lp_m); "logprob": z = sum_m w_m lp_m; ``weights`` (None: uniform) are normalised to sum 1."""
    require_gpu(logits)
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("logits must be float32 [M, rows, V]")
    M, rows, V = logits.shape
    o = ensemble_opts(M, weights, mode)
    logits = logits.contiguous()
    out = torch.empty(rows, V, device=logits.device, dtype=torch.float32)
    L.check(L.load().gic_ensemble_mix(ptr(logits), M, rows, V, o.weights, o.mode, ptr(out), stream_ptr()), "gic_ensemble_mix")
    return out


def gan_losses(loss_type: str, d_real, d_fake, g_out, want_grads: bool = True):
    """Returns (losses[2] device tensor: [g_loss, d_loss], grads dict or None)."""
    if loss_type not in L.LOSS_TYPES:
        raise NotImplementedError("Divergence '%s' is not implemented" % loss_type)   # utils.py:50-51
    require_gpu(d_real, d_fake, g_out)
    d_real, d_fake, g_out = d_real.contiguous(), d_fake.contiguous(), g_out.contiguous()
    n = d_real.numel()
    losses = torch.empty(2, device=d_real.device, dtype=torch.float32)
    g = None
    if want_grads:
        buf = torch.empty(5, n, device=d_real.device, dtype=torch.float32)
        g = {"dd_real": buf[0], "dd_fake": buf[1], "dg_out": buf[2], "dg_real": buf[3], "dg_fake": buf[4],
             "dd_real_fake": buf[:2].view(-1)}          # [real ; fake] contiguous: one backward over both passes
    L.check(L.load().gic_gan_losses(L.LOSS_TYPES[loss_type], ptr(d_real), ptr(d_fake), ptr(g_out), n, ptr(losses),
                                    ptr(g["dd_real"]) if g else None, ptr(g["dd_fake"]) if g else None,
                                    ptr(g["dg_out"]) if g else None, ptr(g["dg_real"]) if g else None,
                                    ptr(g["dg_fake"]) if g else None, stream_ptr()), "gic_gan_losses")
    return losses, g


def gan_losses_mismatch(w: float, losses, grads, losses_wrong, grads_wrong):
    """gic_gan_losses_mismatch: d_loss = (1 - w) d(real, fake) + w d(real, wrong) from two ``gan_losses`` evaluations, in place:
    ``losses[1]`` becomes the mix; ``grads["dd_real"]`` / ``["dd_fake"]`` (hence ``["dd_real_fake"]``) the mixed gradients of the real
    and fake logits; ``grads_wrong["dd_fake"]`` the gradient of the wrong-pair logits.  ``grads`` / ``grads_wrong``: both or neither."""
    if (grads is None) != (grads_wrong is None):
        raise ValueError("gan_losses_mismatch: pass the gradients of both evaluations or of neither")
    require_gpu(losses, losses_wrong)
    g, gw = grads or {}, grads_wrong or {}
    L.check(L.load().gic_gan_losses_mismatch(float(w), g["dd_real"].numel() if g else 1, ptr(losses), ptr(losses_wrong), ptr(g.get("dd_real")),
                                             ptr(g.get("dd_fake")), ptr(gw.get("dd_real")), ptr(gw.get("dd_fake")), stream_ptr()),
            "gic_gan_losses_mismatch")
    return losses, grads, grads_wrong


def rerank(lm_scores: torch.Tensor, lengths: torch.Tensor, d_logits: torch.Tensor, R: int, weight: float, length_penalty: float = 0.0,
           ids: Optional[torch.Tensor] = None, alphas: Optional[torch.Tensor] = None):
    """gic_rerank: K candidates per image ordered by lm / max(len,1)^length_penalty + weight * mean_r d_logits (ties to the lower input
    index, NaN last).  lm_scores f32 [B, K], lengths int32 [B, K], d_logits f32 [B*K*R], ids int64 [B, K, L], alphas f32 [B, K, L, P].
    Returns a dict: order int32 [B, K], final / d f32 [B, K] and scores, lengths, ids, alphas (where given), all in the new order."""
    require_gpu(lm_scores, lengths, d_logits, ids, alphas)
    if lm_scores.dim() != 2 or lm_scores.dtype != torch.float32:
        raise ValueError("rerank: scores must be float32 [B, K]")
    B, K = lm_scores.shape
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B, K):
        raise ValueError(f"rerank: lengths must be int32 [B={B}, K={K}]")
    if d_logits.dtype != torch.float32 or d_logits.numel() != B * K * int(R):
        raise ValueError(f"rerank: d_logits must be float32 with B*K*R={B * K * int(R)} elements")
    Lc = P = 0
    if ids is not None:
        if ids.dtype != torch.int64 or ids.dim() != 3 or tuple(ids.shape[:2]) != (B, K):
            raise ValueError(f"rerank: ids must be int64 [B={B}, K={K}, L]")
        Lc = ids.shape[2]
    if alphas is not None:
        if ids is None or alphas.dtype != torch.float32 or alphas.dim() != 4 or tuple(alphas.shape[:3]) != (B, K, Lc):
            raise ValueError(f"rerank: alphas must be float32 [B={B}, K={K}, L={Lc}, P] beside ids")
        P = alphas.shape[3]
    lm_scores, lengths, d_logits = lm_scores.contiguous(), lengths.contiguous(), d_logits.contiguous()
    ids = ids.contiguous() if ids is not None else None
    alphas = alphas.contiguous() if alphas is not None else None
    dev = lm_scores.device
    out = {"order": torch.empty(B, K, device=dev, dtype=torch.int32), "final": torch.empty(B, K, device=dev, dtype=torch.float32),
           "d": torch.empty(B, K, device=dev, dtype=torch.float32), "scores": torch.empty_like(lm_scores), "lengths": torch.empty_like(lengths),
           "ids": torch.empty_like(ids) if ids is not None and Lc else None, "alphas": torch.empty_like(alphas) if alphas is not None and P else None}
    L.check(L.load().gic_rerank(ptr(lm_scores), ptr(lengths), float(length_penalty), ptr(d_logits), int(R), float(weight), ptr(ids), ptr(alphas),
                                B, K, Lc, P, ptr(out["order"]), ptr(out["final"]), ptr(out["d"]), ptr(out["ids"]), ptr(out["scores"]),
                                ptr(out["lengths"]), ptr(out["alphas"]), stream_ptr()), "gic_rerank")
    return out


def match_ranks(S: torch.Tensor, row_bias: Optional[torch.Tensor] = None, N: Optional[int] = None):
    """gic_match_ranks: (rank_c2i, rank_i2c) int32 [N], 0-based, of the pair scores T[c, j] = S[c, j] + row_bias[c]: the number of other
    candidates that are not strictly below the true pair (a tie or a NaN counts against it).  S f32 [>= N, ld] with unit column stride."""
    require_gpu(S, row_bias)
    if S.dim() != 2 or S.dtype != torch.float32 or S.stride(1) != 1:
        raise ValueError("match_ranks: S must be a float32 matrix with unit column stride")
    N = int(S.shape[0] if N is None else N)
    if N > S.shape[0] or N > S.shape[1]:
        raise ValueError(f"match_ranks: N={N} exceeds S {tuple(S.shape)}")
    if row_bias is not None and (row_bias.dtype != torch.float32 or row_bias.numel() < N or not row_bias.is_contiguous()):
        raise ValueError(f"match_ranks: row_bias must be contiguous float32 [N={N}]")
    c2i = torch.empty(max(N, 0), device=S.device, dtype=torch.int32)
    i2c = torch.empty(max(N, 0), device=S.device, dtype=torch.int32)
    L.check(L.load().gic_match_ranks(ptr(S), S.stride(0) if S.shape[0] > 1 else max(S.shape[1], 1), ptr(row_bias), N, ptr(c2i), ptr(i2c),
                                     stream_ptr()), "gic_match_ranks")
    return c2i, i2c


def xent(logits: torch.Tensor, targets: torch.Tensor, want_grad: bool = True, row_weight: Optional[torch.Tensor] = None):
    """CrossEntropyLoss(mean over all rows). logits [rows,V] (f32/bf16, contiguous). Returns (loss[1], d_logits|None).
    ``row_weight`` f32 [rows]: weighted form (policy-gradient loss, gicap.h)."""
    require_gpu(logits, targets, row_weight)
    rows, V = logits.shape
    dt = L.F32 if logits.dtype == torch.float32 else L.BF16
    buf = torch.empty(1 + rows, device=logits.device, dtype=torch.float32)
    dl = torch.empty_like(logits) if want_grad else None
    if row_weight is not None:
        row_weight = row_weight.contiguous().float()
        if row_weight.numel() != rows:
            raise ValueError("row_weight must hold one weight per row")
    L.check(L.load().gic_xent(ptr(logits), dt, rows, V, ptr(targets.contiguous()), ptr(buf), ptr(dl), ptr(row_weight), stream_ptr()),
            "gic_xent")
    return buf[:1], dl


def xent_seq(logits: torch.Tensor, targets: torch.Tensor, group: int, lengths: Optional[torch.Tensor] = None, ignore_index: int = -100,
             smoothing: float = 0.0, row_weight: Optional[torch.Tensor] = None, want_grad: bool = True) -> Dict[str, Optional[torch.Tensor]]:
    """gic_xent_seq: the masked, label-smoothed sequence cross entropy of logits [rows, V] (f32 / bf16, contiguous) against targets int64
    [rows], ``group`` rows per caption.  A row counts when its target is not ``ignore_index`` and, with ``lengths`` int32 [rows / group],
    its position is below its caption's length.  Returns device tensors {"loss": f32 [] (mean over the counted rows; 0 when there are
    none), "count": f32 [], "row_nll": f32 [rows], "cap_nll": f32 [rows / group], "cap_tokens": int32 [rows / group], "d_logits": [rows, V]
    or None}; the per-row / per-caption values are plain negative log-likelihoods (no smoothing, no weight), zero where not counted."""
    require_gpu(logits, targets, lengths, row_weight)
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16) or not logits.is_contiguous():
        raise ValueError("xent_seq: logits must be a contiguous float32 / bfloat16 matrix [rows, V]")
    rows, V = logits.shape
    group = int(group)
    if targets.dtype != torch.int64 or targets.numel() != rows:
        raise ValueError(f"xent_seq: targets must be int64 [rows={rows}]")
    if group < 1 or rows % group:
        raise ValueError(f"xent_seq: group={group} must be at least 1 and divide rows={rows}")
    smoothing = float(smoothing)
    if not 0.0 <= smoothing < 1.0:                  # false for NaN
        raise ValueError(f"xent_seq: smoothing must be in [0, 1), got {smoothing}")
    caps = rows // group
    if lengths is not None:
        if lengths.numel() != caps:
            raise ValueError(f"xent_seq: lengths must hold one value per caption ({caps})")
        lengths = lengths.to(torch.int32).contiguous()
    if row_weight is not None:
        if row_weight.numel() != rows:
            raise ValueError("xent_seq: row_weight must hold one weight per row")
        row_weight = row_weight.contiguous().float()
    dev = logits.device
    dt = L.F32 if logits.dtype == torch.float32 else L.BF16
    loss = torch.empty(2, device=dev, dtype=torch.float32)
    row_buf = torch.empty(2, rows, device=dev, dtype=torch.float32)          # row_nll, the rows' loss terms (scratch)
    cap_nll = torch.empty(caps, device=dev, dtype=torch.float32)
    cap_tokens = torch.empty(caps, device=dev, dtype=torch.int32)
    dl = torch.empty_like(logits) if want_grad else None
    L.check(L.load().gic_xent_seq(ptr(logits), dt, rows, V, ptr(targets.contiguous()), group, ptr(lengths), int(ignore_index), smoothing,
                                  ptr(row_weight), ptr(loss), ptr(row_buf[0]), ptr(row_buf[1]), ptr(cap_nll), ptr(cap_tokens), ptr(dl),
                                  stream_ptr()), "gic_xent_seq")
    return {"loss": loss[0], "count": loss[1], "row_nll": row_buf[0], "cap_nll": cap_nll, "cap_tokens": cap_tokens, "d_logits": dl}


def rollout_rewards(mc_logits: Optional[torch.Tensor], full_logits: torch.Tensor, B: int, Lc: int, N: int, R: int) -> torch.Tensor:
    """gic_rollout_rewards: f32 [B, L] Monte-Carlo rewards from D's logits on the roll-outs (gicap.h)."""
    require_gpu(mc_logits, full_logits)
    out = torch.empty(B, Lc, device=full_logits.device, dtype=torch.float32)
    L.check(L.load().gic_rollout_rewards(ptr(mc_logits), ptr(full_logits.contiguous()), ptr(out), B, Lc, N, R, stream_ptr()),
            "gic_rollout_rewards")
    return out


def _tf_lengths(lengths, B: int, T: int, tmax: Optional[int]):
    """(Tmax, lengths int32) of a teacher-forced decode: max(lengths) read on the host, or with ``tmax`` the device lengths as given
    (each must be in 1..T; not read back)."""
    if tmax is not None:
        if not (torch.is_tensor(lengths) and lengths.is_cuda and lengths.numel() == B) or not 1 <= int(tmax) <= T:
            raise ValueError(f"tmax needs device lengths [{B}] and a value in 1..{T}")
        return int(tmax), lengths.to(torch.int32).contiguous()
    lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lens) != B or min(lens) < 1 or max(lens) > T:
        raise ValueError(f"lengths must hold {B} values in 1..{T}")
    return max(lens), torch.tensor(lens, dtype=torch.int32)


SS_PICKS = ("sample", "argmax")     # gic_sched_sample_opts.pick


def _ss_opts(prob: float, pick: str, coin_u, noise_u, seed: int, B: int, Lc: int, V: int, dev, inputs=None, replaced=None):
    """(gic_sched_sample_opts, inputs int64 [B, L], replaced int32 [B, L], the tensors the struct points into) of a scheduled-sampling
    decode: ``coin_u`` f32 [B, L] and ``noise_u`` f32 [L, B, V] replace the device draws.  ``inputs`` / ``replaced``: the caller's."""
    prob = float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"sample_prob must be in [0, 1], got {prob}")
    if pick not in SS_PICKS:
        raise ValueError(f"pick must be one of {SS_PICKS}, got {pick!r}")
    if coin_u is not None:
        if tuple(coin_u.shape) != (B, Lc):
            raise ValueError(f"coin_u must be [B, L] = [{B}, {Lc}]")
        coin_u = coin_u.contiguous().float()
    if noise_u is not None:
        if tuple(noise_u.shape) != (Lc, B, V):
            raise ValueError(f"noise_u must be [L, B, V] = [{Lc}, {B}, {V}]")
        noise_u = noise_u.contiguous().float()
    inputs = inputs if inputs is not None else torch.empty(B, Lc, device=dev, dtype=torch.int64)
    replaced = replaced if replaced is not None else torch.empty(B, Lc, device=dev, dtype=torch.int32)
    o = L.SchedSampleOpts()
    o.prob, o.pick, o.coin_u, o.noise_u, o.seed = prob, SS_PICKS.index(pick), ptr(coin_u), ptr(noise_u), int(seed) & (2 ** 64 - 1)
    o.inputs, o.replaced = ptr(inputs), ptr(replaced)
    return o, inputs, replaced, (coin_u, noise_u)


def _drop_p(dropout) -> float:
    p = float(dropout)
    if not 0.0 <= p < 1.0:                        # false for NaN too
        raise ValueError(f"dropout must be in [0, 1), got {dropout}")
    return p


def _drop_keep_u(keep_u, shape):
    if keep_u is None:
        return None
    if tuple(keep_u.shape) != tuple(shape):
        raise ValueError(f"keep_u must be {list(shape)}")
    return keep_u.contiguous().float()


def _drop_struct(d) -> L.DecoderDropout:
    """gic_decoder_dropout of what ``saved`` carries: dict(p, seed, keep_u, hdrop)."""
    o = L.DecoderDropout()
    o.p, o.seed, o.keep_u, o.hdrop = d["p"], int(d["seed"]) & (2 ** 64 - 1), ptr(d["keep_u"]), ptr(d["hdrop"])
    return o


def _tf_own(bufs, key: str, shape, dtype, dev, numel_only: bool = False):
    """``bufs[key]`` checked (a caller-owned buffer of a teacher-forced call: contiguous, on ``dev``, of ``dtype`` and ``shape`` -- or
    with ``numel_only`` of at least as many elements), or a fresh tensor where the caller gives none."""
    t = bufs.get(key)
    if t is None:
        return torch.empty(*shape, device=dev, dtype=dtype)
    n = 1
    for v in shape:
        n *= int(v)
    fits = torch.is_tensor(t) and (t.numel() >= n if numel_only else tuple(t.shape) == tuple(int(v) for v in shape))
    if not (fits and t.device == dev and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"buffers[{key!r}] must be a contiguous {dtype} tensor {list(shape)} on {dev}")
    return t


def hidden_dropout(x: torch.Tensor, p: float, seed: int = 0, keep_u: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """gic_hidden_dropout, the forward stage of the decoder's output dropout on its own: y = keep ? x * s : 0 with s = 1 / (1 - p) in
    f32 over ``x`` f32 or bf16 [..., H] (contiguous; any H, any alignment), element (r, h) of the [rows, H] view drawn at the flat
    index r * H + h from Philox(``seed``) or read from ``keep_u`` f32 of x's shape.  ``out``: a contiguous tensor of x's shape and dtype."""
    require_gpu(x, keep_u, out)
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() < 1 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float32 or bfloat16 tensor [..., H]")
    keep_u = _drop_keep_u(keep_u, x.shape)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("out must be contiguous with x's shape and dtype")
    H = x.shape[-1]
    L.check(L.load().gic_hidden_dropout(ptr(x), L.F32 if x.dtype == torch.float32 else L.BF16, x.numel() // max(H, 1), H, float(p),
                                        int(seed) & (2 ** 64 - 1), ptr(keep_u), ptr(out), stream_ptr()), "gic_hidden_dropout")
    return out


def hidden_dropout_bwd(dhout: torch.Tensor, lengths, p: float, seed: int = 0, keep_u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gic_hidden_dropout_bwd, in place on ``dhout`` f32 [B, Tmax, H] (contiguous): dhout = (t < lengths[b] && keep) ? dhout * s : 0 with
    the mask of ``hidden_dropout(x [B, Tmax, H], p, seed, keep_u)``.  ``lengths``: B values.  Returns ``dhout``."""
    require_gpu(dhout, keep_u)
    if dhout.dtype != torch.float32 or dhout.dim() != 3 or not dhout.is_contiguous():
        raise ValueError("dhout must be a contiguous float32 tensor [B, Tmax, H]")
    B, Tmax, H = dhout.shape
    keep_u = _drop_keep_u(keep_u, dhout.shape)
    lens = torch.as_tensor(lengths).to(device=dhout.device, dtype=torch.int32).contiguous()
    if lens.numel() != B:
        raise ValueError(f"lengths must hold {B} values")
    L.check(L.load().gic_hidden_dropout_bwd(ptr(dhout), ptr(lens), B, Tmax, H, float(p), int(seed) & (2 ** 64 - 1), ptr(keep_u),
                                            stream_ptr()), "gic_hidden_dropout_bwd")
    return dhout


def step_part_floats(B: int, Lc: int, V: int) -> int:
    """Floats of the fused step kernels' scratch (state ``part``): [2][L][B][ceil(V/64)] tile partials + [L][B] 64-bit argmax keys +
    four reserved words -- decoder_step_part_floats of csrc/decoder_step.hip, the one owner of the layout (= gic_decoder_state_bytes'
    figure)."""
    return 2 * Lc * B * ((V + 63) // 64) + 2 * Lc * B + 4


class _TeacherForced:
    """forward_tf, forward_scheduled and forward_tf_bwd of both decoder engines (csrc/teacher_forced.hip).  The engine gives the symbol
    prefix, ``NL`` (the leading dimension of the final states), ``_decode_maps`` (the feature map: the inputs a call takes after
    ``features``), ``_tf_check_inputs(features, caps, B)`` (its own shape / dtype check and text), ``_tf_ws(B, T, Tmax, dev)`` (the
    workspace tensors of the plain call, in argument order), ``_bwd_ws_struct(ws)`` and ``_GRADS`` (the backward's structs) and the
    hooks below; its public methods keep their own signatures and pass what they lack as None."""

    _TF_BWD_WS_STEPS = "Tmax"    # the key of ``saved`` that sizes a backward workspace allocated here

    def _tf_alphas(self, want: bool, B: int, Tmax: int, dev):
        """The outputs a forward call takes after ``out`` (a tensor or None each); they follow (h_n, c_n) in what it returns."""
        return ()

    def _tf_d_alphas(self, d_alphas, B: int, Tmax: int):
        """The gradients a backward call takes after ``d_pred``."""
        return ()

    def alloc_grads(self, params, B: int) -> List[torch.Tensor]:
        """[one gradient per parameter, in the parameters' order ..., d_features]"""
        return [torch.empty_like(p) for p in params] + [torch.empty(B, self.E, device=params[0].device, dtype=torch.float32)]

    def _tf_forward(self, params, features, fmap, caps, lengths, tmax, state, want_alphas, ss, noise_u=None, seed=0, temperature=1.0,
                    pretrain=True, drop=(0.0, 0, None), bufs=None):
        """``ss``: None, or _ss_opts' arguments but the shapes (prob, pick, coin_u, noise_u, seed) -- then the scheduled-sampling call.
        ``bufs``: None, or a dict of caller-owned buffers that stand in for what is allocated here (each optional): ``out``, ``h_n``,
        ``c_n``, ``hdrop`` (16-byte aligned), ``ws`` (the workspace tensors of the plain call in argument order, or the one f32 tensor
        of the scheduled-sampling call, 16-byte aligned and at least *_forward_ss_ws_bytes large), ``inputs``, ``replaced``.
        ``drop``: (dropout, dropout_seed, keep_u) -- with dropout > 0 the gic_*_drop form of the call, whose ``hdrop`` is allocated
        here and carried in ``saved["drop"]`` with (p, seed, keep_u) for the backward.
        Returns (pred, (h_n, c_n), *alphas), saved[, inputs, replaced]."""
        self.check_params(params)
        drop_p = _drop_p(drop[0])
        require_gpu(features, fmap, caps, noise_u, *(ss[2:4] if ss else ()), *((drop[2],) if drop_p > 0.0 else ()))
        B, Lc = caps.shape
        T = Lc + 1
        Tmax, len_dev = _tf_lengths(lengths, B, T, tmax)
        self._tf_check_inputs(features, caps, B)
        if noise_u is not None:
            if tuple(noise_u.shape) != (B, Tmax, self.V):
                raise ValueError(f"noise_u must be [B, max(lengths)={Tmax}, V]")
            noise_u = noise_u.contiguous().float()
        maps = self._decode_maps(fmap, B)
        dev = features.device
        bufs = bufs or {}
        if ss:
            o, inputs, replaced, keep = _ss_opts(*ss, B, Lc, self.V, dev, _tf_own(bufs, "inputs", (B, Lc), torch.int64, dev),
                                                 _tf_own(bufs, "replaced", (B, Lc), torch.int32, dev))
        self.prepare(params)
        st = dict(state) if state is not None else self.alloc_state(B, T, dev)
        out = _tf_own(bufs, "out", (B, Tmax, self.V), self.act, dev)
        h_n = _tf_own(bufs, "h_n", (self.NL, B, self.H), torch.float32, dev)
        c_n = _tf_own(bufs, "c_n", (self.NL, B, self.H), torch.float32, dev)
        alphas = self._tf_alphas(want_alphas, B, Tmax, dev)
        d = self.dims(B, T)
        if ss:
            name, nbytes = f"{self._PREFIX}_forward_ss", C.c_uint64(0)
            L.check(getattr(L.load(), name + "_ws_bytes")(C.byref(d), Tmax, C.byref(nbytes)), name + "_ws_bytes")
            ws = (_tf_own(bufs, "ws", (max(int(nbytes.value) // 4, 1),), torch.float32, dev, numel_only=True),)
            mode = (C.byref(o),)
        else:
            name, ws = f"{self._PREFIX}_forward_tf", self._tf_ws(B, T, Tmax, dev)
            if bufs.get("ws") is not None:
                own = tuple(bufs["ws"])
                if len(own) != len(ws) or any(not (a.device == b.device and a.dtype == b.dtype and a.is_contiguous() and a.numel() >= b.numel())
                                              for a, b in zip(own, ws)):
                    raise ValueError("buffers['ws'] must hold the call's workspace tensors: " + ", ".join(f"{b.dtype} x {b.numel()}" for b in ws))
                ws = own
            mode = (ptr(noise_u), int(seed) & (2 ** 64 - 1), float(temperature), int(bool(pretrain)))
        dropped = None
        if drop_p > 0.0:         # hdrop is the call's own: gic_decoder_state_bytes pins the state's list
            dropped = {"p": drop_p, "seed": int(drop[1]), "keep_u": _drop_keep_u(drop[2], (B, Tmax, self.H)),
                       "hdrop": _tf_own(bufs, "hdrop", (B, Tmax, self.H), self.act, dev)}
            name += "_drop"
        tail = (C.byref(_drop_struct(dropped)),) if dropped else ()
        len_dev, caps = len_dev.to(dev), caps.contiguous()
        L.check(getattr(L.load(), name)(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            ptr(features.contiguous().float()), *map(ptr, maps), ptr(caps), ptr(len_dev), Tmax, *mode, *map(ptr, ws), ptr(out),
            *map(ptr, alphas), ptr(h_n), ptr(c_n), *tail, stream_ptr()), name)
        if maps:
            st["fmap"] = maps[0]
        saved = {"st": st, "caps": inputs if ss else caps, "len_dev": len_dev, "Tmax": Tmax, "T": T}
        if dropped:
            saved["drop"] = dropped
        return (out, (h_n, c_n), *alphas), saved, *((inputs, replaced) if ss else ())

    def _tf_backward(self, params, saved, pred, d_pred, d_alphas, temperature, pretrain, ws, grads, drop=(0.0, 0, None)):
        """``drop``: (dropout, dropout_seed, keep_u); with dropout > 0 they stand in for what ``saved`` carries (the forward call must
        have dropped: ``saved`` holds its hdrop), with 0 the forward call's own values are used."""
        B, Tmax, dev = pred.shape[0], saved["Tmax"], pred.device
        dropped = saved.get("drop")
        if _drop_p(drop[0]) > 0.0:
            if dropped is None:
                raise ValueError("forward_tf_bwd: dropout given, but the forward call that returned `saved` ran without it")
            require_gpu(drop[2])
            dropped = dict(dropped, p=float(drop[0]), seed=int(drop[1]), keep_u=_drop_keep_u(drop[2], (B, Tmax, self.H)))
        if d_pred is None:
            d_pred = torch.zeros(pred.shape, device=dev, dtype=self.act)
        if tuple(d_pred.shape) != tuple(pred.shape):
            raise ValueError("d_pred must have pred's shape")
        d_pred = _to_act(d_pred, self.act)
        d_alphas = self._tf_d_alphas(d_alphas, B, Tmax)
        self.prepare(params)
        ws = ws if ws is not None else self.alloc_bwd_ws(B, saved[self._TF_BWD_WS_STEPS], dev)
        grads = grads if grads is not None else self.alloc_grads(params, B)
        name = f"{self._PREFIX}_forward_tf_drop_bwd" if dropped else f"{self._PREFIX}_forward_tf_bwd"
        tail = (C.byref(_drop_struct(dropped)),) if dropped else ()
        st = saved["st"]
        L.check(getattr(L.load(), name)(
            C.byref(self.dims(B, saved["T"])), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)),
            C.byref(self._state_struct(st)), C.byref(self._bwd_ws_struct(ws)), *map(ptr, self._decode_maps(st.get("fmap"), B)), ptr(pred),
            ptr(saved["caps"]), ptr(saved["len_dev"]), Tmax, ptr(d_pred), *map(ptr, d_alphas), float(temperature), int(bool(pretrain)),
            C.byref(self._pstruct(grads[:-1], self._GRADS, grads[-1])), *tail, stream_ptr()), name)
        return grads


def cider_d(cand_ids: torch.Tensor, cand_len: torch.Tensor, cand_img: torch.Tensor, ref_ids: torch.Tensor, ref_len: torch.Tensor,
            ref_off: torch.Tensor, max_refs: int, keys: torch.Tensor, idf: torch.Tensor, log_n: float, V: int) -> torch.Tensor:
    """gic_cider_d: CIDEr-D f32 [n_cand] of candidates int64 [n_cand, Lc] (cand_len / cand_img int32 [n_cand]) against the references
    int64 [n_ref, Lr] (ref_len int32 [n_ref]; image b owns rows ref_off[b] .. ref_off[b+1], int32 [B+1]), with the document-frequency
    table keys int64 [K] (the uint64 keys of gicap.h, all below 2^62) / idf f32 [K].  ``max_refs``: the largest reference count of
    one image (host-known).  One launch, no host sync."""
    require_gpu(cand_ids, cand_len, cand_img, ref_ids, ref_len, ref_off, keys, idf)
    if cand_ids.dim() != 2 or ref_ids.dim() != 2 or cand_ids.dtype != torch.int64 or ref_ids.dtype != torch.int64:
        raise ValueError("cand_ids and ref_ids must be int64 [rows, L]")
    n_cand, Lc = cand_ids.shape
    n_ref, Lr = ref_ids.shape
    B = ref_off.numel() - 1
    i32 = lambda t: t.to(torch.int32).contiguous()        # noqa: E731
    cand_ids, ref_ids = cand_ids.contiguous(), ref_ids.contiguous()
    cand_len, cand_img, ref_len, ref_off = i32(cand_len), i32(cand_img), i32(ref_len), i32(ref_off)
    if cand_len.numel() != n_cand or cand_img.numel() != n_cand or ref_len.numel() != n_ref:
        raise ValueError("cand_len / cand_img need one value per candidate and ref_len one per reference")
    scores = torch.empty(n_cand, device=cand_ids.device, dtype=torch.float32)
    L.check(L.load().gic_cider_d(ptr(cand_ids), Lc, ptr(cand_len), ptr(cand_img), n_cand, Lc, ptr(ref_ids), Lr, ptr(ref_len), ptr(ref_off),
                                 n_ref, Lr, B, int(max_refs), ptr(keys.contiguous()), ptr(idf.contiguous()), keys.numel(), float(log_n),
                                 int(V), ptr(scores), stream_ptr()), "gic_cider_d")
    return scores


def cider_pairwise(ids: torch.Tensor, lengths: torch.Tensor, keys: torch.Tensor, idf: torch.Tensor, log_n: float, V: int,
                   want_matrix: bool = True, want_consensus: bool = True, want_self_cider: bool = True) -> dict:
    """gic_cider_pairwise: CIDEr-D among the K captions of each image, ids int64 [B, K, L] with lengths int [B, K], under the
    document-frequency table of ``cider_d``.  Returns {"matrix": f32 [B, K, K] (caption i as the candidate against caption j as the
    single reference), "consensus": f32 [B, K] (the row mean without the diagonal), "self_cider": f32 [B]}; an output that is not
    wanted is None and is not computed.  One launch, no host sync."""
    require_gpu(ids, lengths, keys, idf)
    if ids.dim() != 3 or ids.dtype != torch.int64:
        raise ValueError("cider_pairwise: ids must be int64 [B, K, L]")
    B, K, Lc = ids.shape
    if tuple(lengths.shape) != (B, K):
        raise ValueError(f"cider_pairwise: lengths must be [B={B}, K={K}]")
    if not (want_matrix or want_consensus or want_self_cider):
        raise ValueError("cider_pairwise: no output wanted")
    ids, lengths, dev = ids.contiguous(), lengths.to(torch.int32).contiguous(), ids.device
    out = {"matrix": torch.empty(B, K, K, device=dev, dtype=torch.float32) if want_matrix else None,
           "consensus": torch.empty(B, K, device=dev, dtype=torch.float32) if want_consensus else None,
           "self_cider": torch.empty(B, device=dev, dtype=torch.float32) if want_self_cider else None}
    L.check(L.load().gic_cider_pairwise(ptr(ids), Lc, ptr(lengths), B, K, Lc, ptr(keys.contiguous()), ptr(idf.contiguous()), keys.numel(),
                                        float(log_n), int(V), ptr(out["matrix"]), ptr(out["consensus"]), ptr(out["self_cider"]),
                                        stream_ptr()), "gic_cider_pairwise")
    return out


def caption_overlap(cand_ids: torch.Tensor, cand_len: torch.Tensor, cand_img: torch.Tensor, ref_ids: torch.Tensor, ref_len: torch.Tensor,
                    ref_off: torch.Tensor, max_refs: int, V: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gic_caption_overlap: (stats int32 [n_cand, 10], ROUGE-L f32 [n_cand], smoothed sentence BLEU-4 f32 [n_cand]) of candidates int64
    [n_cand, Lc] against the references, both laid out as for ``cider_d``; the stats columns are the per-candidate integers of corpus
    BLEU-1..4 (gicap.h).  One launch, no host sync."""
    require_gpu(cand_ids, cand_len, cand_img, ref_ids, ref_len, ref_off)
    if cand_ids.dim() != 2 or ref_ids.dim() != 2 or cand_ids.dtype != torch.int64 or ref_ids.dtype != torch.int64:
        raise ValueError("cand_ids and ref_ids must be int64 [rows, L]")
    n_cand, Lc = cand_ids.shape
    n_ref, Lr = ref_ids.shape
    B = ref_off.numel() - 1
    i32 = lambda t: t.to(torch.int32).contiguous()        # noqa: E731
    cand_ids, ref_ids = cand_ids.contiguous(), ref_ids.contiguous()
    cand_len, cand_img, ref_len, ref_off = i32(cand_len), i32(cand_img), i32(ref_len), i32(ref_off)
    if cand_len.numel() != n_cand or cand_img.numel() != n_cand or ref_len.numel() != n_ref:
        raise ValueError("cand_len / cand_img need one value per candidate and ref_len one per reference")
    dev = cand_ids.device
    stats = torch.empty(n_cand, L.OVERLAP_STATS, device=dev, dtype=torch.int32)
    rouge = torch.empty(n_cand, device=dev, dtype=torch.float32)
    sbleu = torch.empty(n_cand, device=dev, dtype=torch.float32)
    L.check(L.load().gic_caption_overlap(ptr(cand_ids), Lc, ptr(cand_len), ptr(cand_img), n_cand, Lc, ptr(ref_ids), Lr, ptr(ref_len),
                                         ptr(ref_off), n_ref, Lr, B, int(max_refs), int(V), ptr(stats), ptr(rouge), ptr(sbleu),
                                         stream_ptr()), "gic_caption_overlap")
    return stats, rouge, sbleu


# ------------------------------------------------------------------------------------------ decoder
class DecoderEngine(_CaptionDecodes, _TeacherForced):
    """Decoder.sample forward/backward (reference src/generator.py:55-96) on the HIP library."""

    _GRADS = L.DecoderGrads

    def __init__(self, vocab: int, embed: int, hidden: int, layers: int, dtype: int):
        if not 1 <= layers <= L.MAX_LAYERS:
            raise ValueError(f"gen_num_layers must be in 1..{L.MAX_LAYERS}")
        self.V, self.E, self.H, self.NL, self.dt = vocab, embed, hidden, layers, dtype
        self.act = TORCH_DTYPE[dtype]
        self._shadow: Optional[Dict[str, object]] = None
        self._shadow_key = None

    def din(self, l: int) -> int:
        return self.E if l == 0 else self.H

    def ldx(self, l: int) -> int:
        return self.din(l) + self.H

    def dims(self, B: int, Lc: int) -> L.DecoderDims:
        return L.DecoderDims(B, Lc, self.V, self.E, self.H, self.NL, self.dt)

    # params: [embed, (w_ih, w_hh, b_ih, b_hh) * NL, w_out, b_out]
    def plan(self, B: int, Lc: int, train: bool = True, pretrain: bool = False, dev_scalars: bool = False, resumed: bool = False,
             part: bool = True, transposed_images: bool = True, state_grads: bool = False, logits_aligned: bool = True):
        """gic_debug_decoder_plan: what sample_fwd / sample_bwd select for these shapes -- the forward's path and its per-step launches
        and, with `train`, the backward's -- as lines (gicap.h).  Host-only."""
        flags = (L.DECODER_PLAN_TRAIN if train else 0) | (L.DECODER_PLAN_PRETRAIN if pretrain else 0) | \
                (L.DECODER_PLAN_DEV_SCALARS if dev_scalars else 0) | (L.DECODER_PLAN_RESUMED if resumed else 0) | \
                (0 if part else L.DECODER_PLAN_NO_PART) | (0 if transposed_images else L.DECODER_PLAN_NO_WCAT_T) | \
                (L.DECODER_PLAN_STATE_GRADS if state_grads else 0) | (0 if logits_aligned else L.DECODER_PLAN_LOGITS_UNALIGNED)
        out = C.create_string_buffer(4096)
        L.check(L.load().gic_debug_decoder_plan(C.byref(self.dims(B, Lc)), flags, out, len(out)), "gic_debug_decoder_plan")
        return out.value.decode().splitlines()

    def _pstruct(self, params, cls=L.DecoderParams, extra=None):
        nl = self.NL
        s = cls()
        s.embed = ptr(params[0])
        s.w_ih = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(params[1 + 4 * l]) for l in range(nl)])
        s.w_hh = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(params[2 + 4 * l]) for l in range(nl)])
        s.b_ih = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(params[3 + 4 * l]) for l in range(nl)])
        s.b_hh = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(params[4 + 4 * l]) for l in range(nl)])
        s.w_out = ptr(params[1 + 4 * nl])
        s.b_out = ptr(params[2 + 4 * nl])
        if extra is not None:
            s.features = ptr(extra)
        return s

    def check_params(self, params) -> None:
        if len(params) != 3 + 4 * self.NL:
            raise ValueError("decoder expects embed, 4 tensors per LSTM layer, linear weight and bias")
        require_gpu(*params)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("decoder parameters must be contiguous float32 (master weights)")

    def prepare(self, params) -> Dict[str, object]:
        """Refresh the compute-dtype weight images if any master weight changed."""
        key = _key(params)
        if self._shadow is not None and key == self._shadow_key:
            return self._shadow
        dev = params[0].device
        if self._shadow is None or self._shadow["wcat"][0].device != dev:
            self._shadow = {
                "wcat": [torch.empty(4 * self.H, self.ldx(l), device=dev, dtype=self.act) for l in range(self.NL)],
                "bsum": [torch.empty(4 * self.H, device=dev, dtype=torch.float32) for l in range(self.NL)],
                "wout": None if self.dt == L.F32 else torch.empty(self.V, self.H, device=dev, dtype=self.act),
                # Wcat^T: the k-contiguous weight operand of the BPTT products d[x|h] = d_gates Wcat (fused BPTT step kernel)
                "wcat_t": [torch.empty(self.ldx(l), 4 * self.H, device=dev, dtype=self.act) for l in range(self.NL)],
            }
        sh = self._shadow
        s = self._shadow_struct(params)
        d = self.dims(1, 1)
        L.check(L.load().gic_decoder_prepare(C.byref(d), C.byref(self._pstruct(params)), C.byref(s), stream_ptr()),
                "gic_decoder_prepare")
        self._shadow_key = key
        return sh

    def _shadow_struct(self, params) -> L.DecoderShadow:
        sh = self._shadow
        s = L.DecoderShadow()
        s.wcat = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in sh["wcat"]])
        s.bsum = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in sh["bsum"]])
        s.wout = ptr(params[1 + 4 * self.NL]) if sh["wout"] is None else ptr(sh["wout"])
        if sh["wcat_t"] is not None:
            s.wcat_t = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in sh["wcat_t"]])
        return s

    def alloc_state(self, B: int, Lc: int, dev) -> Dict[str, object]:
        f32 = torch.float32
        return {
            "xh": [torch.empty(Lc + 1, B, self.ldx(l), device=dev, dtype=self.act) for l in range(self.NL)],
            "gates": [torch.empty(Lc, B, 4 * self.H, device=dev, dtype=f32) for _ in range(self.NL)],
            "c": [torch.empty(Lc + 1, B, self.H, device=dev, dtype=f32) for _ in range(self.NL)],
            "hout": torch.empty(B, Lc, self.H, device=dev, dtype=self.act),
            "logits": torch.empty(B, self.V, device=dev, dtype=f32),
            "gpre": torch.empty(B, 4 * self.H, device=dev, dtype=f32),
            # per-tile softmax partials of the fused step kernels ([3][L][B][ceil(V/64)], decoder_step.h)
            "part": torch.empty(self.part_floats(B, Lc), device=dev, dtype=f32),
        }

    def part_floats(self, B: int, Lc: int) -> int:
        return step_part_floats(B, Lc, self.V)

    def fused_rollout_rows(self) -> int:
        """Largest batch the fused step kernels take for this decoder's shapes; 0: they decline them (gic_decoder_fused_rollout_rows:
        the library's own path selection, so buffer planning here cannot disagree with it)."""
        out = C.c_int32(0)
        L.check(L.load().gic_decoder_fused_rollout_rows(C.byref(self.dims(1, 1)), C.byref(out)), "gic_decoder_fused_rollout_rows")
        return int(out.value)

    def alloc_rollout_state(self, B: int, Lc: int, dev) -> Dict[str, object]:
        """State of an inference roll-out (``no_state``): recurrent buffers only, nothing saved for a backward pass."""
        f32 = torch.float32
        fused = B <= self.fused_rollout_rows()
        return {
            "xh": [torch.empty(Lc + 1, B, self.ldx(l), device=dev, dtype=self.act) for l in range(self.NL)],
            "gates": [None] * self.NL,
            "c": [torch.empty(Lc + 1, B, self.H, device=dev, dtype=f32) for _ in range(self.NL)],
            "hout": None,
            # where the fused step kernels decline (row limit, V % 4, E % 8, H % 8) the roll-out runs as generic products: their scratch
            "logits": None if fused else torch.empty(B, self.V, device=dev, dtype=f32),
            "gpre": None if fused else torch.empty(B, 4 * self.H, device=dev, dtype=f32),
            "part": torch.empty(self.part_floats(B, Lc), device=dev, dtype=f32) if fused else None,
        }

    def _state_struct(self, st) -> L.DecoderState:
        s = L.DecoderState()
        s.xh = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in st["xh"]])
        s.gates = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in st["gates"]])
        s.c = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in st["c"]])
        s.hout, s.logits, s.gpre = ptr(st["hout"]), ptr(st["logits"]), ptr(st["gpre"])
        s.part = ptr(st.get("part"))
        return s

    def alloc_bwd_ws(self, B: int, Lc: int, dev) -> Dict[str, object]:
        f32 = torch.float32
        return {
            "dlogits": torch.empty(B, Lc, self.V, device=dev, dtype=self.act),
            "dhout": torch.empty(B, Lc, self.H, device=dev, dtype=f32),
            "dgates": [torch.empty(Lc, B, 4 * self.H, device=dev, dtype=self.act) for _ in range(self.NL)],
            "dxh": [torch.empty(Lc + 1, B, self.ldx(l), device=dev, dtype=f32) for l in range(self.NL)],
            "dc": [torch.empty(B, self.H, device=dev, dtype=f32) for _ in range(self.NL)],
        }

    def _bwd_ws_struct(self, ws) -> L.DecoderBwdWs:
        w = L.DecoderBwdWs()
        w.dlogits, w.dhout = ptr(ws["dlogits"]), ptr(ws["dhout"])
        w.dgates = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in ws["dgates"]])
        w.dxh = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in ws["dxh"]])
        w.dc = _arr(C.c_void_p, L.MAX_LAYERS, [ptr(t) for t in ws["dc"]])
        return w

    def sample_fwd(self, params, features: torch.Tensor, Lc: int, temperature: float, pretrain: bool = False,
                   noise_u: Optional[torch.Tensor] = None, seed: int = 0, state=None, out=None, ids=None,
                   states=None, force_ids: Optional[torch.Tensor] = None, force_len: Optional[torch.Tensor] = None,
                   ids_only: bool = False, resume=None, dev_scalars=None, seed_slot: int = 0):
        """``dev_scalars`` (StepScalarsBuffer) / ``seed_slot``: temperature and seed are read from device memory (gicap.h
        gic_step_scalars; fused step kernels only).  ``states`` = (h0, c0), each f32 [NL, B, H] (generator.py:55,61).  ``force_ids`` int64 [B, L] (+ ``force_len`` int32 [B]):
        trajectory to follow (gicap.h).  ``ids_only``: inference roll-out, returns (None, ids, state) and saves nothing for backward.
        ``resume`` = (state of an earlier call, its batch size, active_rows list[L]): resumed roll-outs (gicap.h,
        gic_decoder_sample_opts.resume_from) -- rows sorted by prefix length, each starting at its prefix from that call's state."""
        self.check_params(params)
        require_gpu(features, noise_u, force_ids, force_len)
        B = features.shape[0]
        if features.shape != (B, self.E) or features.dtype != torch.float32:
            raise ValueError(f"features must be float32 [B,{self.E}], got {tuple(features.shape)} {features.dtype}")
        features = features.contiguous()
        dev = features.device
        if noise_u is not None:
            if tuple(noise_u.shape) != (Lc, B, self.V) or noise_u.dtype != torch.float32:
                raise ValueError(f"noise_u must be float32 [L={Lc},B={B},V={self.V}]")
            noise_u = noise_u.contiguous()
        self.prepare(params)
        if state is not None:
            st = state
        else:
            st = self.alloc_rollout_state(B, Lc, dev) if ids_only else self.alloc_state(B, Lc, dev)
        if not ids_only:
            out = out if out is not None else torch.empty(B, Lc, self.V, device=dev, dtype=self.act)
        ids = ids if ids is not None else torch.empty(B, Lc, device=dev, dtype=torch.int64)
        opts = None
        keep = []
        if states is not None or force_ids is not None or ids_only or dev_scalars is not None:
            opts = L.DecoderSampleOpts()
            if dev_scalars is not None:
                opts.dev_scalars, opts.seed_slot = dev_scalars.ptr, int(seed_slot)
            if states is not None:
                h0, c0 = (t.detach().to(torch.float32).contiguous() for t in states)
                if tuple(h0.shape) != (self.NL, B, self.H) or tuple(c0.shape) != (self.NL, B, self.H):
                    raise ValueError(f"states must be (h0, c0), each [num_layers={self.NL}, B={B}, H={self.H}]")
                require_gpu(h0, c0)
                opts.h0, opts.c0 = ptr(h0), ptr(c0)
                keep += [h0, c0]
            if force_ids is not None:
                if tuple(force_ids.shape) != (B, Lc) or force_ids.dtype != torch.int64:
                    raise ValueError(f"force_ids must be int64 [B={B}, L={Lc}]")
                force_ids = force_ids.contiguous()
                opts.force_ids = ptr(force_ids)
                if force_len is not None:
                    force_len = force_len.to(torch.int32).contiguous()
                    if tuple(force_len.shape) != (B,):
                        raise ValueError("force_len must hold one prefix length per caption")
                    opts.force_len = ptr(force_len)
                keep += [force_ids, force_len]
            opts.no_state = int(bool(ids_only))
        if resume is not None:
            src_state, src_B, active = resume
            if len(active) != Lc or force_ids is None or force_len is None or not ids_only or st.get("logits") is None:
                raise ValueError("resumed roll-outs: active_rows per step, force_ids, force_len, ids_only and a state with the generic "
                                 "products' scratch (more rows than the fused step kernels take)")
            src_struct = self._state_struct(src_state)
            act = _arr(C.c_int32, Lc, [int(v) for v in active])
            opts.resume_from = C.cast(C.pointer(src_struct), C.c_void_p)
            opts.resume_B = int(src_B)
            opts.host_active_rows = C.cast(act, C.c_void_p)
            keep += [src_struct, act]
        d = self.dims(B, Lc)
        L.check(L.load().gic_decoder_sample_fwd(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            ptr(features), ptr(noise_u), int(seed) & (2 ** 64 - 1), float(temperature), int(bool(pretrain)), ptr(out) if not ids_only else None,
            ptr(ids), C.byref(opts) if opts is not None else None, stream_ptr()), "gic_decoder_sample_fwd")
        return (None if ids_only else out), ids, st

    def forward_tf(self, params, features: torch.Tensor, caps: torch.Tensor, lengths, temperature: float, pretrain: bool = False,
                   noise_u: Optional[torch.Tensor] = None, seed: int = 0, keep_state: bool = False, tmax: Optional[int] = None,
                   state=None, buffers=None, dropout: float = 0.0, dropout_seed: int = 0, keep_u: Optional[torch.Tensor] = None):
        """gic_decoder_forward_tf: Decoder.forward (teacher forcing, generator.py:39-53).
        Returns (pred act [B, max(lengths), V], (h_n, c_n) f32 [NL, B, H]); with ``keep_state`` also what ``forward_tf_bwd`` needs.
        ``tmax``: decode that many steps and take ``lengths`` as device int32 values in 1..T unread (no host sync); pred is then
        [B, tmax, V].  ``dropout`` p > 0: output dropout (gic_decoder_forward_tf_drop) -- the LSTM output is dropped with probability p
        in front of the vocabulary projection, by Philox(``dropout_seed``) or ``keep_u`` f32 [B, max(lengths), H] (keep = u >= p); the
        recurrence, h_n and c_n keep the undropped h.  ``saved["drop"]`` then carries (p, seed, keep_u, hdrop) for the backward.
        ``state``: a caller-owned ``alloc_state(B, L + 1, dev)``; ``buffers``: caller-owned outputs and workspaces (_tf_forward)."""
        head, saved = self._tf_forward(params, features, None, caps, lengths, tmax, state, False, None, noise_u, seed, temperature, pretrain,
                                       (dropout, dropout_seed, keep_u), buffers)
        return (*head, saved) if keep_state else head

    def _tf_check_inputs(self, features, caps, B: int) -> None:
        if features.shape != (B, self.E) or caps.dtype != torch.int64:
            raise ValueError("features must be [B, E] and caps int64 [B, L]")

    def _tf_ws(self, B: int, T: int, Tmax: int, dev):
        return (torch.empty(B * Tmax, self.V, device=dev, dtype=torch.float32), torch.empty(B * Tmax, device=dev, dtype=torch.int64))

    def forward_scheduled(self, params, features: torch.Tensor, caps: torch.Tensor, lengths, sample_prob: float, pick: str = "sample",
                          coin_u: Optional[torch.Tensor] = None, noise_u: Optional[torch.Tensor] = None, seed: int = 0,
                          tmax: Optional[int] = None, state=None, buffers=None, dropout: float = 0.0, dropout_seed: int = 0,
                          keep_u: Optional[torch.Tensor] = None):
        """gic_decoder_forward_ss: ``forward_tf(pretrain=True, keep_state=True)`` with scheduled sampling -- the input of step t >= 1 is
        the model's own pick from step t-1's logits where coin < ``sample_prob`` (and t < lengths[b]), else caps[:, t-1].  Returns
        (pred, (h_n, c_n), saved, inputs int64 [B, L], replaced int32 [B, L]); ``saved`` carries ``inputs`` as its captions, so
        ``forward_tf_bwd`` runs on it unchanged.  ``coin_u`` f32 [B, L] / ``noise_u`` f32 [L, B, V] replace the device draws.
        ``dropout`` / ``dropout_seed`` / ``keep_u`` as forward_tf (gic_decoder_forward_ss_drop): the picks see the dropped logits.
        ``state`` / ``buffers`` as forward_tf."""
        head, *rest = self._tf_forward(params, features, None, caps, lengths, tmax, state, False, (sample_prob, pick, coin_u, noise_u, seed),
                                       drop=(dropout, dropout_seed, keep_u), bufs=buffers)
        return (*head, *rest)

    def forward_tf_bwd(self, params, saved, pred: torch.Tensor, d_pred: torch.Tensor, temperature: float, pretrain: bool = False,
                       ws=None, grads=None, dropout: float = 0.0, dropout_seed: int = 0,
                       keep_u: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """gic_decoder_forward_tf_bwd: gradients of a loss on ``pred`` of the ``forward_tf(..., keep_state=True)`` call that returned
        ``saved``; the list is ordered as ``sample_bwd``'s (parameters, then d features).  A forward call with dropout is followed by
        gic_decoder_forward_tf_drop_bwd with the (p, seed, keep_u, hdrop) that ``saved`` carries; ``dropout`` > 0 with ``dropout_seed``
        / ``keep_u`` stands in for the first three."""
        return self._tf_backward(params, saved, pred, d_pred, None, temperature, pretrain, ws, grads, (dropout, dropout_seed, keep_u))

    def sample_bwd(self, params, st, out: torch.Tensor, ids: torch.Tensor, d_out: torch.Tensor, temperature: float,
                   pretrain: bool = False, ws=None, grads=None, phases: int = 3, dev_scalars=None) -> List[torch.Tensor]:
        """phases: 1 = output layer only (w_out / b_out gradients complete), 2 = recurrent part, 3 = both; | 4 = also the gradient of
        the initial states, read back with ``state_grads(ws)`` (gicap.h)."""
        B, Lc = ids.shape
        dev = out.device
        d_out = _to_act(d_out, self.act)
        self.prepare(params)
        ws = ws if ws is not None else self.alloc_bwd_ws(B, Lc, dev)
        grads = grads if grads is not None else self.alloc_grads(params, B)
        w = self._bwd_ws_struct(ws)
        d = self.dims(B, Lc)
        L.check(L.load().gic_decoder_sample_bwd(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            C.byref(w), ptr(out), ptr(ids), ptr(d_out), float(temperature), int(bool(pretrain)),
            C.byref(self._pstruct(grads[:-1], L.DecoderGrads, grads[-1])), int(phases),
            dev_scalars.ptr if dev_scalars is not None else None, stream_ptr()), "gic_decoder_sample_bwd")
        return grads

    def state_grads(self, ws):
        """(d_h0, d_c0), each f32 [NL, B, H], from the backward workspace of the sample_bwd call that just ran: slot 0 of the
        recurrent input-gradient buffers holds d[x_0 | h_-1], the cell-gradient carry ends at d c_-1."""
        d_h0 = torch.stack([ws["dxh"][l][0][:, self.din(l):] for l in range(self.NL)]).contiguous()
        d_c0 = torch.stack([ws["dc"][l] for l in range(self.NL)]).contiguous()
        return d_h0, d_c0

    def _states(self, opts, states, B: int):
        shape = (self.NL, B, self.H)
        return _decode_states(opts, states, shape, f"states must be (h0, c0), each [num_layers={self.NL}, B={B}, H={self.H}]")

    _PREFIX = "gic_decoder"

    def beam_ws_bytes(self, B: int, Lc: int, beam: int) -> int:
        """Bytes of gic_decoder_beam_search's workspace (host-only query; the library's own path choice sizes it)."""
        return self._ws_bytes("beam", B, Lc, beam)

    def beam_fused(self, B: int, beam: int) -> bool:
        """True if the search runs on the fused step kernels (B * beam rows within fused_rollout_rows())."""
        return B * beam <= self.fused_rollout_rows()

    def beam_search(self, params, features: torch.Tensor, Lc: int, beam: int, eos_id: int = 2, pad_id: int = 0,
                    length_penalty: float = 0.0, states=None, ws: Optional[torch.Tensor] = None, force_words=None, no_repeat_ngram: int = 0,
                    min_length: int = 0, suppress_tokens=()):
        """gic_decoder_beam_search: (ids int64 [B, beam, Lc], scores f32 [B, beam], lengths int32 [B, beam]), beams best first.
        ``states`` = (h0, c0), each f32 [NL, B, H].  ``ws``: a uint8 workspace of at least beam_ws_bytes() bytes (256-aligned).
        ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``: decode constraints (gic_decode_constraints); any of them set runs
        gic_decoder_constrained_beam_search.  ``force_words`` (pack_force_words; None = off, nothing new runs): lexically constrained
        beam search, gic_decoder_forced_beam_search -- the outputs in its order plus met int32 [B, beam]; ``ws`` then holds
        forced_beam_ws_bytes() bytes."""
        if force_words is not None:
            return self._forced_beam(params, features, None, Lc, beam, eos_id, pad_id, length_penalty, states, ws, False, force_words,
                                     decode_constraints(no_repeat_ngram, min_length, suppress_tokens), suppress_tokens)
        return self._beam(params, features, None, Lc, beam, eos_id, pad_id, length_penalty, states, ws, False, None,
                          decode_constraints(no_repeat_ngram, min_length, suppress_tokens))

    def diverse_beam_search(self, params, features: torch.Tensor, Lc: int, beam: int, groups: int, diversity: float, eos_id: int = 2,
                            pad_id: int = 0, length_penalty: float = 0.0, states=None, ws: Optional[torch.Tensor] = None,
                            no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
        """gic_decoder_diverse_beam_search: ``beam`` beams in ``groups`` groups (which must divide ``beam``) with the Hamming penalty
        ``diversity``; (ids int64 [B, beam, Lc], scores f32 [B, beam], lengths int32 [B, beam]) in group-major order, each group's
        beams best first.  ``states`` and ``ws`` (beam_ws_bytes() for the same beam) and the decode constraints as for beam_search."""
        return self._beam(params, features, None, Lc, beam, eos_id, pad_id, length_penalty, states, ws, False, (groups, diversity),
                          decode_constraints(no_repeat_ngram, min_length, suppress_tokens))

    def sample_ws_bytes(self, B: int, Lc: int, num_samples: int) -> int:
        """Bytes of gic_decoder_sample_captions' workspace (host-only query; the library's own path choice sizes it)."""
        return self._ws_bytes("sample", B, Lc, num_samples)

    def sample_captions(self, params, features: torch.Tensor, Lc: int, num_samples: int, top_k: int = 0, top_p: float = 1.0,
                        temperature: float = 1.0, eos_id: int = 2, pad_id: int = 0, seed: int = 0,
                        noise_u: Optional[torch.Tensor] = None, states=None, ws: Optional[torch.Tensor] = None,
                        no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
        """gic_decoder_sample_captions: (ids int64 [B, n, Lc], scores f32 [B, n], lengths int32 [B, n]) in row order.  ``noise_u`` f32
        [Lc, B*n, V] or None = Philox(seed).  ``states`` = (h0, c0), each f32 [NL, B, H].  ``ws``: a uint8 workspace of at least
        sample_ws_bytes() bytes (256-aligned).  ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``: decode constraints
        (gic_decode_constraints); any of them set runs gic_decoder_constrained_sample_captions."""
        return self._sample(params, features, None, Lc, num_samples, top_k, top_p, temperature, eos_id, pad_id, seed, noise_u, states, ws,
                            decode_constraints(no_repeat_ngram, min_length, suppress_tokens))


# ------------------------------------------------------------------------------------------ discriminator
class DiscEngine:
    """Discriminator.forward/backward (reference src/discriminator.py:34-62) on the HIP library."""

    OUT = 100
    OUT_PAD = 104

    def __init__(self, vocab: int, embed_dim: int, num_rep: int, filter_sizes: Sequence[int], num_filters: Sequence[int], dtype: int,
                 dropout: float = 0.2):
        if len(filter_sizes) != len(num_filters) or not 1 <= len(filter_sizes) <= L.MAX_CONVS:
            raise ValueError("disc_filter_sizes / disc_num_filters must have equal length in 1..%d" % L.MAX_CONVS)
        if embed_dim % num_rep:
            raise ValueError("disc_embed_dim must be a multiple of disc_num_rep")
        self.V, self.De, self.R = vocab, embed_dim, num_rep
        self.fs, self.nf = list(filter_sizes), list(num_filters)
        self.F = sum(self.nf)
        # leading dimension of the [B*R, F] activations: whole 128-byte lines per row in bf16 (64 elements), so that a 64-byte LDS-DMA piece of
        # a row never straddles two cache lines (the highway product over cfg5's 622 592 roll-out rows: 1.65 -> 1.45 ms; cfg5 10.46 -> 10.18 ms,
        # profiles/r03_gemm_tile16_experiment.txt)
        pad = int(os.environ.get("GIC_DISC_FP_ALIGN", "64"))
        self.Fp = (self.F + pad - 1) // pad * pad
        self.s = embed_dim // num_rep
        self.dt = dtype
        self.act = TORCH_DTYPE[dtype]
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout probability has to be in [0, 1), got %r" % (dropout,))
        self.drop_p = float(dropout)
        self._shadow = None
        self._shadow_key = None

    # params: [emb, (conv_w, conv_b)*nconv, hw_w, hw_b, f2o_w, f2o_b, o2l_w, o2l_b]
    def nparams(self) -> int:
        return 7 + 2 * len(self.fs)

    def dims(self, B: int, Lc: int) -> L.DiscDims:
        d = L.DiscDims()
        d.B, d.L, d.V, d.De, d.R, d.nconv = B, Lc, self.V, self.De, self.R, len(self.fs)
        d.fsize = _arr(C.c_int32, L.MAX_CONVS, self.fs)
        d.nfilt = _arr(C.c_int32, L.MAX_CONVS, self.nf)
        d.F, d.Fp, d.dtype, d.drop_p = self.F, self.Fp, self.dt, self.drop_p
        return d

    def plan(self, B: int, Lc: int, want_param_grads: bool = True, train: bool = True, keeps_argmax: bool = True, hw_aligned: bool = True):
        """gic_debug_disc_plan: the kernels gic_disc_fwd / gic_disc_bwd select for these shapes in the library's current deterministic
        mode, one line per launch (line 0: the forward's conv + pool kernel).  Host-only."""
        flags = (0 if keeps_argmax else L.DISC_PLAN_NO_ARGMAX) | (L.DISC_PLAN_GRADS if want_param_grads else 0) | \
                (L.DISC_PLAN_TRAIN if train else 0) | (0 if hw_aligned else L.DISC_PLAN_HW_UNALIGNED)
        out = C.create_string_buffer(2048)
        L.check(L.load().gic_debug_disc_plan(C.byref(self.dims(B, Lc)), flags, out, len(out)), "gic_debug_disc_plan")
        return out.value.decode().splitlines()

    def _pstruct(self, params, cls=L.DiscParams):
        n = len(self.fs)
        s = cls()
        s.emb = ptr(params[0])
        s.conv_w = _arr(C.c_void_p, L.MAX_CONVS, [ptr(params[1 + 2 * k]) for k in range(n)])
        s.conv_b = _arr(C.c_void_p, L.MAX_CONVS, [ptr(params[2 + 2 * k]) for k in range(n)])
        o = 1 + 2 * n
        s.hw_w, s.hw_b, s.f2o_w, s.f2o_b, s.o2l_w, s.o2l_b = (ptr(params[o + i]) for i in range(6))
        return s

    def check_params(self, params) -> None:
        if len(params) != self.nparams():
            raise ValueError("discriminator expects %d parameter tensors" % self.nparams())
        require_gpu(*params)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("discriminator parameters must be contiguous float32 (master weights)")

    def prepare(self, params):
        key = _key(params)
        if self._shadow is not None and key == self._shadow_key:
            return self._shadow
        dev = params[0].device
        if self._shadow is None or self._shadow["hw_w"].device != dev:
            self._shadow = {
                "emb": None if self.dt == L.F32 else torch.empty(self.De, self.V, device=dev, dtype=self.act),
                "hw_w": torch.empty(self.Fp, self.Fp, device=dev, dtype=self.act),
                "f2o_w": torch.empty(self.OUT_PAD, self.Fp, device=dev, dtype=self.act),
                # bf16 mode: highway^T so that the input-gradient product d_pooled += dh W runs on k-contiguous operands
                "hw_w_t": None if self.dt == L.F32 else torch.empty(self.Fp, self.Fp, device=dev, dtype=self.act),
            }
        d = self.dims(1, max(self.fs))
        L.check(L.load().gic_disc_prepare(C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)),
                                          stream_ptr()), "gic_disc_prepare")
        self._shadow_key = key
        return self._shadow

    def _shadow_struct(self, params) -> L.DiscShadow:
        sh = self._shadow
        s = L.DiscShadow()
        s.emb = ptr(params[0]) if sh["emb"] is None else ptr(sh["emb"])
        s.hw_w, s.f2o_w = ptr(sh["hw_w"]), ptr(sh["f2o_w"])
        s.hw_w_t = ptr(sh["hw_w_t"])
        return s

    def alloc_state(self, B: int, Lc: int, dev, forward_only: bool = False):
        """``forward_only``: an eval-mode forward that no backward follows (reward evaluation): no argmax / pre-activation / keep
        buffers (gic_disc_fwd then writes none), and only the pad columns of ``ydrop`` are zeroed."""
        f32, u8 = torch.float32, torch.uint8
        MR = B * self.R
        if forward_only:
            ydrop = torch.empty(MR, self.Fp, device=dev, dtype=self.act)
            if self.Fp > self.F:
                ydrop[:, self.F:].zero_()
            return {"emb": torch.empty(B * Lc, self.De, device=dev, dtype=f32), "pooled": torch.empty(MR, self.Fp, device=dev, dtype=self.act),
                    "argmax": None, "hpre": None, "keep": None, "ydrop": ydrop, "feat": torch.empty(MR, self.OUT, device=dev, dtype=f32)}
        return {
            "emb": torch.empty(B * Lc, self.De, device=dev, dtype=f32),
            "pooled": torch.empty(MR, self.Fp, device=dev, dtype=self.act),
            "argmax": torch.empty(MR, self.Fp, device=dev, dtype=u8),
            "hpre": torch.empty(MR, self.Fp, device=dev, dtype=f32),
            "keep": torch.empty(MR, self.Fp, device=dev, dtype=u8),
            "ydrop": torch.zeros(MR, self.Fp, device=dev, dtype=self.act),    # pad columns must stay zero
            "feat": torch.empty(MR, self.OUT, device=dev, dtype=f32),
        }

    def _state_struct(self, st) -> L.DiscState:
        s = L.DiscState()
        for k in ("emb", "pooled", "argmax", "hpre", "keep", "ydrop", "feat"):
            setattr(s, k, ptr(st.get(k)))
        return s

    def alloc_bwd_ws(self, B: int, Lc: int, dev):
        f32 = torch.float32
        MR = B * self.R
        return {
            "dfeat": torch.empty(MR, self.OUT_PAD, device=dev, dtype=self.act),
            "dh": torch.empty(MR, self.Fp, device=dev, dtype=self.act),
            "dydrop": torch.empty(MR, self.Fp, device=dev, dtype=f32),
            "dpooled": torch.empty(MR, self.Fp, device=dev, dtype=f32),
            "demb": torch.empty(B * Lc, self.De, device=dev, dtype=self.act),
        }

    def soft_input(self, inp: torch.Tensor) -> torch.Tensor:
        """[B,L,V] float tensor -> contiguous compute-dtype tensor (converted by gic_cast2d if needed)."""
        if inp.dim() != 3 or inp.shape[2] != self.V:
            raise ValueError(f"discriminator input must be [B, L, V={self.V}], got {tuple(inp.shape)}")
        require_gpu(inp)
        if inp.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("discriminator input must be float32 or bfloat16")
        inp = inp.contiguous()
        if inp.dtype != self.act:
            dst = torch.empty(inp.shape, device=inp.device, dtype=self.act)
            cast2d(inp, dst, inp.shape[0] * inp.shape[1], self.V, self.V, self.V)
            inp = dst
        return inp

    def fwd(self, params, inp_soft: Optional[torch.Tensor], inp_ids: Optional[torch.Tensor], train: bool,
            keep_mask: Optional[torch.Tensor] = None, seed: int = 0, state=None, logits=None, forward_only: bool = False,
            dev_scalars=None, seed_slot: int = 0, cond: Optional[torch.Tensor] = None, cond_index: Optional[torch.Tensor] = None):
        """``dev_scalars`` / ``seed_slot``: the dropout seed is read from device memory (gic_step_scalars).  ``forward_only`` (eval mode only): nothing is saved for a backward pass (see alloc_state).
        ``cond``: f32 [B, F], one row per caption (the image projection q of a conditioned D): the match term is added to the logits.
        ``cond_index`` (inference only: no backward knows it): int32 [B], caption b is scored against ``cond[cond_index[b]]`` and ``cond``
        is [q_rows, F] (match_logits)."""
        if forward_only and train:
            raise ValueError("forward_only is an eval-mode option: the train-mode forward saves its dropout mask for the backward")
        if cond_index is not None and cond is None:
            raise ValueError("cond_index without cond")
        self.check_params(params)
        src = inp_soft if inp_soft is not None else inp_ids
        require_gpu(src, keep_mask)
        B, Lc = src.shape[0], src.shape[1]
        if cond is not None:
            cond = self._check_cond(cond, B, cond_index)                 # before anything is launched
        dev = src.device
        if inp_ids is not None:
            if inp_ids.dtype != torch.int64:
                raise ValueError("token ids must be int64")
            inp_ids = inp_ids.contiguous()
        if keep_mask is not None:
            if tuple(keep_mask.shape) != (B * self.R, self.F):
                raise ValueError(f"keep_mask must be [B*R={B * self.R}, F={self.F}]")
            keep_mask = keep_mask.to(torch.uint8).contiguous()
        self.prepare(params)
        st = state if state is not None else self.alloc_state(B, Lc, dev, forward_only=forward_only)
        logits = logits if logits is not None else torch.empty(B * self.R, device=dev, dtype=torch.float32)
        d = self.dims(B, Lc)
        L.check(L.load().gic_disc_fwd(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            ptr(inp_soft), self.V, ptr(inp_ids), int(bool(train)), ptr(keep_mask), int(seed) & (2 ** 64 - 1), ptr(logits),
            dev_scalars.ptr if dev_scalars is not None else None, int(seed_slot), stream_ptr()), "gic_disc_fwd")
        if cond is not None:
            self.match_logits(st, cond, logits=logits, accumulate=True, q_index=cond_index)
        return logits, st

    def match_scale(self) -> float:
        return float(self.F) ** -0.5

    def _check_cond(self, q: torch.Tensor, B: int, q_index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``q`` f32 [B, F], one row per caption; with ``q_index`` (int32 device tensor [B]) f32 [q_rows, F], q_rows >= 1."""
        require_gpu(q, q_index)
        if q.dtype != torch.float32:
            raise ValueError("the image projection q must be float32")
        if q_index is None:
            if tuple(q.shape) != (B, self.F):
                raise ValueError(f"the image projection q must be [captions={B}, F={self.F}], got {tuple(q.shape)}")
        else:
            if q.dim() != 2 or q.shape[1] != self.F or q.shape[0] < 1:
                raise ValueError(f"the image projection q must be [q_rows >= 1, F={self.F}] under an index, got {tuple(q.shape)}")
            if q_index.dtype != torch.int32 or tuple(q_index.shape) != (B,) or not q_index.is_contiguous():
                raise ValueError(f"the image index must be a contiguous int32 tensor [captions={B}], got {q_index.dtype} {tuple(q_index.shape)}")
        return q.contiguous()

    def match_logits(self, state: dict, q: torch.Tensor, logits=None, accumulate: bool = False, q_index: Optional[torch.Tensor] = None):
        """gic_disc_match_fwd: the match term F^-1/2 <ydrop[m], q[m // R]> of a forward's state (a forward-only one included), alone or
        (``accumulate``) added to ``logits``.  ``q_index`` (int32 [captions]): gic_disc_match_fwd_grouped, caption b against
        ``q[q_index[b]]`` of ``q`` [q_rows, F]; an index outside [0, q_rows) gives that caption NaN logits."""
        MR = state["ydrop"].shape[0]
        B = MR // self.R
        q = self._check_cond(q, B, q_index)
        if logits is None:
            if accumulate:
                raise ValueError("match_logits: accumulate needs logits")
            logits = torch.empty(MR, device=q.device, dtype=torch.float32)
        d = self.dims(B, max(self.fs))
        if q_index is not None:
            L.check(L.load().gic_disc_match_fwd_grouped(C.byref(d), C.byref(self._state_struct(state)), ptr(q), q.shape[0], ptr(q_index),
                                                        self.match_scale(), int(bool(accumulate)), ptr(logits), stream_ptr()),
                    "gic_disc_match_fwd_grouped")
            return logits
        L.check(L.load().gic_disc_match_fwd(C.byref(d), C.byref(self._state_struct(state)), ptr(q), self.match_scale(), int(bool(accumulate)),
                                            ptr(logits), stream_ptr()), "gic_disc_match_fwd")
        return logits

    def rep_mean(self, state: dict, logits: Optional[torch.Tensor] = None, ybar=None, lbar=None):
        """gic_disc_rep_mean: (ybar f32 [B, F], lbar f32 [B] or None) = the means over the R representations of a forward's ``ydrop``
        and of its base ``logits`` [B*R], summed in index order.  ``ybar`` / ``lbar``: destinations (rows of a larger buffer)."""
        MR = state["ydrop"].shape[0]
        B = MR // self.R
        dev = state["ydrop"].device
        require_gpu(state["ydrop"], logits, ybar, lbar)
        ybar = ybar if ybar is not None else torch.empty(B, self.F, device=dev, dtype=torch.float32)
        if logits is not None:
            if logits.dtype != torch.float32 or logits.numel() != MR or not logits.is_contiguous():
                raise ValueError(f"rep_mean: logits must be contiguous float32 [B*R={MR}]")
            lbar = lbar if lbar is not None else torch.empty(B, device=dev, dtype=torch.float32)
        for name, t, shape in (("ybar", ybar, (B, self.F)), ("lbar", lbar, (B,))):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"rep_mean: {name} must be contiguous float32 {shape}")
        d = self.dims(B, max(self.fs))
        L.check(L.load().gic_disc_rep_mean(C.byref(d), C.byref(self._state_struct(state)), ptr(logits), ptr(ybar),
                                           ptr(lbar) if logits is not None else None, stream_ptr()), "gic_disc_rep_mean")
        return ybar, (lbar if logits is not None else None)

    def shared_state(self, src: dict, B: int, Lc: int, dev) -> dict:
        """State of a second forward on the same input: its own dropout / head buffers, the rest aliases ``src``."""
        st = dict(src)
        own = self.alloc_state(B, Lc, dev)
        for k in ("keep", "ydrop", "feat"):
            st[k] = own[k]
        return st

    def fwd_redrop(self, params, src_state: dict, dst_state: dict, train: bool, keep_mask: Optional[torch.Tensor] = None,
                   seed: int = 0, logits=None, dev_scalars=None, seed_slot: int = 0, cond: Optional[torch.Tensor] = None):
        """gic_disc_fwd_redrop: D on the same input as the forward that filled ``src_state``, under another dropout draw.  ``cond``: as in fwd."""
        self.check_params(params)
        MR = src_state["pooled"].shape[0]
        dev = src_state["pooled"].device
        if keep_mask is not None:
            require_gpu(keep_mask)
            if tuple(keep_mask.shape) != (MR, self.F):
                raise ValueError(f"keep_mask must be [B*R={MR}, F={self.F}]")
            keep_mask = keep_mask.to(torch.uint8).contiguous()
        self.prepare(params)
        logits = logits if logits is not None else torch.empty(MR, device=dev, dtype=torch.float32)
        B = MR // self.R
        d = self.dims(B, src_state["emb"].shape[0] // B)
        L.check(L.load().gic_disc_fwd_redrop(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(src_state)),
            C.byref(self._state_struct(dst_state)), int(bool(train)), ptr(keep_mask), int(seed) & (2 ** 64 - 1), ptr(logits),
            dev_scalars.ptr if dev_scalars is not None else None, int(seed_slot), stream_ptr()), "gic_disc_fwd_redrop")
        if cond is not None:
            self.match_logits(dst_state, cond, logits=logits, accumulate=True)
        return logits, dst_state

    def split_state(self, st: dict):
        """Views of the first / second half of a state's rows (two forward passes of B/2 captions each written into one state)."""
        a, b = {}, {}
        for k, v in st.items():
            h = v.shape[0] // 2
            a[k], b[k] = v[:h], v[h:]
        return a, b

    def bwd(self, params, st, inp_soft, inp_ids, train: bool, d_logits: torch.Tensor, want_param_grads: bool,
            want_input_grad: bool, grads=None, accumulate: bool = False, ws=None, d_inp=None, cond: Optional[torch.Tensor] = None, d_q=None,
            cond_entry: bool = False):
        """Both ``inp_soft`` and ``inp_ids`` given: mixed batch (gicap.h) -- ``st`` holds the ids pass in its first half of the rows
        and the soft pass in its second half; one backward serves both.
        ``cond`` (the q the forward was given; a mixed batch: [q; q]): gic_disc_bwd_cond, and a third result ``d_q`` f32 [B, F].
        ``cond_entry`` without ``cond``: gic_disc_bwd_cond with q = NULL (what must equal gic_disc_bwd; d_q is None)."""
        src = inp_soft if inp_soft is not None else inp_ids
        B, Lc = src.shape[0], src.shape[1]
        if inp_soft is not None and inp_ids is not None:
            if inp_soft.shape[:2] != inp_ids.shape[:2] or want_input_grad or not want_param_grads:
                raise ValueError("mixed batch: equal halves, parameter gradients only")
            B *= 2
        dev = src.device
        d_logits = d_logits.contiguous().float()
        self.prepare(params)
        ws = ws if ws is not None else self.alloc_bwd_ws(B, Lc, dev)
        if want_param_grads and grads is None:
            grads = [torch.empty_like(p) for p in params]
            accumulate = False
        if want_input_grad and d_inp is None:
            d_inp = torch.empty(B, Lc, self.V, device=dev, dtype=self.act)
        w = L.DiscBwdWs()
        for k in ("dfeat", "dh", "dydrop", "dpooled", "demb"):
            setattr(w, k, ptr(ws[k]))
        d = self.dims(B, Lc)
        gs = self._pstruct(grads, L.DiscGrads) if want_param_grads else None
        if cond is not None or cond_entry:
            if cond is not None:
                cond = self._check_cond(cond, B)
                d_q = d_q if d_q is not None else torch.empty(B, self.F, device=dev, dtype=torch.float32)
            L.check(L.load().gic_disc_bwd_cond(
                C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
                C.byref(w), ptr(inp_soft), self.V, ptr(inp_ids), int(bool(train)), ptr(d_logits),
                C.byref(gs) if gs is not None else None, int(bool(accumulate)), ptr(d_inp) if want_input_grad else None, self.V,
                ptr(cond), self.match_scale(), ptr(d_q), stream_ptr()), "gic_disc_bwd_cond")
            return (grads if want_param_grads else None), (d_inp if want_input_grad else None), d_q
        L.check(L.load().gic_disc_bwd(
            C.byref(d), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            C.byref(w), ptr(inp_soft), self.V, ptr(inp_ids), int(bool(train)), ptr(d_logits),
            C.byref(gs) if gs is not None else None, int(bool(accumulate)), ptr(d_inp) if want_input_grad else None, self.V,
            stream_ptr()), "gic_disc_bwd")
        return (grads if want_param_grads else None), (d_inp if want_input_grad else None)


    # ---- the conditioned D's image projection q = img_proj(pooled) (no kernel of its own: the generic GEMM and column sum)
    def img_proj_fwd(self, weight: torch.Tensor, bias: torch.Tensor, pooled: torch.Tensor, out=None):
        """q f32 [B, F] = pooled [B, C] W^T + b on the compute-dtype image of ``weight`` [F, C] (refreshed when the weight changes), f32
        accumulate.  Returns (q, pooled in the compute dtype: what the backward reads)."""
        require_gpu(weight, bias, pooled)
        Fq, Cin = weight.shape
        pooled = _to_act(pooled.reshape(pooled.shape[0], -1), self.act)
        if Fq != self.F or pooled.shape[1] != Cin:
            raise ValueError(f"img_proj: weight {tuple(weight.shape)} against F={self.F} and pooled features {tuple(pooled.shape)}")
        key = _key([weight])
        if getattr(self, "_proj_key", None) != key:
            self._proj_w = weight if self.act == torch.float32 else cast2d(weight, torch.empty(Fq, Cin, device=weight.device, dtype=self.act), Fq, Cin, Cin, Cin)
            self._proj_key = key
        B = pooled.shape[0]
        q = out if out is not None else torch.empty(B, Fq, device=pooled.device, dtype=torch.float32)
        gemm(pooled, self._proj_w, q, B, Fq, Cin, Cin, Cin, Fq, True, True, bias=bias)
        return q, pooled

    def img_proj_bwd(self, d_q: torch.Tensor, pooled: torch.Tensor, d_weight: torch.Tensor, d_bias: torch.Tensor, accumulate: bool = False):
        """d_weight [F, C] (+)= d_q^T pooled, d_bias [F] (+)= colsum(d_q): f32 products over the B captions."""
        B, Fq = d_q.shape
        Cin = pooled.shape[1]
        p32 = _to_act(pooled, torch.float32)
        gemm(d_q, p32, d_weight, Fq, Cin, B, Fq, Cin, Cin, False, False, accumulate=accumulate)
        L.check(L.load().gic_colsum(ptr(d_q), L.F32, Fq, B, Fq, ptr(d_bias), int(bool(accumulate)), stream_ptr()), "gic_colsum")


# ------------------------------------------------------------------------------------------ fused clip + Adam
def clip_adam_partials(n: int) -> int:
    return int(L.load().gic_clip_adam_partials(n))


def clip_adam(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, clip_norm, step_count, norm_out, partials):
    require_gpu(params, grads, exp_avg, exp_avg_sq, step_count, norm_out, partials)
    L.check(L.load().gic_clip_adam(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), float(lr), float(beta1),
                                   float(beta2), float(eps), float(clip_norm), ptr(step_count), ptr(norm_out), ptr(partials),
                                   stream_ptr()), "gic_clip_adam")
    bump_param_epoch()


def adamw_opts(weight_decay=0.0, ranges=(), ranges_dev=None, schedule="none", warmup_steps=0, total_steps=0, min_ratio=0.0,
               step_size=0, gamma=0.1, ema=None, ema_count=None, ema_decay=0.0, ema_warmup=True, sched_out=None) -> L.AdamwOpts:
    """gic_adamw_opts, built once per optimizer.  ``ranges``: the host table, a flat sequence s0, e0, s1, e1, ...; ``ranges_dev``: the
    same values as a device int64 tensor.  The struct keeps the host table and every tensor alive."""
    require_gpu(ranges_dev, ema, ema_count, sched_out)
    flat = [int(x) for x in ranges]
    if len(flat) % 2:
        raise ValueError("decay ranges are (start, end) pairs")
    if flat and (ranges_dev is None or ranges_dev.dtype != torch.int64 or ranges_dev.numel() != len(flat)):
        raise ValueError("ranges_dev must be the int64 device copy of the decay ranges")
    if schedule not in L.LR_SCHEDULES:
        raise ValueError(f"unknown LR schedule {schedule!r}; choose from {sorted(L.LR_SCHEDULES)}")
    host = _arr(C.c_int64, max(len(flat), 1), flat)
    o = L.AdamwOpts(float(weight_decay), C.cast(host, C.c_void_p).value if flat else None, ptr(ranges_dev) if flat else None,
                    len(flat) // 2, L.LR_SCHEDULES[schedule], int(warmup_steps), int(total_steps), int(step_size), float(min_ratio),
                    float(gamma), ptr(ema), ptr(ema_count), float(ema_decay), int(bool(ema_warmup)), 0, ptr(sched_out))
    o._keep = (host, ranges_dev, ema, ema_count, sched_out)
    return o


def clip_adamw(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, clip_norm, step_count, norm_out, partials, opts):
    """gic_clip_adamw: clip_adam plus ``opts`` (adamw_opts): device-side LR schedule, decoupled weight decay, weight EMA."""
    require_gpu(params, grads, exp_avg, exp_avg_sq, step_count, norm_out, partials)
    L.check(L.load().gic_clip_adamw(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), float(lr), float(beta1),
                                    float(beta2), float(eps), float(clip_norm), ptr(step_count), ptr(norm_out), ptr(partials),
                                    C.byref(opts), stream_ptr()), "gic_clip_adamw")
    bump_param_epoch()


# ------------------------------------------------------------------------------------------ visual-attention decoder
class AttnDecoderEngine(_CaptionDecodes, _TeacherForced):
    """gic_attn_sample_fwd / bwd (gicap.h): the reference's roll-out loop with soft attention over the trunk's feature map
    (BASELINE config 4; no reference counterpart, oracle/cpu_attention.py).
    params order: [embed, w_ih, w_hh, b_ih, b_hh, w_out, b_out, w_f, b_f, w_h, w_a]."""

    NAMES = ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a")
    NL = 1                        # one LSTM layer: the final states are [1, B, H]
    _GRADS = L.AttnGrads
    _TF_BWD_WS_STEPS = "T"

    def __init__(self, vocab: int, embed: int, hidden: int, feat_c: int, positions: int, attn: int, dtype: int):
        self.V, self.E, self.H, self.C, self.P, self.A, self.dt = vocab, embed, hidden, feat_c, positions, attn, dtype
        self.act = TORCH_DTYPE[dtype]
        self.ldx = embed + feat_c + hidden
        self._shadow = None
        self._shadow_key = None

    def dims(self, B: int, Lc: int) -> L.AttnDims:
        return L.AttnDims(B, Lc, self.V, self.E, self.H, self.C, self.P, self.A, self.dt)

    def _pstruct(self, params, cls=L.AttnParams, extra=None):
        s = cls()
        for n, p in zip(self.NAMES, params):
            setattr(s, n, ptr(p))
        if extra is not None:
            s.features = ptr(extra)
        return s

    def check_params(self, params) -> None:
        if len(params) != len(self.NAMES):
            raise ValueError("attention decoder expects %d parameter tensors" % len(self.NAMES))
        require_gpu(*params)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("attention decoder parameters must be contiguous float32 (master weights)")

    def prepare(self, params):
        key = _key(params)
        if self._shadow is not None and key == self._shadow_key:
            return self._shadow
        dev = params[0].device
        if self._shadow is None:
            self._shadow = {
                "wcat": torch.empty(4 * self.H, self.ldx, device=dev, dtype=self.act),
                "bsum": torch.empty(4 * self.H, device=dev, dtype=torch.float32),
                "wout": None if self.dt == L.F32 else torch.empty(self.V, self.H, device=dev, dtype=self.act),
                "wcat_t": torch.empty(self.ldx, 4 * self.H, device=dev, dtype=self.act),
                "wf": torch.empty(self.A, self.C, device=dev, dtype=self.act),
                "wh": torch.empty(self.A, self.H, device=dev, dtype=self.act),
            }
        L.check(L.load().gic_attn_prepare(C.byref(self.dims(1, 1)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)),
                                          stream_ptr()), "gic_attn_prepare")
        self._shadow_key = key
        return self._shadow

    def _shadow_struct(self, params) -> L.AttnShadow:
        sh = self._shadow
        s = L.AttnShadow()
        s.wcat, s.bsum, s.wcat_t, s.wf, s.wh = ptr(sh["wcat"]), ptr(sh["bsum"]), ptr(sh["wcat_t"]), ptr(sh["wf"]), ptr(sh["wh"])
        s.wout = ptr(params[5]) if sh["wout"] is None else ptr(sh["wout"])
        return s

    def alloc_state(self, B: int, Lc: int, dev):
        f32 = torch.float32
        return {
            "xh": torch.empty(Lc + 1, B, self.ldx, device=dev, dtype=self.act),
            "gates": torch.empty(Lc, B, 4 * self.H, device=dev, dtype=f32),
            "c": torch.empty(Lc + 1, B, self.H, device=dev, dtype=f32),
            "hout": torch.empty(B, Lc, self.H, device=dev, dtype=self.act),
            "part": torch.empty(step_part_floats(B, Lc, self.V), device=dev, dtype=f32),
            "fproj": torch.empty(B, self.P, self.A, device=dev, dtype=self.act),
            "alpha": torch.empty(Lc, B, self.P, device=dev, dtype=f32),
            "hproj": torch.empty(Lc, B, self.A, device=dev, dtype=f32),
        }

    def _state_struct(self, st) -> L.AttnState:
        s = L.AttnState()
        for k in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
            setattr(s, k, ptr(st[k]))
        return s

    def sample_fwd(self, params, features, fmap, Lc: int, temperature: float, pretrain: bool = False, noise_u=None, seed: int = 0,
                   state=None, out=None, ids=None, states=None, dev_scalars=None, seed_slot: int = 0):
        """``dev_scalars`` / ``seed_slot``: temperature and seed from device memory (StepScalarsBuffer).
        ``state`` / ``out`` / ``ids``: caller-owned buffers (alloc_state; the fused step driver pre-allocates them).
        ``states`` = (h0, c0), each [1, B, H] or [B, H]: initial LSTM state (constants of the backward pass)."""
        self.check_params(params)
        require_gpu(features, fmap, noise_u)
        B = features.shape[0]
        if tuple(features.shape) != (B, self.E) or features.dtype != torch.float32:
            raise ValueError(f"features must be float32 [B,{self.E}]")
        fmap = self._act_fmap(fmap, B)
        if noise_u is not None:
            if tuple(noise_u.shape) != (Lc, B, self.V) or noise_u.dtype != torch.float32:
                raise ValueError(f"noise_u must be float32 [L={Lc},B={B},V={self.V}]")
            noise_u = noise_u.contiguous()
        dev = features.device
        self.prepare(params)
        st = dict(state) if state is not None else self.alloc_state(B, Lc, dev)
        out = out if out is not None else torch.empty(B, Lc, self.V, device=dev, dtype=self.act)
        ids = ids if ids is not None else torch.empty(B, Lc, device=dev, dtype=torch.int64)
        h0 = c0 = None
        if states is not None:
            h0, c0 = (t.detach().to(torch.float32).reshape(-1, self.H).contiguous() for t in states)
            if tuple(h0.shape) != (B, self.H) or tuple(c0.shape) != (B, self.H):
                raise ValueError(f"states must be (h0, c0), each [1, B={B}, H={self.H}]")
            require_gpu(h0, c0)
        L.check(L.load().gic_attn_sample_fwd(
            C.byref(self.dims(B, Lc)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            ptr(features.contiguous()), ptr(fmap), ptr(noise_u), int(seed) & (2 ** 64 - 1), float(temperature), int(bool(pretrain)),
            ptr(out), ptr(ids), ptr(h0), ptr(c0), dev_scalars.ptr if dev_scalars is not None else None, int(seed_slot), stream_ptr()),
            "gic_attn_sample_fwd")
        st["fmap"] = fmap
        return out, ids, st

    def _act_fmap(self, fmap: torch.Tensor, B: int) -> torch.Tensor:
        """``fmap`` [B, P, C] as a contiguous tensor of the compute dtype (cast on the GPU when it is not)."""
        if tuple(fmap.shape) != (B, self.P, self.C):
            raise ValueError(f"fmap must be [B, P={self.P}, C={self.C}], got {tuple(fmap.shape)}")
        fmap = fmap.contiguous()
        if fmap.dtype != self.act:
            dst = torch.empty(fmap.shape, device=fmap.device, dtype=self.act)
            cast2d(fmap.float() if fmap.dtype not in (torch.float32, torch.bfloat16) else fmap, dst, B * self.P, self.C, self.C, self.C)
            fmap = dst
        return fmap

    def _states(self, opts, states, B: int):
        states = None if states is None else [t.reshape(-1, self.H) for t in states]
        return _decode_states(opts, states, (B, self.H), f"states must be (h0, c0), each [1, B={B}, H={self.H}]")

    _PREFIX = "gic_attn"

    def _decode_maps(self, fmap, B: int):
        return (self._act_fmap(fmap, B),)

    def _beam_alphas(self, want: bool, B: int, beam, Lc: int, dev):
        return (torch.empty(B, beam, Lc, self.P, device=dev, dtype=torch.float32) if want else None,)

    def beam_ws_bytes(self, B: int, Lc: int, beam: int) -> int:
        """Bytes of gic_attn_beam_search's workspace (host-only query)."""
        return self._ws_bytes("beam", B, Lc, beam)

    def beam_search(self, params, features, fmap, Lc: int, beam: int, eos_id: int = 2, pad_id: int = 0, length_penalty: float = 0.0,
                    states=None, ws: Optional[torch.Tensor] = None, want_alphas: bool = False, force_words=None, no_repeat_ngram: int = 0,
                    min_length: int = 0, suppress_tokens=()):
        """gic_attn_beam_search: (ids int64 [B, beam, Lc], scores f32 [B, beam], lengths int32 [B, beam][, alphas f32 [B, beam, Lc, P]]),
        beams best first.  ``fmap`` [B, P, C] is cast to the compute dtype as in sample_fwd.  ``states`` = (h0, c0), each [1, B, H] or
        [B, H].  ``ws``: a uint8 workspace of at least beam_ws_bytes() bytes (256-aligned).  ``no_repeat_ngram`` / ``min_length`` /
        ``suppress_tokens``: decode constraints (gic_decode_constraints); any of them set runs gic_attn_constrained_beam_search.
        ``force_words`` (pack_force_words; None = off, nothing new runs): gic_attn_forced_beam_search -- the outputs in its order, the
        alphas re-ordered alongside, plus met int32 [B, beam] last; ``ws`` then holds forced_beam_ws_bytes() bytes."""
        if force_words is not None:
            return self._forced_beam(params, features, fmap, Lc, beam, eos_id, pad_id, length_penalty, states, ws, want_alphas, force_words,
                                     decode_constraints(no_repeat_ngram, min_length, suppress_tokens), suppress_tokens)
        return self._beam(params, features, fmap, Lc, beam, eos_id, pad_id, length_penalty, states, ws, want_alphas, None,
                          decode_constraints(no_repeat_ngram, min_length, suppress_tokens))

    def diverse_beam_search(self, params, features, fmap, Lc: int, beam: int, groups: int, diversity: float, eos_id: int = 2,
                            pad_id: int = 0, length_penalty: float = 0.0, states=None, ws: Optional[torch.Tensor] = None,
                            want_alphas: bool = False, no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
        """gic_attn_diverse_beam_search: beam_search's outputs for ``beam`` beams in ``groups`` groups (which must divide ``beam``)
        with the Hamming penalty ``diversity``, in group-major order, each group's beams best first; the decode constraints as for
        beam_search."""
        return self._beam(params, features, fmap, Lc, beam, eos_id, pad_id, length_penalty, states, ws, want_alphas,
                          (groups, diversity), decode_constraints(no_repeat_ngram, min_length, suppress_tokens))

    def sample_ws_bytes(self, B: int, Lc: int, num_samples: int) -> int:
        """Bytes of gic_attn_sample_captions' workspace (host-only query)."""
        return self._ws_bytes("sample", B, Lc, num_samples)

    def sample_captions(self, params, features, fmap, Lc: int, num_samples: int, top_k: int = 0, top_p: float = 1.0,
                        temperature: float = 1.0, eos_id: int = 2, pad_id: int = 0, seed: int = 0,
                        noise_u: Optional[torch.Tensor] = None, states=None, ws: Optional[torch.Tensor] = None,
                        no_repeat_ngram: int = 0, min_length: int = 0, suppress_tokens=()):
        """gic_attn_sample_captions: (ids int64 [B, n, Lc], scores f32 [B, n], lengths int32 [B, n]) in row order.  ``fmap`` [B, P, C]
        is cast to the compute dtype as in sample_fwd.  ``noise_u`` f32 [Lc, B*n, V] or None = Philox(seed).  ``states`` = (h0, c0),
        each [1, B, H] or [B, H].  ``no_repeat_ngram`` / ``min_length`` / ``suppress_tokens``: decode constraints
        (gic_decode_constraints); any of them set runs gic_attn_constrained_sample_captions."""
        return self._sample(params, features, fmap, Lc, num_samples, top_k, top_p, temperature, eos_id, pad_id, seed, noise_u, states, ws,
                            decode_constraints(no_repeat_ngram, min_length, suppress_tokens))

    def tf_ws_bytes(self, B: int, T: int, Tmax: int) -> int:
        """Bytes of gic_attn_forward_tf's logits_ws (host-only query)."""
        out = C.c_uint64(0)
        L.check(L.load().gic_attn_forward_tf_ws_bytes(C.byref(self.dims(B, T)), int(Tmax), C.byref(out)), "gic_attn_forward_tf_ws_bytes")
        return int(out.value)

    def forward_tf(self, params, features, fmap, caps: torch.Tensor, lengths, temperature: float, pretrain: bool = False,
                   noise_u: Optional[torch.Tensor] = None, seed: int = 0, want_alphas: bool = False, keep_state: bool = False,
                   tmax: Optional[int] = None, state=None, dropout: float = 0.0, dropout_seed: int = 0,
                   keep_u: Optional[torch.Tensor] = None):
        """gic_attn_forward_tf: the teacher-forced decode (DecoderEngine.forward_tf with the attention step).  ``caps`` int64 [B, T-1],
        ``lengths`` B values in 1..T, ``fmap`` [B, P, C] (cast to the compute dtype as in sample_fwd).  Returns (pred act [B, Tmax, V],
        (h_n, c_n) f32 [1, B, H], alphas f32 [B, Tmax, P] or None); with ``keep_state`` also what ``forward_tf_bwd`` needs.  ``tmax``
        as DecoderEngine.forward_tf.  ``state``: a caller-owned state (alloc_state(B, T, dev)) as in sample_fwd.  ``dropout`` /
        ``dropout_seed`` / ``keep_u``: output dropout as DecoderEngine.forward_tf (gic_attn_forward_tf_drop)."""
        head, saved = self._tf_forward(params, features, fmap, caps, lengths, tmax, state, want_alphas, None, noise_u, seed, temperature,
                                       pretrain, (dropout, dropout_seed, keep_u))
        return (*head, saved) if keep_state else head

    def _tf_check_inputs(self, features, caps, B: int) -> None:
        if tuple(features.shape) != (B, self.E) or features.dtype != torch.float32 or caps.dtype != torch.int64:
            raise ValueError(f"features must be float32 [B, {self.E}] and caps int64 [B, L]")

    def _tf_ws(self, B: int, T: int, Tmax: int, dev):
        return (torch.empty(self.tf_ws_bytes(B, T, Tmax) // 4, device=dev, dtype=torch.float32),)

    def _tf_alphas(self, want: bool, B: int, Tmax: int, dev):
        return (torch.empty(B, Tmax, self.P, device=dev, dtype=torch.float32) if want else None,)

    def _tf_d_alphas(self, d_alphas, B: int, Tmax: int):
        if d_alphas is not None:
            if tuple(d_alphas.shape) != (B, Tmax, self.P):
                raise ValueError(f"d_alphas must be [B, max(lengths)={Tmax}, P={self.P}]")
            d_alphas = d_alphas.contiguous().float()
        return (d_alphas,)

    def _bwd_ws_struct(self, ws) -> L.AttnBwdWs:
        w = L.AttnBwdWs()
        for k, v in ws.items():
            setattr(w, k, ptr(v))
        return w

    def forward_scheduled(self, params, features, fmap, caps: torch.Tensor, lengths, sample_prob: float, pick: str = "sample",
                          coin_u: Optional[torch.Tensor] = None, noise_u: Optional[torch.Tensor] = None, seed: int = 0,
                          tmax: Optional[int] = None, state=None, dropout: float = 0.0, dropout_seed: int = 0,
                          keep_u: Optional[torch.Tensor] = None):
        """gic_attn_forward_ss: ``forward_tf(pretrain=True, want_alphas=True, keep_state=True)`` with scheduled sampling
        (DecoderEngine.forward_scheduled).  Returns (pred, (h_n, c_n), alphas, saved, inputs, replaced).  ``state`` as forward_tf;
        ``dropout`` / ``dropout_seed`` / ``keep_u`` as there (gic_attn_forward_ss_drop)."""
        head, *rest = self._tf_forward(params, features, fmap, caps, lengths, tmax, state, True, (sample_prob, pick, coin_u, noise_u, seed),
                                       drop=(dropout, dropout_seed, keep_u))
        return (*head, *rest)

    def forward_tf_bwd(self, params, saved, pred: torch.Tensor, d_pred: Optional[torch.Tensor], temperature: float, pretrain: bool = False,
                       d_alphas: Optional[torch.Tensor] = None, ws=None, grads=None, dropout: float = 0.0, dropout_seed: int = 0,
                       keep_u: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """gic_attn_forward_tf_bwd: gradients of a loss on ``pred`` (``d_pred``; None = zeros) and on the alphas (``d_alphas`` f32
        [B, Tmax, P] or None) of the ``forward_tf(..., keep_state=True)`` call that returned ``saved``; ordered as ``sample_bwd``'s
        (parameters in NAMES order, then d features).  ``dropout`` / ``dropout_seed`` / ``keep_u`` as DecoderEngine.forward_tf_bwd."""
        return self._tf_backward(params, saved, pred, d_pred, d_alphas, temperature, pretrain, ws, grads, (dropout, dropout_seed, keep_u))

    def rollout_ws_bytes(self, B: int, Lc: int, rows: int) -> int:
        """Bytes of gic_attn_rollout's workspace (host-only query)."""
        out = C.c_uint64(0)
        L.check(L.load().gic_attn_rollout_ws_bytes(C.byref(self.dims(B, Lc)), int(rows), C.byref(out)), "gic_attn_rollout_ws_bytes")
        return int(out.value)

    def rollout(self, params, tf_saved, Y: torch.Tensor, num_rollouts: int, noise_u: Optional[torch.Tensor] = None, seed: int = 0,
                ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gic_attn_rollout: the SeqGAN step's Monte-Carlo roll-outs of the captions ``Y`` int64 [B, L].  ``tf_saved``: what
        ``forward_tf(params, features, fmap, Y[:, :-1], L, ..., keep_state=True)`` returned last (the roll-outs join at their prefix
        length from its state and read its feature map).  Returns ids int64 [(L-1)*N*B, L], row (t-1)*N*B + n*B + b = roll-out n of
        caption b with the prefix Y[b, :t].  ``noise_u`` f32 [L, (L-1)*N*B, V] or None = Philox(seed)."""
        self.check_params(params)
        require_gpu(Y, noise_u)
        B, Lc = Y.shape
        N = int(num_rollouts)
        rows = (Lc - 1) * N * B
        if Y.dtype != torch.int64 or N < 1 or Lc < 2:
            raise ValueError("rollout: Y must be int64 [B, L] with L >= 2 and num_rollouts >= 1")
        if tf_saved["T"] != Lc or tf_saved["Tmax"] != Lc or tuple(tf_saved["st"]["xh"].shape) != (Lc + 1, B, self.ldx):
            raise ValueError(f"rollout: tf_saved must come from forward_tf along Y[:, :-1] with every length L={Lc}")
        if noise_u is not None:
            if tuple(noise_u.shape) != (Lc, rows, self.V) or noise_u.dtype != torch.float32:
                raise ValueError(f"noise_u must be float32 [L={Lc}, rows={rows}, V={self.V}]")
            noise_u = noise_u.contiguous()
        dev = Y.device
        self.prepare(params)
        Y = Y.contiguous()
        flen = torch.arange(1, Lc, device=dev, dtype=torch.int32).repeat_interleave(N * B)
        act = _arr(C.c_int32, Lc, [min(t, Lc - 1) * N * B for t in range(Lc)])
        ws = _aligned_ws(ws, self.rollout_ws_bytes(B, Lc, rows), dev)
        ids = torch.empty(rows, Lc, device=dev, dtype=torch.int64)
        st = tf_saved["st"]
        L.check(L.load().gic_attn_rollout(
            C.byref(self.dims(B, Lc)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            ptr(st["fmap"]), ptr(Y), rows, ptr(flen), C.cast(act, C.c_void_p), ptr(noise_u), int(seed) & (2 ** 64 - 1), ptr(ws), ptr(ids),
            stream_ptr()), "gic_attn_rollout")
        return ids

    def alloc_bwd_ws(self, B: int, Lc: int, dev):
        f32 = torch.float32
        return {
            "dlogits": torch.empty(B, Lc, self.V, device=dev, dtype=self.act),
            "dhout": torch.empty(B, Lc, self.H, device=dev, dtype=f32),
            "dgates": torch.empty(Lc, B, 4 * self.H, device=dev, dtype=self.act),
            "dc": torch.empty(B, self.H, device=dev, dtype=f32),
            "dz": torch.empty(B, self.C, device=dev, dtype=f32),
            "dalpha": torch.empty(B, self.P, device=dev, dtype=f32),
            "dh_extra": torch.empty(B, self.H, device=dev, dtype=f32),
            "dhproj": torch.empty(Lc, B, self.A, device=dev, dtype=self.act),
            "dfproj": torch.empty(B, self.P, self.A, device=dev, dtype=f32),
            "dfproj_act": None if self.dt == L.F32 else torch.empty(B, self.P, self.A, device=dev, dtype=self.act),
            "dwa_rows": torch.empty(B, self.A, device=dev, dtype=f32),
            "dx": torch.empty(Lc * B, self.E, device=dev, dtype=f32),
        }

    def sample_bwd(self, params, st, out, ids, d_out, temperature: float, pretrain: bool = False, ws=None, grads=None, dev_scalars=None):
        """Returns [grads in NAMES order ..., d_features].  ``ws`` (alloc_bwd_ws) / ``grads`` (12 tensors): caller-owned buffers."""
        B, Lc = ids.shape
        dev = out.device
        d_out = _to_act(d_out, self.act)
        self.prepare(params)
        ws = ws if ws is not None else self.alloc_bwd_ws(B, Lc, dev)
        w = self._bwd_ws_struct(ws)
        grads = grads if grads is not None else self.alloc_grads(params, B)
        L.check(L.load().gic_attn_sample_bwd(
            C.byref(self.dims(B, Lc)), C.byref(self._pstruct(params)), C.byref(self._shadow_struct(params)), C.byref(self._state_struct(st)),
            C.byref(w), ptr(st["fmap"]), ptr(out), ptr(ids), ptr(d_out), float(temperature), int(bool(pretrain)),
            C.byref(self._pstruct(grads[:-1], L.AttnGrads, grads[-1])), dev_scalars.ptr if dev_scalars is not None else None, stream_ptr()),
            "gic_attn_sample_bwd")
        return grads
