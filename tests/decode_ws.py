"""What a caption-decode head (csrc/decode.hip) writes, reads and leaves behind, and the tools that pin it (no GPU at import).

The contract these tools check.  Every search and sampler runs inside one caller-owned workspace (and, with decode constraints, a
second one for the ban lists), documented as reusable across calls.  A head therefore
  * writes nothing outside the ``*_ws_bytes`` bytes of its workspaces and outside its output tensors,
  * reads no state word of the workspace before its own init kernels have written it: whatever an earlier call -- or nobody -- left
    in the buffer cannot change a result,
  * writes every element of ids / scores / lengths / met / alphas (ids past a caption's length hold pad_id),
  * leaves its inputs and the weights as they were.

The tools: a replica of the workspace layout (``decode_regions`` .. ``constraints_regions``, derived from the header comment of
decode.hip; tests/test_decode_ws.py pins its total against the eleven ``gic_*_ws_bytes`` queries), ``Banded`` buffers (the live part
inside one allocation with sentinel bands of 64 KiB on both sides, so a stray write lands in memory the test owns), the ``Harness``
that hands an engine module banded workspaces and banded, pre-filled outputs for the duration of a call, the three prior contents of
a workspace (``ZERO``, ``KEEP`` after a finished twin search, ``POISON``) and the checker (``Harness.check``, ``same_bits``,
``run_priors``)."""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple

import torch

ALIGN = 256                     # every region of a workspace, and the workspace itself
BAND = 64 * 1024                # bytes of sentinel on either side of a banded buffer
BAND_BYTE = 0xA5
TILE = 64                       # beam.h kBeamTile: nblk = ceil(V / 64)
HOP_MAX = 12                    # beam.h kHopMax = C * D at its largest
F32, BF16 = 0, 1

ZERO, KEEP, POISON = "zeros", "finished twin", "typed poison"

# pre-fill of the outputs: an id outside [0, V), NaN, a negative count
IDS_FILL_ABOVE_V = 1000
LEN_FILL = -3
MET_FILL = -5


class Dims(NamedTuple):
    """A decode's dims: the LSTM decoder's (C = 0) or the attention decoder's (NL = 1)."""
    B: int
    L: int
    V: int
    E: int
    H: int
    NL: int = 1
    C: int = 0
    P: int = 0
    A: int = 0

    @property
    def attn(self):
        return self.C > 0


class Region(NamedTuple):
    name: str                   # unique within a workspace ("m1.xh0": member 1's, "cws0.ban": the forced head's own ban list)
    role: str                   # what the bytes are (a key of int_ranges() for the integer regions)
    kind: str                   # "f32", "act" (the compute dtype) or "i32"
    shape: tuple
    offset: int
    nbytes: int


class _Carver:
    def __init__(self, dt, at=0):
        self.asz = 2 if dt == BF16 else 4
        self.at = at
        self.regions = []

    def take(self, name, role, kind, *shape):
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * (self.asz if kind == "act" else 4)
        self.regions.append(Region(name, role, kind, tuple(int(s) for s in shape), self.at, nbytes))
        self.at += (nbytes + ALIGN - 1) & ~(ALIGN - 1)


def is_fused(d: Dims, K: int, fused_rows: int) -> bool:
    """Attention, or B * K rows within gic_decoder_fused_rollout_rows (512 where the shapes qualify, 0 where they do not)."""
    return d.attn or d.B * K <= fused_rows


def _recurrent(cv, d, K, fused, pre=""):
    """recurrent_layout: one recurrence's own regions."""
    R = d.B * K
    for l in range(d.NL):
        din = d.E + d.C if l == 0 else d.H
        cv.take(f"{pre}xh{l}", "xh", "act", 2, R, din + d.H)
        cv.take(f"{pre}c{l}", "c", "f32", 2, R, d.H)
    if not fused:
        cv.take(pre + "gpre", "gpre", "f32", R, 4 * d.H)
    if d.attn:
        cv.take(pre + "fproj", "fproj", "act", d.B, d.P, d.A)
        cv.take(pre + "hp", "hp", "f32", R, d.A)
        cv.take(pre + "e", "e", "f32", R, d.P)


def _decode(cv, d, K, beam, fused, ensemble):
    """decode_layout: the regions of one search, in the header comment's order."""
    R, nblk = d.B * K, -(-d.V // TILE)
    _recurrent(cv, d, K, fused)
    if d.attn and beam and not ensemble:
        cv.take("ahist", "ahist", "f32", d.L, R, d.P)
    if not beam or not fused or ensemble:
        cv.take("logits", "logits", "f32", R, d.V)
    if beam:
        cv.take("pm", "pm", "f32", R, nblk)
        cv.take("ps", "ps", "f32", R, nblk)
        cv.take("pv", "pv", "f32", R, nblk, K)
        cv.take("pi", "pi", "i32", R, nblk, K)
    cv.take("score", "score", "f32", R)
    for name in ("fin", "len", "tok", "par"):
        cv.take(name, name, "i32", R)
    cv.take("htok", "htok", "i32", d.L, R)
    if beam:
        cv.take("hpar", "hpar", "i32", d.L, R)
    if beam and d.attn and not ensemble:
        cv.take("anc", "anc", "i32", d.B, K, d.L)
    cv.take("last", "last", "i32", d.B)
    cv.take("done", "done", "i32", d.B)
    cv.take("count", "count", "i32", 1)


def _constraints(cv, rows, L, S, pre=""):
    cv.take(pre + "nban", "nban", "i32", rows)
    cv.take(pre + "ban", "ban", "i32", rows, S + 1 + L)
    cv.take(pre + "hist", "hist", "i32", 2, rows, L)


def decode_regions(d: Dims, K: int, dt: int, beam: bool, fused: bool):
    """(regions, total bytes) of gic_*_beam_ws_bytes (beam) / gic_*_sample_ws_bytes: decode_layout of decode.hip."""
    cv = _Carver(dt)
    _decode(cv, d, K, beam, fused, False)
    return cv.regions, cv.at


def ensemble_regions(d: Dims, K: int, dt: int, beam: bool, fused: bool, M: int):
    """gic_*_ensemble_*_ws_bytes: ensemble_layout -- the search with the logits and without ahist / anc, the slabs, then the recurrent
    regions of members 1..M-1."""
    cv = _Carver(dt)
    _decode(cv, d, K, beam, fused, True)
    cv.take("slabs", "slabs", "f32", M, d.B * K, d.V)
    for m in range(1, M):
        _recurrent(cv, d, K, fused, f"m{m}.")
    return cv.regions, cv.at


def forced_regions(d: Dims, K: int, dt: int, fused: bool):
    """gic_*_forced_beam_ws_bytes: forced_layout -- the beam search's regions, the hop lists, init and a ban-list workspace at S = 0."""
    cv = _Carver(dt)
    _decode(cv, d, K, True, fused, False)
    R = d.B * K
    cv.take("hop_id", "hop_id", "i32", R, HOP_MAX)
    cv.take("hop_tgt", "hop_tgt", "i32", R, HOP_MAX)
    cv.take("hop_val", "hop_val", "f32", R, HOP_MAX)
    cv.take("init", "init", "i32", d.B)
    _constraints(cv, R, d.L, 0, "cws0.")
    return cv.regions, cv.at


def constraints_regions(rows: int, L: int, S: int):
    """gic_decode_constraints_ws_bytes: constraints_layout."""
    cv = _Carver(F32)
    _constraints(cv, rows, L, S)
    return cv.regions, cv.at


def region_table(regions):
    return "\n".join(f"  {r.name:<10} {r.kind} {list(r.shape)} @ {r.offset} ({r.nbytes} bytes)" for r in regions)


# ------------------------------------------------------------------------------------------------ prior contents
def int_ranges(d: Dims, K: int, S: int, n_sets: int):
    """[lo, hi] (inclusive) of the values each integer region can legally hold in a search of these dims."""
    R = d.B * K
    return {"fin": (0, 1), "done": (0, 1), "count": (0, R), "len": (0, d.L), "tok": (0, d.V - 1), "par": (0, R - 1), "hpar": (0, K - 1),
            "anc": (-1, R - 1), "htok": (0, d.V - 1), "pi": (0, d.V - 1), "last": (-1, d.L - 1), "init": (0, (1 << n_sets) - 1),
            "hop_id": (-1, d.V - 1), "hop_tgt": (0, (1 << n_sets) - 1), "nban": (0, S + 1 + d.L), "ban": (0, d.V - 1), "hist": (0, d.V - 1)}


def poison_ints(d: Dims, K: int, eos_id: int, S: int):
    """The integer regions' poison: legal for this search, and as misleading as a legal value gets (a finished search that ran L
    steps on <E>).  ``S``: num_suppress of the workspace the value goes into (nban = the list's capacity)."""
    return {"fin": 1, "done": 1, "count": d.B * K, "len": d.L, "tok": eos_id, "par": 0, "hpar": 0, "anc": 0, "htok": 3, "pi": d.V - 1,
            "last": 0, "init": 1, "hop_id": 3, "hop_tgt": 0, "nban": S + 1 + d.L, "ban": 3, "hist": 3}


def region_view(live: torch.Tensor, r: Region, dt: int) -> torch.Tensor:
    """The bytes of region ``r`` of the workspace ``live`` (uint8) in the region's own type and shape."""
    ty = torch.int32 if r.kind == "i32" else torch.bfloat16 if (r.kind == "act" and dt == BF16) else torch.float32
    return live[r.offset:r.offset + r.nbytes].view(ty).view(r.shape)


def write_poison(live: torch.Tensor, regions, dt: int, ints: dict, ranges: dict) -> None:
    """Typed poison.  Float and act regions get NaN in their own type; the bytes between regions get zero.  An integer region never
    receives NaN bits, 0xFF bytes or any value outside the index range it can legally hold. A premature read must change a result,
    never form a wild address."""
    live.zero_()
    for r in regions:
        v = region_view(live, r, dt)
        if r.kind == "i32":
            lo, hi = ranges[r.role]
            assert lo <= ints[r.role] <= hi, f"poison {ints[r.role]} of region {r.name} outside its legal range [{lo}, {hi}]"
            v.fill_(int(ints[r.role]))
        else:
            v.fill_(float("nan"))


# ------------------------------------------------------------------------------------------------ banded buffers
class Banded:
    """``nbytes`` live bytes, 256-byte aligned, inside one larger allocation with bands of at least 64 KiB of BAND_BYTE on both
    sides.  ``typed(dtype, shape)`` views the live part."""

    def __init__(self, nbytes: int, dev, name: str):
        self.name, self.nbytes = name, int(nbytes)
        self.flat = torch.full((self.nbytes + 2 * BAND + ALIGN,), BAND_BYTE, dtype=torch.uint8, device=dev)
        self.lo = BAND + (-(self.flat.data_ptr() + BAND)) % ALIGN
        self.live = self.flat[self.lo:self.lo + self.nbytes]
        assert self.live.data_ptr() % ALIGN == 0 and self.lo >= BAND and self.flat.numel() - self.lo - self.nbytes >= BAND

    def typed(self, dtype, shape):
        return self.live.view(dtype).view(tuple(shape))

    def breach(self):
        """None, or where the bands changed: (side, the byte's distance from the live part, its value)."""
        for side, band in (("below", self.flat[:self.lo].flip(0)), ("above", self.flat[self.lo + self.nbytes:])):
            bad = (band != BAND_BYTE).nonzero()
            if bad.numel():
                i = int(bad[0])
                return side, i + 1 if side == "below" else i, int(band[i])
        return None


def banded_tensor(t: torch.Tensor, dev, name: str):
    """(the Banded buffer, its typed live view holding a copy of ``t``)."""
    t = t.contiguous()
    b = Banded(t.numel() * t.element_size(), dev, name)
    v = b.typed(t.dtype, t.shape)
    v.copy_(t)
    return b, v


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.uint8).cpu().clone()          # (a copy on the CPU too, where .cpu() aliases)


class OutSpec(NamedTuple):
    """What the outputs of a call must look like: tokens in [0, V), pad_id past lengths, lengths in [0, L].  ``dead_ok``: the forced
    head alone may return dead beams (length 0, all pad, score -inf by gicap.h); every other score is finite."""
    V: int
    L: int
    pad_id: int = 0
    dead_ok: bool = False


class Harness:
    """Substitutes the allocation helpers of an engine module (``_aligned_ws``, ``_decode_outputs`` and, for met / alphas, ``torch.empty``
    behind a proxy) for the duration of ``call``.  The workspaces persist across calls of one Harness -- request i of every call gets
    the same banded buffer (0: the workspace, 1: the constraint workspace), after ``prior(i, live)`` has prepared its contents -- and
    the outputs are fresh banded tensors holding the pre-fill."""

    def __init__(self, module, dev, spec: OutSpec, extra_shapes=()):
        self.E, self.dev, self.spec = module, dev, spec
        self.extra_shapes = {(tuple(s), dt) for s, dt in extra_shapes}          # the met / alphas shapes the proxy bands
        self.ws = []
        self.inputs = {}          # name -> (Banded or None, live view, bits before the call)
        self.outs = []            # this call's (name, Banded, view)

    # -- inputs
    def put(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """A banded copy of an input tensor; the call must leave it bit-equal."""
        b, v = banded_tensor(t.to(self.dev), self.dev, name)
        self.inputs[name] = (b, v, _bits(v))
        return v

    def watch(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """A parameter tensor (not banded): the call must leave it bit-equal."""
        self.inputs[name] = (None, t, _bits(t))
        return t

    # -- the substitutes
    def _aligned_ws(self, ws, nbytes, dev):
        i = self._i
        self._i += 1
        if i == len(self.ws):
            self.ws.append(Banded(nbytes, self.dev, "the workspace" if i == 0 else "the constraint workspace"))
        b = self.ws[i]
        assert b.nbytes == int(nbytes), f"workspace request {i}: {nbytes} bytes now, {b.nbytes} in the earlier call"
        self._prior(i, b.live)
        return b.live

    def _out(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= int(s)
        b = Banded(n * torch.empty((), dtype=dtype).element_size(), self.dev, name)
        v = b.typed(dtype, shape)
        if dtype == torch.int64:
            v.fill_(self.spec.V + IDS_FILL_ABOVE_V)
        elif dtype == torch.int32:
            v.fill_(LEN_FILL if name == "lengths" else MET_FILL)
        else:
            v.fill_(float("nan"))
        self.outs.append((name, b, v))
        return v

    def _decode_outputs(self, B, n, Lc, dev):
        return (self._out("ids", (B, n, Lc), torch.int64), self._out("scores", (B, n), torch.float32),
                self._out("lengths", (B, n), torch.int32))

    class _Torch:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            return getattr(torch, name)

        def empty(self, *shape, device=None, dtype=torch.float32, **kw):
            shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(int(s) for s in shape)
            if (shape, dtype) in self._h.extra_shapes:
                return self._h._out("met" if dtype == torch.int32 else "alphas", shape, dtype)
            return torch.empty(*shape, device=device, dtype=dtype, **kw)

    @contextlib.contextmanager
    def call(self, prior):
        """``prior(i, live)`` prepares workspace request i (0: the workspace, 1: the constraint workspace) before the head sees it."""
        self._i, self._prior, self.outs = 0, prior, []
        saved = (self.E._aligned_ws, self.E._decode_outputs, self.E.torch)
        self.E._aligned_ws, self.E._decode_outputs, self.E.torch = self._aligned_ws, self._decode_outputs, Harness._Torch(self)
        try:
            yield self
        finally:
            self.E._aligned_ws, self.E._decode_outputs, self.E.torch = saved

    # -- the checks after a call
    def check(self, what: str):
        """Checks 1-3 of the contract on the call that just ran; returns {name: the output on the CPU}."""
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        sp = self.spec
        for b in self.ws + [o[1] for o in self.outs] + [i[0] for i in self.inputs.values() if i[0] is not None]:
            hit = b.breach()
            assert hit is None, f"{what}: a write outside {b.name}: byte {hit[1]} {hit[0]} it holds {hit[2]:#x}, not the band's {BAND_BYTE:#x}"
        for name, (_, v, before) in self.inputs.items():
            assert torch.equal(_bits(v), before), f"{what}: the call changed its input {name}"
        out = {name: v.detach().cpu().clone() for name, _, v in self.outs}
        assert {"ids", "scores", "lengths"} <= set(out), f"{what}: outputs allocated: {sorted(out)}"
        ids, scores, lengths = out["ids"], out["scores"], out["lengths"].long()
        left = (ids == sp.V + IDS_FILL_ABOVE_V)
        assert not left.any(), f"{what}: {int(left.sum())} elements of ids were never written, the first at {left.nonzero()[0].tolist()}"
        assert not (out["lengths"] == LEN_FILL).any(), f"{what}: lengths holds unwritten elements"
        assert not torch.isnan(scores).any(), f"{what}: scores holds NaN (unwritten, or computed from stale values)"
        assert ((lengths >= 0) & (lengths <= sp.L)).all(), f"{what}: lengths outside [0, {sp.L}]: {lengths.tolist()}"
        assert ((ids >= 0) & (ids < sp.V)).all(), f"{what}: ids outside [0, {sp.V}): {ids[(ids < 0) | (ids >= sp.V)].tolist()[:8]}"
        past = torch.arange(sp.L)[None, None] >= lengths[..., None]
        bad = past & (ids != sp.pad_id)
        assert not bad.any(), (f"{what}: ids past a caption's length must be <PAD> ({sp.pad_id}): {ids[bad].tolist()[:8]} at "
                               f"{bad.nonzero()[:4].tolist()} (lengths {lengths.tolist()})")
        dead = lengths == 0
        if sp.dead_ok:
            assert (scores[dead] == -math.inf).all(), f"{what}: a dead beam (length 0) must score -inf"
        else:
            assert not dead.any(), f"{what}: a caption of length 0"
        assert torch.isfinite(scores[~dead]).all(), f"{what}: scores not finite: {scores.tolist()}"
        if "met" in out:
            assert not (out["met"] == MET_FILL).any() and (out["met"] >= 0).all(), f"{what}: met holds unwritten elements: {out['met'].tolist()}"
        if "alphas" in out:
            assert not torch.isnan(out["alphas"]).any(), f"{what}: alphas holds NaN (unwritten rows, or computed from stale values)"
        return out


def same_bits(what: str, prior: str, got: dict, want: dict) -> None:
    """Check 5: a run on other prior contents of the workspaces returns the bits of the run on zeros, in every output."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name in ("ids", "lengths", "scores", "met", "alphas"):
        if name in want and not torch.equal(_bits(got[name]), _bits(want[name])):
            g, w = got[name], want[name]
            where = (g != w).nonzero()
            at = where[0].tolist() if where.numel() else "?"
            raise AssertionError(f"{what}: the run on a workspace holding {prior} differs from the run on zeros in {name} "
                                 f"({int((g != w).sum())} elements, the first at {at}: {g[tuple(at)] if at != '?' else ''} for "
                                 f"{w[tuple(at)] if at != '?' else ''}): the head read workspace state it had not written")


def run_priors(h: Harness, what: str, call, twin, poison):
    """The three prior contents of one case.  ``call()`` runs the head under test through the engine wrappers, ``twin()`` a completed
    search of the same head, dims and K on other weights and features; ``poison(i, live)`` writes the typed poison of workspace
    request i.  Returns the outputs of the run on zeros (checks 1-3 hold for all four calls, check 5 for the two other priors)."""
    with h.call(lambda i, live: live.zero_()):
        call()
    first = h.check(f"{what} [on {ZERO}]")
    with h.call(lambda i, live: None):
        twin()
    h.check(f"{what} [the twin search]")
    with h.call(lambda i, live: None):
        call()
    same_bits(what, KEEP, h.check(f"{what} [on {KEEP}]"), first)
    with h.call(poison):
        call()
    same_bits(what, POISON, h.check(f"{what} [on {POISON}]"), first)
    return first


# ------------------------------------------------------------------------------------------------ check 4: the oracles' criteria
def compare_beam(what, got, want, margins, k, G, rtol, atol, alphas=None, ralphas=None, every=True):
    """The criterion of tests/test_gpu_beam.py::_check_vs_oracle (G = 1) and tests/test_gpu_diverse_beam.py::_compare (per group): on the
    images whose selection the oracle decides by >= 1e-4, the same beams in every group, in the same order where the order is decided
    by >= 1e-4 too (else as sets); scores within the head's own rtol / atol; each returned beam's alphas those of the oracle's beam
    with its ids.  ``every``: the cases are seeded so that the oracle decides every image (tests/test_decode_ws.py asserts it)."""
    ids, sc, ln = got["ids"], got["scores"].double(), got["lengths"].long()
    rid, rsc, rlen = want
    kg = k // G
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    assert not every or len(ok) == len(margins), f"{what}: the oracle leaves images undecided: margins {margins}"
    for b in ok:
        for g in range(G):
            s = slice(g * kg, (g + 1) * kg)
            if margins[b][1] >= 1e-4:
                assert torch.equal(ids[b, s], rid[b, s]), f"{what}: image {b}, group {g}: ids {ids[b, s].tolist()} for {rid[b, s].tolist()}"
                assert torch.equal(ln[b, s], rlen[b, s]), f"{what}: image {b}, group {g}: lengths {ln[b, s].tolist()} for {rlen[b, s].tolist()}"
                torch.testing.assert_close(sc[b, s], rsc[b, s], rtol=rtol, atol=atol, msg=lambda m: f"{what}: image {b}, group {g}: scores: {m}")
            else:
                assert sorted(zip(ids[b, s].tolist(), ln[b, s].tolist())) == sorted(zip(rid[b, s].tolist(), rlen[b, s].tolist())), \
                    f"{what}: image {b}, group {g}: the set of beams differs"
                torch.testing.assert_close(sc[b, s].sort().values, rsc[b, s].sort().values, rtol=rtol, atol=atol,
                                           msg=lambda m: f"{what}: image {b}, group {g}: scores: {m}")
            if alphas is not None:
                for j in range(g * kg, (g + 1) * kg):
                    r = next(i for i in range(g * kg, (g + 1) * kg) if torch.equal(rid[b, i], ids[b, j]))
                    torch.testing.assert_close(alphas[b, j].double(), ralphas[b, r], rtol=1e-4, atol=1e-6,
                                               msg=lambda m: f"{what}: image {b}, beam {j}: alphas: {m}")
    return ok


def compare_forced(what, got, want, sets, K, pad_id, absent_mask, ralphas=None):
    """The criterion of tests/test_gpu_forced_beam.py::test_f32_matches_oracle: rtol 1e-4 / atol 1e-5."""
    ids, sc, ln, met = got["ids"], got["scores"].double(), got["lengths"].long(), got["met"].long()
    rid, rsc, rln, rmet, margins = want[:5]
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    assert len(ok) == len(margins), f"{what}: the oracle leaves images undecided: margins {margins}"
    for b in ok:
        init = absent_mask(sets[b])
        live = rln[b] > 0
        assert torch.equal(ln[b] > 0, live), f"{what}: image {b}: dead beams in other slots: lengths {ln[b].tolist()} for {rln[b].tolist()}"
        assert (sc[b][~live] == -math.inf).all() and (ids[b][~live] == pad_id).all() and (met[b][~live] == init).all(), f"{what}: image {b}: a dead beam"
        if margins[b][1] >= 1e-4:
            assert torch.equal(ids[b], rid[b]) and torch.equal(ln[b], rln[b]) and torch.equal(met[b], rmet[b]), \
                f"{what}: image {b}: ids {ids[b].tolist()} lengths {ln[b].tolist()} met {met[b].tolist()} for {rid[b].tolist()} {rln[b].tolist()} {rmet[b].tolist()}"
            torch.testing.assert_close(sc[b][live], rsc[b][live], rtol=1e-4, atol=1e-5, msg=lambda m: f"{what}: image {b}: scores: {m}")
        else:
            real = lambda m: [bin(int(v) & ~init).count("1") for v in m]     # noqa: E731
            assert real(met[b]) == real(rmet[b]), f"{what}: image {b}: constraints met {met[b].tolist()} for {rmet[b].tolist()}"
            for n in set(real(met[b][live])):
                s = live & (torch.tensor(real(rmet[b])) == n)
                key = lambda i, l, m: sorted(zip(i[s].tolist(), l[s].tolist(), m[s].tolist()))     # noqa: E731
                assert key(ids[b], ln[b], met[b]) == key(rid[b], rln[b], rmet[b]), f"{what}: image {b}: the beams that meet {n} constraints differ"
                torch.testing.assert_close(sc[b][s].sort().values, rsc[b][s].sort().values, rtol=1e-4, atol=1e-5,
                                           msg=lambda m: f"{what}: image {b}: scores: {m}")
        if ralphas is not None:
            for j in range(K):
                r = next(i for i in range(K) if torch.equal(rid[b, i], ids[b, j]) and rln[b, i] == ln[b, j])
                torch.testing.assert_close(got["alphas"][b, j].double(), ralphas[b, r], rtol=1e-4, atol=1e-6,
                                           msg=lambda m: f"{what}: image {b}, beam {j}: alphas: {m}")
    return ok


def compare_rows(what, got, want, atol):
    """The samplers' criterion (tests/test_gpu_sample.py::test_lstm_f32_matches_oracle): the rows whose every draw and nucleus the
    oracle decides by > 1e-5 -- here every row, by the choice of seeds -- have the oracle's ids and lengths; scores rtol 1e-5 and the
    head's atol (1e-4; an ensemble's adds the mix kernel's bound)."""
    rid, rsc, rlen, margin = want
    ok = margin > 1e-5
    assert ok.all(), f"{what}: the oracle leaves rows undecided: margins {margin.tolist()}"
    assert torch.equal(got["ids"], rid), f"{what}: ids {got['ids'].tolist()} for {rid.tolist()}"
    assert torch.equal(got["lengths"].long(), rlen), f"{what}: lengths {got['lengths'].tolist()} for {rlen.tolist()}"
    torch.testing.assert_close(got["scores"].double(), rsc, rtol=1e-5, atol=atol, msg=lambda m: f"{what}: scores: {m}")
