"""gic_attn_rollout / gic_attn_rollout_ws_bytes (the attention decoder's Monte-Carlo roll-outs, --adv-mode seqgan --decoder attention)
without a GPU: the new C ABI symbols, the argument checks (all before any launch), the host-only workspace query -- smaller than one
replicated feature projection and affine in the rows -- the plain-torch oracle's own consistency and the instructor's mode check."""
import ctypes
import os
import re

import pytest
import torch

from oracle import cpu_attention as CA
from tests import attn_seqgan_oracle as SO

SYMBOLS = ("gic_attn_rollout_ws_bytes", "gic_attn_rollout")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = (32, 20, 10000, 512, 512, 2048, 49, 512, 1)          # B, L, V, E, H, C, P, A, bf16


def _lib():
    from gan_image_captioning_amd import _lib
    return _lib, _lib.load()


def test_symbols_agree_across_header_lib_and_so():
    L_, lib = _lib()
    with open(os.path.join(ROOT, "include", "gicap.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % s, header)
        assert m, s
        assert s in L_._SIGNATURES and s in L_.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
        assert len(L_._SIGNATURES[s][1]) == len(m.group(1).split(",")), s
    assert lib.gic_abi_version() == 5 and re.search(r"#define\s+GIC_ABI_VERSION\s+5\b", header)


def _rollout(lib, L_, dims, rows=6, active=None, null=(), ws=256):
    p, s, st = L_.AttnParams(), L_.AttnShadow(), L_.AttnState()
    for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
        setattr(p, n, 256)
    for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
        setattr(s, n, 256)
    for n in ("xh", "gates", "c", "hout", "part", "fproj", "alpha", "hproj"):
        setattr(st, n, 256)
    Lc = dims.L if dims is not None else 4
    act = (ctypes.c_int32 * max(Lc, 1))(*(active if active is not None else [min(t, Lc - 1) * 2 for t in range(Lc)]))
    a = {"fmap": 256, "force_ids": 256, "force_len": 256, "act": ctypes.cast(act, ctypes.c_void_p), "ws": ws, "ids": 256}
    for n in null:
        a[n] = None
    return lib.gic_attn_rollout(ctypes.byref(dims) if dims is not None else None, ctypes.byref(p), ctypes.byref(s),
                                None if "state" in null else ctypes.byref(st), a["fmap"], a["force_ids"], rows, a["force_len"], a["act"],
                                None, 0, a["ws"], a["ids"], None)


def test_rollout_argument_checks_return_before_any_launch():
    """Every refused call returns INVALID_ARG with a text; none of them reaches a launch (there is no GPU here, and the pointers
    are not memory)."""
    L_, lib = _lib()
    good = L_.AttnDims(2, 4, 32, 8, 8, 8, 5, 8, 0)
    err = lambda: lib.gic_last_error().decode()                 # noqa: E731
    for null in ("fmap", "force_ids", "force_len", "act", "ws", "ids", "state"):
        assert _rollout(lib, L_, good, null=(null,)) == -1, null
        assert "null" in err()
    assert _rollout(lib, L_, None) == -1 and "null dims" in err()
    for rows in (0, -3):
        assert _rollout(lib, L_, good, rows=rows) == -1 and "rows" in err()
    assert _rollout(lib, L_, good, active=[1, 2, 4, 6]) == -1 and "host_active_rows[0]" in err()
    assert _rollout(lib, L_, good, active=[0, 4, 2, 6]) == -1 and "non-decreasing" in err()
    assert _rollout(lib, L_, good, active=[0, 2, 4, 7]) == -1 and "<= rows" in err()
    assert _rollout(lib, L_, good, ws=264) == -1 and "256-byte aligned" in err()
    for bad in (L_.AttnDims(2, 4, 30, 8, 8, 8, 5, 8, 0), L_.AttnDims(2, 4, 32, 8, 12, 8, 5, 8, 0), L_.AttnDims(2, 4, 32, 8, 8, 8, 1025, 8, 0),
                L_.AttnDims(2, 4, 32, 8, 8, 8, 5, 2056, 0), L_.AttnDims(2, 4, 32, 8, 8, 8, 5, 8, 7)):
        assert _rollout(lib, L_, bad) == -1 and "attn:" in err()
        out = ctypes.c_uint64(0)
        assert lib.gic_attn_rollout_ws_bytes(ctypes.byref(bad), 6, ctypes.byref(out)) == -1
    assert _rollout(lib, L_, L_.AttnDims(2, 1, 32, 8, 8, 8, 5, 8, 0), active=[0]) == -1 and "L must be" in err()


def _ws(lib, L_, dims, rows):
    out = ctypes.c_uint64(0)
    assert lib.gic_attn_rollout_ws_bytes(ctypes.byref(L_.AttnDims(*dims)), rows, ctypes.byref(out)) == 0, lib.gic_last_error()
    return out.value


def test_workspace_is_host_only_smaller_than_one_replicated_fproj_and_affine_in_rows():
    from gan_image_captioning_amd import engine
    L_, lib = _lib()
    rows = 19 * 16 * 32
    assert rows == 9728
    n = _ws(lib, L_, BENCH, rows)
    assert 0 < n < 9728 * 49 * 512 * 2                          # one replicated fproj: the workspace cannot hold per-row image data
    assert n - _ws(lib, L_, BENCH, 4864) == _ws(lib, L_, BENCH, 14592) - n > 0
    assert engine.AttnDecoderEngine(10000, 512, 512, 2048, 49, 512, 1).rollout_ws_bytes(32, 20, rows) == n
    # the logits scratch covers exactly the steps the fused vocabulary product declines: with the product switched off (a fresh
    # process: the switch is read once) it covers every row, so that every step still has its plain product
    import subprocess
    import sys
    code = ("import ctypes, sys; sys.path.insert(0, %r); from gan_image_captioning_amd import _lib as L; lib = L.load(); "
            "o = ctypes.c_uint64(0); d = L.AttnDims(*%r); assert lib.gic_attn_rollout_ws_bytes(ctypes.byref(d), %d, ctypes.byref(o)) == 0; "
            "print(o.value)" % (ROOT, BENCH, rows))
    env = dict(os.environ, GIC_NO_FUSED_GUMBELMAX="1")
    off = int(subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()[-1])
    assert off - n == (rows - 256) * 10000 * 4                  # 256 rows of logits grow to all 9728
    # f32 mode keeps the logits of every row (the fused vocabulary product is bf16): still no [rows, P, .] term -- the same bytes at any P
    small = (4, 5, 64, 16, 32, 40, 49, 24, 0)
    assert _ws(lib, L_, small, 272) == _ws(lib, L_, small[:6] + (9,) + small[7:], 272)
    d = L_.AttnDims(*BENCH)
    out = ctypes.c_uint64(0)
    assert lib.gic_attn_rollout_ws_bytes(ctypes.byref(d), rows, None) == -1
    assert lib.gic_attn_rollout_ws_bytes(None, rows, ctypes.byref(out)) == -1
    assert lib.gic_attn_rollout_ws_bytes(ctypes.byref(d), 0, ctypes.byref(out)) == -1


def test_oracle_self_check_rollouts_keep_prefixes_and_continue_the_sampler():
    """A self-check of the test oracle, not of the feature (it passes without it), against oracle/cpu_attention.py: a roll-out row
    follows its caption's prefix, and with the noise of the caption's own draw from the prefix on it reproduces the caption (the
    roll-out IS the sampler resumed at the prefix)."""
    B, L, V, N = 3, 5, 12, 2
    g = torch.Generator().manual_seed(2)
    gp = {k: v * 6 for k, v in CA.make_attn_params(V, 8, 16, 8, 9, g).items()}
    feats = torch.randn(B, 8, generator=g) * 0.3
    fmap = torch.relu(torch.randn(B, 4, 8, generator=g))
    us = [torch.empty(B, V).uniform_(0, 1, generator=g) for _ in range(L)]
    Y = CA.attn_decoder_sample(gp, feats, fmap, L, 1.0, us)[1]
    rows = (L - 1) * N * B
    u_mc = torch.empty(L, rows, V).uniform_(0, 1, generator=g)
    u_mc[:, :B] = torch.stack(us)                               # rows 0..B-1: prefix length 1, roll-out 0, with Y's own noise
    mc, gap = SO.attn_rollouts(gp, feats, fmap, Y, N, u_mc)
    assert mc.shape == (rows, L) and gap > 0
    mc4 = mc.view(L - 1, N, B, L)
    for t in range(1, L):
        assert torch.equal(mc4[t - 1, :, :, :t], Y[None, :, :t].expand(N, B, t))
    assert torch.equal(mc[:B], Y)
    assert len(torch.unique(mc[:N * B], dim=0)) > 1


def test_attention_decoder_passes_the_instructors_mode_check_with_seqgan():
    """--decoder attention --adv-mode seqgan is no longer refused by the instructor's checks of the mode flags (the construction
    itself needs a GPU: the check is the unit); the flags it still refuses stay refused."""
    from gan_image_captioning_amd import seqgan, training
    from gan_image_captioning_amd.args import default_args
    args = default_args(decoder="attention", adv_mode="seqgan", conditional_gan=1)
    assert training.check_modes(args) == ("sample", 0.0)
    assert hasattr(seqgan.SeqGANStep, "_attn_step")
    with pytest.raises(ValueError):
        training.check_modes(default_args(decoder="lstm", attn_reg=0.5))
    with pytest.raises(ValueError):
        training.check_modes(default_args(pretrain_mode="both"))
