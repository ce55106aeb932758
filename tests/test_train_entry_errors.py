"""Which check of a teacher-forced entry point fires, and with which text: a recorded table (no GPU).

Every row of tests/golden/train_entry_errors.json is one invalid call of one of the nine teacher-forced entry points of
csrc/teacher_forced.hip -- gic_{decoder,attn}_forward_{tf,ss}, gic_attn_forward_tf_ws_bytes, gic_{decoder,attn}_forward_ss_ws_bytes
and gic_{decoder,attn}_forward_tf_bwd -- on fake (non-null, 16-byte aligned) pointers, with the (status, gic_last_error() text) it
returned.  Rows with two faults at once pin the ORDER of an entry point's checks (shapes, null arguments, caps, Tmax, the
scheduled-sampling options, the workspace's alignment, weights, state, workspace, gradients), and the last rows that the deterministic
mode refuses gic_attn_forward_ss and not gic_attn_forward_tf.

The table was recorded from the library of commit dac4657 ("Pin caption search at exact ties and over searches that run long"), the
last one in which the nine entry points were written out once per decoder (csrc/decoder.hip, csrc/attn_tf.hip): that commit built in
a checkout of its own, `_rows()` of this file run against its libgicap.so, the result dumped with json.dump(rows, f, indent=0).  It
is not regenerated from later code: a library that disagrees with a row has changed an error text or the order of its checks."""
import ctypes as C
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_entry_errors.json")
PTR = 256                                         # a fake pointer: non-null, aligned, never dereferenced by a call that is refused
NL = 2
LSTM_DIMS = dict(B=4, L=6, V=50, E=8, H=16, NL=NL, dtype=0)
ATTN_DIMS = dict(B=2, L=4, V=64, E=8, H=8, C=8, P=4, A=8, dtype=0)

# An argument list is spelled with: a name (a pointer argument, or one of the structs dims / P / S / st / w / G / opts), "Tmax", or a
# literal (the optional inputs stay null, the scalars are arbitrary).  After it: the struct fields the entry point checks, as
# "<struct>.<field>" and, for the LSTM decoder's per-layer arrays, "<struct>.<field>[<layer>]" with the layers 0..NL-1 it looks at.
_LAYERS = lambda s, names: tuple(f"{s}.{n}[{l}]" for l in range(NL) for n in names)        # noqa: E731
LSTM_FWD_FIELDS = ("P.embed", "P.b_out", "S.wout", "st.hout", "st.gpre") + _LAYERS("st", ("xh", "c")) + _LAYERS("S", ("wcat", "bsum"))
ATTN_WEIGHTS = tuple(f"P.{n}" for n in ("embed", "b_out", "b_f", "w_a")) + tuple(f"S.{n}" for n in ("wcat", "bsum", "wout", "wf", "wh"))
ATTN_STATE = tuple(f"st.{n}" for n in ("xh", "gates", "c", "hout", "fproj", "alpha", "hproj"))
ATTN_BWD_WS = tuple(f"w.{n}" for n in ("dlogits", "dhout", "dgates", "dc", "dz", "dalpha", "dh_extra", "dhproj", "dfproj", "dwa_rows", "dx"))
ATTN_GRADS = tuple(f"G.{n}" for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a", "features"))
# symbol -> (model, kind, argument list, checked struct fields)
ENTRIES = {
    "gic_decoder_forward_tf": ("lstm", "tf", ("dims", "P", "S", "st", "features", "caps", "lengths", "Tmax", None, 0, 1.0, 1, "logits_ws", "ids_ws",
                                              "out", "h_n", "c_n", None), LSTM_FWD_FIELDS),
    "gic_decoder_forward_ss": ("lstm", "ss", ("dims", "P", "S", "st", "features", "caps", "lengths", "Tmax", "opts", "ws", "out", "h_n", "c_n",
                                              None), LSTM_FWD_FIELDS),
    "gic_decoder_forward_tf_bwd": ("lstm", "bwd", ("dims", "P", "S", "st", "w", "pred", "caps", "lengths", "Tmax", "d_pred", 1.0, 1, "G", None),
                                   ("w.dlogits", "w.dhout", "st.hout", "S.wout", "G.embed", "G.w_out", "G.b_out", "G.features")
                                   + _LAYERS("st", ("xh", "c", "gates")) + _LAYERS("w", ("dgates", "dxh", "dc"))
                                   + _LAYERS("G", ("w_ih", "w_hh", "b_ih", "b_hh"))),
    "gic_attn_forward_tf": ("attn", "tf", ("dims", "P", "S", "st", "features", "fmap", "caps", "lengths", "Tmax", None, 0, 1.0, 1, "logits_ws",
                                           "out", None, "h_n", "c_n", None), ATTN_WEIGHTS + ATTN_STATE),
    "gic_attn_forward_ss": ("attn", "ss", ("dims", "P", "S", "st", "features", "fmap", "caps", "lengths", "Tmax", "opts", "ws", "out", None, "h_n",
                                           "c_n", None), ATTN_WEIGHTS + ATTN_STATE),
    "gic_attn_forward_tf_bwd": ("attn", "bwd", ("dims", "P", "S", "st", "w", "fmap", "pred", "caps", "lengths", "Tmax", "d_pred", None, 1.0, 1, "G",
                                                None), ("S.wcat_t", "S.wout", "S.wh", "P.w_a") + ATTN_STATE + ATTN_BWD_WS + ATTN_GRADS),
    "gic_attn_forward_tf_ws_bytes": ("attn", "ws_bytes", ("dims", "Tmax", "nbytes"), ()),
    "gic_decoder_forward_ss_ws_bytes": ("lstm", "ws_bytes", ("dims", "Tmax", "nbytes"), ()),
    "gic_attn_forward_ss_ws_bytes": ("attn", "ws_bytes", ("dims", "Tmax", "nbytes"), ()),
}

NAN = math.nan
# (case, what the entry point must be for the case to apply, the faults).  Faults: dims=dict (fields replaced), Tmax, null=tuple of
# arguments / struct fields to null, opts=dict (fields of gic_sched_sample_opts), ws = the ss workspace's pointer value, det = the
# deterministic mode
SHAPE_CASES = [
    ("null_dims", (), dict(null=("dims",))),
    ("B0", (), dict(dims=dict(B=0))),
    ("V1", (), dict(dims=dict(V=1))),
    ("NL0", ("lstm",), dict(dims=dict(NL=0))),
    ("NL5", ("lstm",), dict(dims=dict(NL=5))),
    ("dtype7", (), dict(dims=dict(dtype=7))),
    ("V62", ("attn",), dict(dims=dict(V=62))),
    ("E12", ("attn",), dict(dims=dict(E=12))),
    ("P100000", ("attn",), dict(dims=dict(P=100000))),
    ("Tmax0", (), dict(Tmax=0)),
    ("Tmax_L+1", (), dict(Tmax=99)),
    ("B0+dtype7", (), dict(dims=dict(B=0, dtype=7))),
    ("B0+Tmax0", (), dict(dims=dict(B=0), Tmax=0)),
    ("dtype7+Tmax0", (), dict(dims=dict(dtype=7), Tmax=0)),
    ("NL0+dtype7", ("lstm",), dict(dims=dict(NL=0, dtype=7))),
    ("dtype7+V62", ("attn",), dict(dims=dict(dtype=7, V=62))),
    ("E12+P100000", ("attn",), dict(dims=dict(E=12, P=100000))),
]
WS_BYTES_CASES = SHAPE_CASES + [
    ("null_out", (), dict(null=("nbytes",))),
    ("null_dims+null_out", (), dict(null=("dims", "nbytes"))),
    ("Tmax0+null_out", (), dict(Tmax=0, null=("nbytes",))),
]
TWO_FAULTS = [
    ("null_dims+null_P", (), dict(null=("dims", "P"))),
    ("B0+null_P", (), dict(dims=dict(B=0), null=("P",))),
    ("null_S+null_caps", (), dict(null=("S", "caps"))),
    ("null_lengths+Tmax0", (), dict(null=("lengths",), Tmax=0)),
    ("null_caps+Tmax0", (), dict(null=("caps",), Tmax=0)),
    ("L1+null_caps+Tmax2", (), dict(dims=dict(L=1), null=("caps",), Tmax=2)),              # L = 1: no caption column, caps may be null
    ("Tmax0+null_S.wout", (), dict(Tmax=0, null=("S.wout",))),
    ("Tmax_L+1+null_st.hout", (), dict(Tmax=99, null=("st.hout",))),
    ("null_st+null_P.embed", ("fwd",), dict(null=("st", "P.embed"))),
    ("null_P.embed+null_S.wcat[1]", ("lstm", "fwd"), dict(null=("P.embed", "S.wcat[1]"))),
    ("null_st.gpre+null_st.xh[0]", ("lstm", "fwd"), dict(null=("st.gpre", "st.xh[0]"))),
    ("null_S.bsum[0]+null_st.c[1]", ("lstm", "fwd"), dict(null=("S.bsum[0]", "st.c[1]"))),
    ("null_S.wh+null_st.xh", ("attn", "fwd"), dict(null=("S.wh", "st.xh"))),
    ("null_fmap+null_P.b_f", ("attn", "fwd"), dict(null=("fmap", "P.b_f"))),
    ("null_opts+null_caps", ("ss",), dict(null=("opts", "caps"))),
    ("Tmax0+prob_neg", ("ss",), dict(Tmax=0, opts=dict(prob=-0.5))),
    ("prob_nan+pick2", ("ss",), dict(opts=dict(prob=NAN, pick=2))),
    ("pick2+null_inputs", ("ss",), dict(opts=dict(pick=2, inputs=None))),
    ("null_inputs+ws_8", ("ss",), dict(opts=dict(inputs=None), ws=264)),
    ("L1+null_inputs+ws_8", ("ss",), dict(dims=dict(L=1), Tmax=1, opts=dict(inputs=None), ws=264)),      # L = 1: no position to decide
    ("ws_8+null_P.embed", ("ss",), dict(ws=264, null=("P.embed",))),
    ("prob_2+null_st.hout", ("ss",), dict(opts=dict(prob=2.0), null=("st.hout",))),
    ("null_w+null_G", ("bwd",), dict(null=("w", "G"))),
    ("null_w.dhout+null_st.gates[0]", ("lstm", "bwd"), dict(null=("w.dhout", "st.gates[0]"))),
    ("null_G.features+null_w.dc[0]", ("lstm", "bwd"), dict(null=("G.features", "w.dc[0]"))),
    ("null_st.xh[0]+null_G.b_hh[1]", ("lstm", "bwd"), dict(null=("st.xh[0]", "G.b_hh[1]"))),
    ("null_S.wcat_t+null_st.xh", ("attn", "bwd"), dict(null=("S.wcat_t", "st.xh"))),
    ("null_st.hproj+null_w.dz", ("attn", "bwd"), dict(null=("st.hproj", "w.dz"))),
    ("null_w.dx+null_G.embed", ("attn", "bwd"), dict(null=("w.dx", "G.embed"))),
    ("bf16+null_w.dfproj_act", ("attn", "bwd"), dict(dims=dict(dtype=1), null=("w.dfproj_act",))),
    ("bf16+null_w.dfproj_act+null_G.w_a", ("attn", "bwd"), dict(dims=dict(dtype=1), null=("w.dfproj_act", "G.w_a"))),
    # the deterministic mode: gic_attn_forward_ss refuses before it looks at anything, no other teacher-forced entry point refuses
    ("det+null_dims", (), dict(det=1, null=("dims",))),
    ("det+Tmax0", (), dict(det=1, Tmax=0)),
]
SS_CASES = [
    ("prob_neg", ("ss",), dict(opts=dict(prob=-0.5))),
    ("prob_2", ("ss",), dict(opts=dict(prob=2.0))),
    ("prob_nan", ("ss",), dict(opts=dict(prob=NAN))),
    ("pick2", ("ss",), dict(opts=dict(pick=2))),
    ("pick_neg", ("ss",), dict(opts=dict(pick=-1))),
    ("null_inputs", ("ss",), dict(opts=dict(inputs=None))),
    ("ws_8", ("ss",), dict(ws=264)),
    ("ws_4", ("ss",), dict(ws=260)),
]

_STRUCTS = {"lstm": dict(dims="DecoderDims", P="DecoderParams", S="DecoderShadow", st="DecoderState", w="DecoderBwdWs", G="DecoderGrads"),
            "attn": dict(dims="AttnDims", P="AttnParams", S="AttnShadow", st="AttnState", w="AttnBwdWs", G="AttnGrads")}


def _applies(needs, traits):
    return all(n in traits for n in needs)


def _cases(symbol):
    model, kind, args, fields = ENTRIES[symbol]
    if kind == "ws_bytes":
        table = WS_BYTES_CASES
    else:
        table = SHAPE_CASES + [(f"null_{a}", (), dict(null=(a,))) for a in args if isinstance(a, str) and a not in ("dims", "Tmax")] \
            + [(f"null_{f}", (), dict(null=(f,))) for f in fields] + SS_CASES + TWO_FAULTS
    traits = {model, kind} | ({"fwd"} if kind in ("tf", "ss") else set())
    return [(case, faults) for case, needs, faults in table if _applies(needs, traits)]


def _filled(L, model, name, null):
    """The struct ``name`` of the model with every pointer set but the fields that ``null`` names."""
    s = getattr(L, _STRUCTS[model][name])()
    for field, ctype in s._fields_:
        if ctype is C.c_void_p:
            setattr(s, field, None if f"{name}.{field}" in null else PTR)
        else:
            for l in range(L.MAX_LAYERS):
                getattr(s, field)[l] = None if f"{name}.{field}[{l}]" in null else PTR
    return s


def _call(L, lib, symbol, dims=None, Tmax=3, null=(), opts=None, ws=PTR, det=0):
    model, kind, args, fields = ENTRIES[symbol]
    assert all(n in args or n in fields or n == "w.dfproj_act" for n in null), (symbol, null)
    d = getattr(L, _STRUCTS[model]["dims"])(**{**(LSTM_DIMS if model == "lstm" else ATTN_DIMS), **(dims or {})})
    o = L.SchedSampleOpts()
    o.prob, o.pick, o.inputs, o.replaced = 0.25, 0, PTR, PTR
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    nbytes = C.c_uint64(0)
    keep, call = [d, o, nbytes], []
    for a in args:
        if not isinstance(a, str):
            call.append(a)
        elif a == "Tmax":
            call.append(Tmax)
        elif a in null:
            call.append(None)
        elif a in ("dims", "opts", "nbytes"):
            call.append(C.byref({"dims": d, "opts": o, "nbytes": nbytes}[a]))
        elif a in ("P", "S", "st", "w", "G"):
            keep.append(_filled(L, model, a, null))
            call.append(C.byref(keep[-1]))
        else:
            call.append(ws if a == "ws" else PTR)
    was = lib.gic_get_deterministic()
    lib.gic_set_deterministic(det)
    try:
        rc = getattr(lib, symbol)(*call)
        return rc, lib.gic_last_error().decode()
    finally:
        lib.gic_set_deterministic(was)


def _rows():
    """[[row id, status, text], ...] of the whole grid on the library that gan_image_captioning_amd._lib loads."""
    from gan_image_captioning_amd import _lib as L
    lib = L.load()
    return [[f"{symbol}/{case}", *_call(L, lib, symbol, **faults)] for symbol in ENTRIES for case, faults in _cases(symbol)]


def test_the_grid_covers_every_entry_point_and_check():
    """All nine functions, and per entry point every check of its sequence at least once, two-fault rows among them."""
    from gan_image_captioning_amd import _lib as L
    want = json.load(open(GOLDEN))
    assert {r[0].split("/")[0] for r in want} == set(ENTRIES) and set(ENTRIES) <= set(L.EXPORTED_SYMBOLS) and len(ENTRIES) == 9
    for symbol, (model, kind, args, fields) in ENTRIES.items():
        texts = " | ".join(r[2] for r in want if r[0].startswith(symbol + "/"))
        phrases = ["null dims", "bad dims", "bad dtype", "Tmax must be in 1..L"]
        phrases += ["gen_num_layers"] if model == "lstm" else ["multiple of 4", "at most 1024 positions"]
        phrases += ["null out"] if kind == "ws_bytes" else ["null argument", "caps is null"]
        phrases += ["prob must be", "pick must be", "opts->inputs is null", "16-byte aligned"] if kind == "ss" else []
        if kind != "ws_bytes":
            phrases += {("lstm", False): ["null buffer", "null layer 0 buffer", "null layer 1 buffer"],
                        ("lstm", True): ["null buffer", "null layer 1 buffer (the forward call must have been given state->gates)"],
                        ("attn", False): ["null weights", "null state buffer"],
                        ("attn", True): ["null weights", "null state buffer", "null workspace buffer", "null gradient buffer"]}[model, kind == "bwd"]
        for p in phrases:
            assert p in texts, (symbol, p)
        assert sum(1 for r in want if r[0].startswith(symbol + "/") and "+" in r[0]) >= (6 if kind == "ws_bytes" else 12), symbol


def test_every_row_is_refused_as_recorded():
    want = json.load(open(GOLDEN))
    got = _rows()
    assert [r[0] for r in got] == [r[0] for r in want], "the grid and the recorded table list different calls"
    # refused before any launch (a call that got through would launch on fake pointers): with the argument status, or by the
    # deterministic mode (gic_attn_forward_ss alone)
    unsupported = [r[0] for r in want if r[1] == -2]
    assert unsupported == ["gic_attn_forward_ss/det+null_dims", "gic_attn_forward_ss/det+Tmax0"], unsupported
    assert all(r[1] in (-1, -2) for r in want), [r for r in want if r[1] not in (-1, -2)]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} rows differ from the recorded table (got, recorded): {wrong[:5]}"
