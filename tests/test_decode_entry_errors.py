"""Which check of a caption-decode entry point fires, and with which text: a recorded table (no GPU).

Every row of tests/golden/decode_entry_errors.json is one invalid call of one of the ten decode entry points or the four
gic_*_ws_bytes queries of csrc/decode.hip, on fake (non-null, 256-byte aligned) pointers, with the (status, gic_last_error() text)
it returned.  Rows with two faults at once pin the ORDER of an entry point's checks -- among them that the beam searches check the
weights before the options and the samplers the options before the weights -- which the API tests, asserting a phrase of one
message per fault, do not.

The table was recorded from the library of commit 216ebaa ("Score BLEU-1..4 and ROUGE-L on the device; mixed SCST rewards"), the
last one whose fourteen entry points were written out by hand: that commit built in a checkout of its own, `_rows()` of this file
run against its libgicap.so, the result dumped with json.dump(rows, f, indent=0).  It is not regenerated from later code: a library
that disagrees with a row has changed an error text or the order of its checks."""
import ctypes as C
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_entry_errors.json")
PTR = 256                                         # a fake pointer: non-null, aligned, never dereferenced by a call that is refused
LSTM_DIMS = dict(B=4, L=6, V=50, E=8, H=16, NL=2, dtype=0)
ATTN_DIMS = dict(B=2, L=4, V=64, E=8, H=8, C=8, P=4, A=8, dtype=0)
LSTM_WEIGHTS = ("embed", "b_out", "wout", "wcat0", "bsum0", "wcat1", "bsum1")
ATTN_WEIGHTS = ("embed", "b_out", "b_f", "w_a", "wcat", "bsum", "wout", "wf", "wh")
BUFFERS = ("ws", "features", "ids", "scores", "lengths")

# (symbol, model, head, options struct, takes constraints)
ENTRIES = [(f"gic_{m}_{n}", "lstm" if m == "decoder" else "attn", head, opts, cons)
           for m in ("decoder", "attn")
           for n, head, opts, cons in (("beam_search", "beam", "plain", False), ("diverse_beam_search", "beam", "diverse", False),
                                       ("constrained_beam_search", "beam", "diverse", True), ("sample_captions", "sample", "sample", False),
                                       ("constrained_sample_captions", "sample", "sample", True))]
WS_BYTES = [(f"gic_{m}_{h}_ws_bytes", "lstm" if m == "decoder" else "attn", h) for m in ("decoder", "attn") for h in ("beam", "sample")]

NAN, INF = math.nan, math.inf
# (case, what the entry point must have for the case to apply, the faults).  Faults: dims=dict (fields replaced), K, opts=dict
# (fields of the options struct; groups / diversity go to the diverse struct), null=tuple of arguments / weights / buffers to null,
# ws / cws = the pointer values, cons=dict(n, min_length, S, suppress) or None (a null pointer)
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
    ("K0", (), dict(K=0)),
    ("K9", (), dict(K=9)),
    ("K_gt_V", ("beam",), dict(dims=dict(V=4), K=8)),
    ("L1025", (), dict(dims=dict(L=1025))),
    ("rows", (), dict(dims=dict(B=1 << 22), K=8)),
    ("B0+K0", (), dict(dims=dict(B=0), K=0)),
    ("dtype7+K9", (), dict(dims=dict(dtype=7), K=9)),
    ("K0+L1025", (), dict(dims=dict(L=1025), K=0)),
]
WS_BYTES_CASES = SHAPE_CASES + [
    ("null_out", (), dict(null=("out",))),
    ("null_dims+null_out", (), dict(null=("dims", "out"))),
    ("K0+null_out", (), dict(K=0, null=("out",))),
    ("L1025+null_out", (), dict(dims=dict(L=1025), null=("out",))),
]
DECODE_CASES = SHAPE_CASES + [
    ("null_opts", (), dict(null=("opts",))),
    ("eos_neg", (), dict(opts=dict(eos_id=-1))),
    ("eos_V", (), dict(opts=dict(eos_id=64))),
    ("pad_neg", (), dict(opts=dict(pad_id=-1))),
    ("pad_V", (), dict(opts=dict(pad_id=64))),
    ("lp_nan", ("beam",), dict(opts=dict(length_penalty=NAN))),
    ("groups0", ("diverse",), dict(opts=dict(groups=0))),
    ("groups3", ("diverse",), dict(opts=dict(groups=3))),
    ("div_neg", ("diverse",), dict(opts=dict(diversity=-1.0))),
    ("div_inf", ("diverse",), dict(opts=dict(diversity=INF))),
    ("div_nan", ("diverse",), dict(opts=dict(diversity=NAN))),
    ("topk_neg", ("sample",), dict(opts=dict(top_k=-1))),
    ("topk_gt_V", ("sample",), dict(opts=dict(top_k=65))),
    ("topp_0", ("sample",), dict(opts=dict(top_p=0.0))),
    ("topp_gt_1", ("sample",), dict(opts=dict(top_p=1.5))),
    ("topp_nan", ("sample",), dict(opts=dict(top_p=NAN))),
    ("temp_0", ("sample",), dict(opts=dict(temperature=0.0))),
    ("temp_inf", ("sample",), dict(opts=dict(temperature=INF))),
    ("temp_nan", ("sample",), dict(opts=dict(temperature=NAN))),
    ("null_params", (), dict(null=("params",))),
    ("null_shadow", (), dict(null=("shadow",))),
] + [(f"null_{w}", ("lstm",), dict(null=(w,))) for w in LSTM_WEIGHTS] \
  + [(f"null_{w}", ("attn",), dict(null=(w,))) for w in ATTN_WEIGHTS] \
  + [(f"null_{b}", (), dict(null=(b,))) for b in BUFFERS] + [
    ("null_fmap", ("attn",), dict(null=("fmap",))),
    ("ws_260", (), dict(ws=260)),
    ("ws_8", (), dict(ws=8)),
    ("null_cons", ("cons",), dict(cons=None)),
    ("n_neg", ("cons",), dict(cons=dict(n=-1))),
    ("n_gt_L", ("cons",), dict(cons=dict(n=99))),
    ("min_neg", ("cons",), dict(cons=dict(min_length=-2))),
    ("min_gt_L", ("cons",), dict(cons=dict(min_length=99))),
    ("S_neg", ("cons",), dict(cons=dict(S=-1))),
    ("S_17", ("cons",), dict(cons=dict(S=17))),
    ("sup_neg", ("cons",), dict(cons=dict(suppress=(1, -3)))),
    ("sup_V", ("cons",), dict(cons=dict(suppress=(64,)))),
    ("sup_eos", ("cons",), dict(cons=dict(suppress=(1, 3, 2)))),
    ("infeasible", ("cons",), dict(dims=dict(V=4), cons=dict(n=1, suppress=(1, 3)))),
    ("null_cws", ("cons",), dict(cws=None)),
    ("cws_260", ("cons",), dict(cws=260)),
    # ---- two faults: the first check in the entry point's order answers
    ("null_opts+null_dims", (), dict(null=("opts", "dims"))),
    ("null_opts+null_params", (), dict(null=("opts", "params"))),
    ("null_dims+null_params", (), dict(null=("dims", "params"))),
    ("B0+null_params", (), dict(dims=dict(B=0), null=("params",))),
    ("K0+null_embed", (), dict(K=0, null=("embed",))),
    ("K9+eos_neg", (), dict(K=9, opts=dict(eos_id=-1))),
    ("null_embed+eos_neg", (), dict(null=("embed",), opts=dict(eos_id=-1))),          # weights first (beam) / options first (sampler)
    ("null_params+pad_V", (), dict(null=("params",), opts=dict(pad_id=64))),
    ("null_ids+eos_V", (), dict(null=("ids",), opts=dict(eos_id=64))),
    ("null_wout+lp_nan", ("beam",), dict(null=("wout",), opts=dict(length_penalty=NAN))),
    ("null_shadow+groups0", ("diverse",), dict(null=("shadow",), opts=dict(groups=0))),
    ("null_lengths+temp_0", ("sample",), dict(null=("lengths",), opts=dict(temperature=0.0))),
    ("null_wout+topk_neg", ("sample",), dict(null=("wout",), opts=dict(top_k=-1))),
    ("null_params+null_embed", (), dict(null=("params", "embed"))),
    ("null_features+null_wout", (), dict(null=("features", "wout"))),
    ("null_embed+null_wcat1", ("lstm",), dict(null=("embed", "wcat1"))),
    ("null_fmap+null_wf", ("attn",), dict(null=("fmap", "wf"))),
    ("null_fmap+eos_neg", ("attn",), dict(null=("fmap",), opts=dict(eos_id=-1))),
    ("eos_neg+pad_neg", (), dict(opts=dict(eos_id=-1, pad_id=-1))),
    ("pad_V+lp_nan", ("beam",), dict(opts=dict(pad_id=64, length_penalty=NAN))),
    ("eos_V+groups3", ("diverse",), dict(opts=dict(eos_id=64, groups=3))),
    ("lp_nan+groups0", ("diverse",), dict(opts=dict(length_penalty=NAN, groups=0))),
    ("groups3+div_neg", ("diverse",), dict(opts=dict(groups=3, diversity=-1.0))),
    ("topk_neg+temp_nan", ("sample",), dict(opts=dict(top_k=-1, temperature=NAN))),
    ("topp_0+eos_neg", ("sample",), dict(opts=dict(top_p=0.0, eos_id=-1))),
    ("temp_0+pad_V", ("sample",), dict(opts=dict(temperature=0.0, pad_id=64))),
    ("null_embed+ws_260", (), dict(null=("embed",), ws=260)),
    ("null_ws+null_cons", ("cons",), dict(null=("ws",), cons=None)),
    ("eos_neg+ws_260", (), dict(opts=dict(eos_id=-1), ws=260)),
    ("div_neg+ws_260", ("diverse",), dict(opts=dict(diversity=-1.0), ws=260)),
    ("temp_0+ws_260", ("sample",), dict(opts=dict(temperature=0.0), ws=260)),
    ("null_embed+null_cons", ("cons",), dict(null=("embed",), cons=None)),
    ("eos_neg+null_cons", ("cons",), dict(opts=dict(eos_id=-1), cons=None)),
    ("groups0+n_neg", ("cons", "diverse"), dict(opts=dict(groups=0), cons=dict(n=-1))),
    ("topk_neg+n_neg", ("cons", "sample"), dict(opts=dict(top_k=-1), cons=dict(n=-1))),
    ("null_cons+ws_260", ("cons",), dict(cons=None, ws=260)),
    ("n_neg+ws_260", ("cons",), dict(cons=dict(n=-1), ws=260)),
    ("n_neg+min_neg", ("cons",), dict(cons=dict(n=-1, min_length=-2))),
    ("min_gt_L+S_17", ("cons",), dict(cons=dict(min_length=99, S=17))),
    ("sup_V+sup_eos", ("cons",), dict(cons=dict(suppress=(64, 2)))),
    ("sup_eos+sup_V", ("cons",), dict(cons=dict(suppress=(2, 64)))),
    ("infeasible+ws_260", ("cons",), dict(dims=dict(V=4), cons=dict(n=1, suppress=(1, 3)), ws=260)),
    ("infeasible+null_cws", ("cons",), dict(dims=dict(V=4), cons=dict(n=1, suppress=(1, 3)), cws=None)),
    ("ws_260+null_cws", ("cons",), dict(ws=260, cws=None)),
    ("ws_260+cws_260", ("cons",), dict(ws=260, cws=260)),
    ("cons_off+ws_260", ("cons",), dict(cons=dict(n=0), ws=260)),          # every constraint off: the alignment check still comes first
    ("cons_off+ws_260+null_cws", ("cons",), dict(cons=dict(n=0), ws=260, cws=None)),
    ("cons_off+null_ws", ("cons",), dict(cons=dict(n=0), null=("ws",), cws=None)),
    ("cons_off+S_17", ("cons",), dict(cons=dict(n=0, S=17), cws=None)),
]


def _applies(needs, traits):
    return all(n in traits for n in needs)


def _model(L, model, dims, null):
    """(dims, params, shadow) of a model with every pointer set but those named in ``null``."""
    if model == "lstm":
        d = L.DecoderDims(**{**LSTM_DIMS, **dims})
        p, s = L.DecoderParams(), L.DecoderShadow()
        p.embed, p.w_out, p.b_out, s.wout = (None if "embed" in null else PTR), PTR, (None if "b_out" in null else PTR), \
            (None if "wout" in null else PTR)
        for l in range(L.MAX_LAYERS):
            s.wcat[l] = None if f"wcat{l}" in null else PTR
            s.bsum[l] = None if f"bsum{l}" in null else PTR
    else:
        d = L.AttnDims(**{**ATTN_DIMS, **dims})
        p, s = L.AttnParams(), L.AttnShadow()
        for n in ("embed", "w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out", "w_f", "b_f", "w_h", "w_a"):
            setattr(p, n, None if n in null else PTR)
        for n in ("wcat", "bsum", "wout", "wcat_t", "wf", "wh"):
            setattr(s, n, None if n in null else PTR)
    ref = lambda x, name: None if name in null else C.byref(x)
    return (d, p, s), (ref(d, "dims"), ref(p, "params"), ref(s, "shadow"))


def _constraints(L, n=2, min_length=0, S=None, suppress=()):
    c = L.DecodeConstraints()
    c.no_repeat_ngram, c.min_length = n, min_length
    c.num_suppress = len(suppress) if S is None else S
    for i, v in enumerate(suppress):
        c.suppress[i] = v
    return c


_DEFAULT_CONS = dict()


def _decode_call(L, lib, entry, dims=None, K=4, opts=None, null=(), ws=PTR, cws=PTR, cons=_DEFAULT_CONS):
    symbol, model, head, kind, takes_cons = entry
    opts = dict(opts or {})
    keep, (dp, pp, sp) = _model(L, model, dims or {}, null)
    if kind == "sample":
        o = L.SampleOpts()
        o.num_samples, o.top_k, o.top_p, o.temperature, o.eos_id, o.pad_id = K, 0, 1.0, 1.0, 2, 0
        plain = o
    else:
        o = L.DiverseBeamOpts() if kind == "diverse" else L.DecoderBeamOpts()
        plain = o.beam if kind == "diverse" else o
        plain.beam, plain.eos_id, plain.pad_id, plain.length_penalty = K, 2, 0, 0.0
        if kind == "diverse":
            o.groups, o.diversity = 2, 0.5
    for k, v in opts.items():
        setattr(o if k in ("groups", "diversity") else plain, k, v)
    buf = {b: (None if b in null else PTR) for b in BUFFERS + ("fmap",)}
    buf["ws"] = None if "ws" in null else ws
    args = [dp, pp, sp, None if "opts" in null else C.byref(o)]
    if takes_cons:
        c = None if cons is None else _constraints(L, **cons)
        args += [None if c is None else C.byref(c), buf["ws"], cws]
    else:
        args += [buf["ws"]]
    args += [buf["features"]] + ([buf["fmap"]] if model == "attn" else [])
    if head == "sample":
        args += [None, 0]                         # noise_u, seed
    args += [buf["ids"], buf["scores"], buf["lengths"]]
    if head == "beam" and model == "attn":
        args += [None]                            # alphas
    args += [None]                                # stream
    rc = getattr(lib, symbol)(*args)
    return rc, lib.gic_last_error().decode()


def _ws_bytes_call(L, lib, entry, dims=None, K=4, null=()):
    symbol, model, head = entry
    keep, (dp, _, _) = _model(L, model, dims or {}, null)
    out = C.c_uint64(0)
    rc = getattr(lib, symbol)(dp, K, None if "out" in null else C.byref(out))
    return rc, lib.gic_last_error().decode()


def _rows():
    """[[row id, status, text], ...] of the whole grid on the library that gan_image_captioning_amd._lib loads."""
    from gan_image_captioning_amd import _lib as L
    lib = L.load()
    rows = []
    for entry in WS_BYTES:
        traits = {entry[1], entry[2]}
        for case, needs, faults in WS_BYTES_CASES:
            if _applies(needs, traits):
                rows.append([f"{entry[0]}/{case}", *_ws_bytes_call(L, lib, entry, **faults)])
    for entry in ENTRIES:
        symbol, model, head, kind, takes_cons = entry
        traits = {model, head} | ({"diverse"} if kind == "diverse" else set()) | ({"cons"} if takes_cons else set())
        for case, needs, faults in DECODE_CASES:
            if _applies(needs, traits):
                rows.append([f"{symbol}/{case}", *_decode_call(L, lib, entry, **faults)])
    return rows


def test_the_grid_covers_every_entry_point_and_check():
    """All fourteen functions, and per decode entry point every check of its sequence at least once, two-fault rows among them."""
    from gan_image_captioning_amd import _lib as L
    want = json.load(open(GOLDEN))
    names = {r[0].split("/")[0] for r in want}
    assert names == {e[0] for e in ENTRIES} | {e[0] for e in WS_BYTES} and names <= set(L.EXPORTED_SYMBOLS)
    assert len(ENTRIES) == 10 and len(WS_BYTES) == 4
    for symbol, model, head, kind, takes_cons in ENTRIES:
        texts = " | ".join(r[2] for r in want if r[0].startswith(symbol + "/"))
        phrases = ["null options", "null dims", "bad dims", "bad dtype", "must be 1..8", "at most 1024 steps", "too many rows", "eos_id", "pad_id",
                   "null argument", "256-byte aligned"]
        phrases += ["exceeds the vocabulary", "length_penalty is NaN"] if head == "beam" else ["top_k", "top_p", "temperature"]
        phrases += ["groups must be", "diversity must be"] if kind == "diverse" else []
        phrases += ["null embedding", "null layer 1 weights", "gen_num_layers"] if model == "lstm" else ["null weights", "multiple of 4"]
        phrases += ["null constraints", "no_repeat_ngram must", "min_length must", "num_suppress must", "suppress[0] = 64 outside", "is eos_id", "infeasible",
                    "constraint workspace"] if takes_cons else []
        for p in phrases:
            assert p in texts, (symbol, p)
        assert sum(1 for r in want if r[0].startswith(symbol + "/") and "+" in r[0]) >= 15, symbol


def test_every_row_is_refused_as_recorded():
    want = json.load(open(GOLDEN))
    got = _rows()
    assert [r[0] for r in got] == [r[0] for r in want], "the grid and the recorded table list different calls"
    # refused with the argument status, that is before any launch (a call that got through would launch on fake pointers)
    assert all(r[1] == -1 for r in want), [r for r in want if r[1] != -1]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} rows differ from the recorded table (got, recorded): {wrong[:5]}"
