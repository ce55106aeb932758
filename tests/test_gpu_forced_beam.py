"""Lexically constrained beam search on the GPU (gic_*_forced_beam_search; the engines', decoders' and Generator's force_words;
GANInstructor.evaluate_forced) against the float64 oracle (tests/forced_beam_oracle.py) on the cases that
tests/test_forced_beam_api.py pins, the invariants of every returned caption, teacher-forced rescoring, and itself."""
import math

import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import forced_beam_oracle as FO
from tests import test_constrained_api as T
from tests import test_forced_beam_api as F
from tests.test_gpu_attn_beam import _check_alphas
from tests.test_gpu_constrained import _ATTN, _gen_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _eng(which, dt=0):
    from gan_image_captioning_amd import engine
    if which == "attn":
        return engine.AttnDecoderEngine(*T.ATTN_SHAPE[2:], dt)
    B, L, V, E, H, NL = F.FUSED200 if which == "fused200" else T.LSTM_SHAPES[which]
    return engine.DecoderEngine(V, E, H, NL, dt)


def _gpu_forced(case, dev):
    """(ids, scores, lengths[, alphas], met) of the engine for one of F.CASES."""
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    B, L, V = F.shape_of(which)
    eng = _eng(which)
    force = F.case_force(case).to(dev)
    if which == "attn":
        params, feats, fmap = F.case_problem(case)
        return eng.beam_search([p.to(dev) for p in params], feats.to(dev), fmap.to(dev), L, K, 2, pad, alpha, want_alphas=True,
                               force_words=force, **cons)
    params, feats = F.case_problem(case)
    assert eng.beam_fused(B, K) == (which != "generic")
    return eng.beam_search([p.to(dev) for p in params], feats.to(dev), L, K, 2, pad, alpha, force_words=force, **cons)


# ---------------------------------------------------------------- 1. f32 against the oracle, every case, all three recurrences
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_f32_matches_oracle(dev, case):
    """On the images whose every selection the oracle decides by >= 1e-4: the same beams with the same lengths and masks, in the
    same order where the final order is decided by >= 1e-4 too (else as sets per count of real constraints met; dead beams always
    come last, in place), scores within rtol 1e-4 / atol 1e-5."""
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    B, L, V = F.shape_of(which)
    got = _gpu_forced(case, dev)
    torch.cuda.synchronize()
    want = F.case_oracle(case)
    ids, sc, ln, met = got[0].cpu(), got[1].cpu().double(), got[2].cpu().long(), got[-1].cpu().long()
    rid, rsc, rln, rmet, margins = want[:5]
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    print(f"{F.case_id(case)}: {len(ok)} of {B} images compared; margins {margins}")
    assert 4 * len(ok) >= 3 * B
    sets = F.case_force(case).tolist()
    for b in ok:
        init = FO.absent_mask(sets[b])
        live = rln[b] > 0
        assert torch.equal(ln[b] > 0, live), b                  # dead beams: the same slots (they sort last, by beam index)
        assert (sc[b][~live] == -math.inf).all() and (ids[b][~live] == pad).all() and (met[b][~live] == init).all(), b
        if margins[b][1] >= 1e-4:
            assert torch.equal(ids[b], rid[b]) and torch.equal(ln[b], rln[b]) and torch.equal(met[b], rmet[b]), b
            torch.testing.assert_close(sc[b][live], rsc[b][live], rtol=1e-4, atol=1e-5)
        else:
            real = lambda m: [bin(int(v) & ~init).count("1") for v in m]     # noqa: E731
            assert real(met[b]) == real(rmet[b]), b            # (the count of real constraints met orders before the scores)
            for n in set(real(met[b][live])):
                s = live & (torch.tensor(real(rmet[b])) == n)
                key = lambda i, l, m: sorted(zip(i[s].tolist(), l[s].tolist(), m[s].tolist()))     # noqa: E731
                assert key(ids[b], ln[b], met[b]) == key(rid[b], rln[b], rmet[b]), (b, n)
                torch.testing.assert_close(sc[b][s].sort().values, rsc[b][s].sort().values, rtol=1e-4, atol=1e-5)
        if which == "attn":
            for j in range(K):
                r = next(i for i in range(K) if torch.equal(rid[b, i], ids[b, j]) and rln[b, i] == ln[b, j])
                torch.testing.assert_close(got[3][b, j].cpu().double(), want[5][b, r], rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------- 2. invariants of every returned caption, and its score
def _lstm_decoder(dev, shape, dtype, seed=11):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Decoder
    B, L, V, E, H, NL = shape
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, gen_num_layers=NL, compute_dtype=dtype, max_seq_len=L,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(seed)
    dec = Decoder(args).to(dev)
    with torch.no_grad():
        dec.linear.weight.mul_(8.0)
        dec.linear.bias[2] += 1.0
    return dec


def _attn_decoder(dev, dtype, seed=12):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import AttnDecoder
    B, L, V, E, H, Cc, P, A = T.ATTN_SHAPE
    args = default_args(vocab_size=V, gen_embed_dim=E, gen_hidden_dim=H, attn_dim=A, decoder="attention", compute_dtype=dtype, max_seq_len=L,
                        device="cuda", log_file=None, model_dir=None, save_dir=None)
    torch.manual_seed(seed)
    dec = AttnDecoder(args, Cc, P).to(dev)
    with torch.no_grad():
        dec.linear.weight.mul_(8.0)
        dec.linear.bias[2] += 1.0
    return dec


def _force_for(B, V, Cn, D, seed):
    """Sets over ids 4 .. V - 1 (no special, none that C_ALL suppresses): image b carries C constraints, b % 4 == 1 one, b % 4 == 2
    none; the first id of image 0 is V - 1, and with C >= 2 image 3's second set shares an id with its first."""
    g = torch.Generator().manual_seed(seed)
    f = torch.full((B, Cn, D), -1, dtype=torch.int32)
    for b in range(B):
        n = 1 if b % 4 == 1 else 0 if b % 4 == 2 else Cn
        perm = (torch.randperm(V - 4, generator=g)[:n * D] + 4).to(torch.int32).reshape(n, D)
        f[b, :n] = perm
        for c in range(n):
            f[b, c, 1 + (b + c) % D:] = -1
    f[0, 0, 0] = V - 1 if not bool((f[0] == V - 1).any()) else f[0, 0, 0]
    if Cn >= 2 and B > 3:
        f[3, 1, 0] = f[3, 0, 0]
    return f


def _check_outputs(ids, scores, lengths, met, force, K, Cn, alpha, cons, pad=0):
    """met is the mask recomputed from the ids; the decode constraints hold on every live caption; the slots follow the stated key;
    dead beams come last as all-pad ids of length 0 and score -inf."""
    ids, scores, lengths, met = ids.cpu(), scores.cpu().double(), lengths.cpu().long(), met.cpu().long()
    sets = force.tolist()
    B, L = ids.shape[0], ids.shape[2]
    for b in range(B):
        init = FO.absent_mask(sets[b])
        live = lengths[b] > 0
        n_live = int(live.sum())
        assert n_live >= 1 and bool(live[:n_live].all()), (b, lengths[b])
        assert (scores[b][~live] == -math.inf).all() and (ids[b][~live] == pad).all()
        for j in range(K):
            assert int(met[b, j]) == FO.met_mask(ids[b, j].tolist(), int(lengths[b, j]), sets[b]), (b, j)
        assert int(met[b, 0]) == (1 << Cn) - 1, (b, met[b])
        real = [bin(int(m) & ~init).count("1") for m in met[b][:n_live]]
        norm = (scores[b][:n_live] / lengths[b][:n_live].double() ** alpha).tolist()
        for j in range(n_live - 1):
            assert real[j] > real[j + 1] or (real[j] == real[j + 1] and norm[j] >= norm[j + 1] - 1e-6 * abs(norm[j + 1])), (b, j, real, norm)
        T.check_invariants(ids[b][live], lengths[b][live], L, cons["no_repeat_ngram"], cons["min_length"], cons["suppress_tokens"], pad_id=pad)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["generic", "fused", "fused200"])
def test_lstm_invariants_and_scores(dev, which, dtype):
    shape = F.FUSED200 if which == "fused200" else T.LSTM_SHAPES[which]
    B, L, V, E, H, NL = shape
    dec = _lstm_decoder(dev, shape, dtype)
    feats = torch.randn(B, E, device=dev)
    tol = 1e-4 if dtype == "fp32" else 1e-2
    for Cn, K, D, alpha, cons in ((1, 2, 4, 0.0, F.C_OFF), (2, 8, 4, 0.7, T.C_ALL), (3, 8, 1, 0.0, T.C_ALL)):
        assert dec.engine().beam_fused(B, K) == (which != "generic")
        force = _force_for(B, V, Cn, D, seed=Cn)
        ids, scores, lengths, met = dec.beam_search(feats, beam_size=K, return_beams=True, length_penalty=alpha, force_words=force.to(dev),
                                                    return_met=True, **cons)
        torch.cuda.synchronize()
        _check_outputs(ids, scores, lengths, met, force, K, Cn, alpha, cons)
        for j in range(K):                                       # every live caption's score is the log-likelihood of its ids
            live = lengths[:, j] > 0
            if bool(live.any()):
                logp, _ = dec.log_likelihood(feats[live], ids[live, j], lengths[live, j])
                torch.testing.assert_close(logp, scores[live, j], rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attn_invariants_and_scores(dev, dtype):
    B, L, V, E, H, Cc, P, A = T.ATTN_SHAPE
    dec = _attn_decoder(dev, dtype)
    feats, fmap = torch.randn(B, E, device=dev), torch.randn(B, P, Cc, device=dev)
    for Cn, K, D, alpha, cons in ((1, 2, 4, 0.0, F.C_OFF), (2, 8, 4, 0.7, T.C_ALL), (3, 8, 1, 0.0, T.C_ALL)):
        force = _force_for(B, V, Cn, D, seed=Cn)
        ids, scores, lengths, alphas, met = dec.beam_search(feats, fmap, beam_size=K, return_beams=True, return_alphas=True, length_penalty=alpha,
                                                            force_words=force.to(dev), return_met=True, **cons)
        torch.cuda.synchronize()
        _check_outputs(ids, scores, lengths, met, force, K, Cn, alpha, cons)
        _check_alphas(alphas, lengths)
        for j in range(K):
            live = lengths[:, j] > 0
            if bool(live.any()):
                logp, _ = dec.log_likelihood(feats[live], fmap[live], ids[live, j], lengths[live, j])
                ref, got, n = logp.double(), scores[live, j].double(), lengths[live, j].double()
                tol = (1e-4 * ref.abs() + 1e-4) if dtype == "fp32" else (2e-2 * ref.abs() + 0.05 * n)
                assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()


# ---------------------------------------------------------------- 3. the same bits twice, and in the deterministic mode
def test_bits_and_deterministic_mode(dev):
    from gan_image_captioning_amd import engine
    cases = [F.CASES[4], F.CASES[8], F.CASES[14], F.CASES[19]]           # generic, fused, attn, fused200

    def all_cases():
        return [_gpu_forced(c, dev) for c in cases]

    runs = [all_cases(), all_cases()]
    was = engine.deterministic()
    engine.set_deterministic(True)
    try:
        runs.append(all_cases())
    finally:
        engine.set_deterministic(was)
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            for a, b in zip(x, y):
                assert torch.equal(a, b)


def test_keyword_at_its_default_runs_the_plain_search(dev, monkeypatch):
    """force_words=None: the calls the engine made before, the same bits, and no forced entry point."""
    from gan_image_captioning_amd import _lib as L
    case = F.CASES[7]
    params, feats = F.case_problem(case)
    B, Lc, V = F.shape_of(case[0])
    eng = _eng(case[0])
    p, f = [t.to(dev) for t in params], feats.to(dev)
    want = eng.beam_search(p, f, Lc, 4, **T.C_ALL)
    lib = L.load()
    for name in ("gic_decoder_forced_beam_search", "gic_decoder_forced_beam_ws_bytes"):
        monkeypatch.setattr(lib, name, lambda *a: pytest.fail("a forced entry point ran"))
    got = eng.beam_search(p, f, Lc, 4, force_words=None, **T.C_ALL)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. through the public interface
@pytest.mark.parametrize("kind", ["lstm", "lstm_uncond", "attention"])
def test_generator_caption(dev, kind):
    from gan_image_captioning_amd.generator import Generator
    kw = {"lstm": {}, "lstm_uncond": dict(conditional_gan=0), "attention": _ATTN}[kind]
    torch.manual_seed(4)
    gen = Generator(_gen_args(**kw)).to(dev)
    gen.eval()
    images = torch.randn(4, 3, 64, 64, device=dev)
    words = [[(40, 41), 50], [63], [], [(7, 8), (8, 9)]]
    force = torch.tensor([[[40, 41], [50, -1]], [[63, -1], [-1, -1]], [[-1, -1], [-1, -1]], [[7, 8], [8, 9]]], dtype=torch.int32)
    plain = gen.caption(images, beam_size=4, return_beams=True)
    beams = gen.caption(images, beam_size=4, return_beams=True, force_words=words, return_met=True)
    same = gen.caption(images, beam_size=4, return_beams=True, force_words=force.to(dev), return_met=True)
    best = gen.caption(images, beam_size=4, force_words=words, return_met=True)
    quiet = gen.caption(images, beam_size=4, force_words=words)
    held = gen.caption(images, beam_size=4, return_beams=True, force_words=words, return_met=True, **T.C_UNI)
    torch.cuda.synchronize()
    assert [t.shape for t in beams] == [(4, 4, 8), (4, 4), (4, 4), (4, 4)] and beams[3].dtype == torch.int32
    for a, b in zip(beams, same):
        assert torch.equal(a, b)
    assert len(quiet) == 3 and len(best) == 4
    for a, b in zip(best, beams):
        assert torch.equal(a, b[:, 0])
    for a, b in zip(quiet, best):
        assert torch.equal(a, b)
    _check_outputs(*beams, force, 4, 2, 0.0, F.C_OFF)
    _check_outputs(*held, force, 4, 2, 0.0, T.C_UNI)
    # image 2 carries nothing: its last state group is plain beam search of its width (one beam), the other slots are dead
    assert torch.equal(beams[0][2, 0], gen.caption(images, beam_size=1)[0][2]) and int((beams[2][2] > 0).sum()) == 1
    assert not torch.equal(plain[0][:, 0], beams[0][:, 0])
    if kind == "attention":
        al = gen.caption(images, beam_size=4, return_beams=True, return_alphas=True, force_words=words, return_met=True)
        assert len(al) == 5 and torch.equal(al[0], beams[0]) and torch.equal(al[4], beams[3]) and al[3].shape == (4, 4, 8, al[3].shape[-1])
        _check_alphas(al[3], al[2])
        feats, fmap = gen._features(images)
        with torch.no_grad():
            tf = gen.decoder(feats, fmap, al[0][:, 0, :-1].contiguous(), al[2][:, 0].cpu(), pretrain=True, return_alphas=True)
        n = tf[2].shape[1]
        pos = torch.arange(n, device=dev)[None, :, None] < al[2][:, 0, None, None]
        torch.testing.assert_close(al[3][:, 0, :n], torch.where(pos, tf[2].float(), torch.zeros_like(tf[2].float())), rtol=1e-4, atol=1e-6)
    with pytest.raises(ValueError, match="beam_groups > 1"):
        gen.caption(images, beam_size=4, beam_groups=2, force_words=words)
    with pytest.raises(ValueError, match=r"2\^C = 4 must divide the beam size 6"):
        gen.caption(images, beam_size=6, force_words=words)
    with pytest.raises(ValueError, match="<E>"):
        gen.caption(images, beam_size=4, force_words=[[2], [], [], []])
    with pytest.raises(ValueError, match="suppressed id"):
        gen.caption(images, beam_size=4, force_words=words, suppress_tokens=(63,))


# ---------------------------------------------------------------- 5. the oracle-tags evaluation
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_evaluate_forced(dev, kind):
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    kw = _ATTN if kind == "attention" else {}
    args = _gen_args(eval_force_words=2, eval_force_beam_size=8, eval_min_length=3, **kw)
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    assert inst.eval_forced == (2, 8)
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    out = inst.evaluate_forced("val", *inst.eval_forced)
    assert set(out) == {"bleu4", "cider_d", "satisfied", "satisfied_plain"}
    assert all(math.isfinite(v) for v in out.values()) and 0.0 <= out["bleu4"] <= 1.0 and out["cider_d"] >= 0.0
    assert out["satisfied"] == 1.0 and out["satisfied_plain"] < 1.0, out
    assert {"BLEU4F_val", "CIDErDF_val", "ForcedSat_val", "PlainSat_val"} <= {t for t, _ in seen}
    assert out == inst.evaluate_forced("val", 2, 8)


# ---------------------------------------------------------------- 6. what the Python layer normally keeps out, and its cost
def test_a_suppressed_id_in_a_set_proposes_nothing(dev, monkeypatch):
    """The library cannot read the ids, so a C caller may put a suppressed id into a set.  The id is on every row's ban list, its hop
    value is -inf, and the hop slot proposes nothing: no caption holds the id, the states that need it stay dead, and every live
    caption's mask is still the one recomputed from its ids."""
    from gan_image_captioning_amd import engine
    case = F.CASES[7]                                           # fused, C = 2, K = 4, C_ALL (suppresses 1 and 3)
    which, seed, Cn, K, D, cons, alpha, pad, special = case
    B, L, V = F.shape_of(which)
    force = F.case_force(case)
    force[0, 0, 0], force[3, 1, 0] = 3, 1                       # image 0: its first set is the suppressed id alone; image 3: its second
    monkeypatch.setattr(engine, "check_force_words", lambda *a, **k: None)
    params, feats = F.case_problem(case)
    ids, scores, lengths, met = _eng(which).beam_search([p.to(dev) for p in params], feats.to(dev), L, K, 2, pad, alpha,
                                                        force_words=force.to(dev), **cons)
    torch.cuda.synchronize()
    ids, scores, lengths, met = ids.cpu(), scores.cpu(), lengths.cpu().long(), met.cpu().long()
    sets = force.tolist()
    for b in range(B):
        live = lengths[b] > 0
        assert bool(live.any()) and (scores[b][~live] == -math.inf).all() and (ids[b][~live] == pad).all()
        assert bool(torch.isfinite(scores[b][live]).all())
        for j in range(K):
            assert int(met[b, j]) == FO.met_mask(ids[b, j].tolist(), int(lengths[b, j]), sets[b]), (b, j)
            assert not {1, 3} & set(ids[b, j, :int(lengths[b, j])].tolist())
    assert not bool((met[0][lengths[0] > 0] & 1).any()) and not bool((met[3][lengths[3] > 0] & 2).any())
    assert bool((met[0][lengths[0] > 0] == 2).any())           # the set that can be met still is


def test_a_reused_device_tensor_is_read_once(dev, monkeypatch):
    """check_force_words copies a device tensor to the host once; the same tensor, unmodified, is not read again, and a modified one is."""
    from gan_image_captioning_amd import engine
    calls = []
    real = engine._check_force_words_host
    monkeypatch.setattr(engine, "_check_force_words_host", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(engine, "_FORCE_CHECKED", [None])
    case = F.CASES[6]
    params, feats = F.case_problem(case)
    B, L, V = F.shape_of(case[0])
    p, f, eng = [t.to(dev) for t in params], feats.to(dev), _eng(case[0])
    force = F.case_force(case).to(dev)
    outs = [eng.beam_search(p, f, L, case[3], force_words=force) for _ in range(3)]
    assert len(calls) == 1
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b)
    eng.beam_search(p, f, L, case[3], force_words=force, suppress_tokens=(1,))      # other arguments: checked again
    assert len(calls) == 2
    force[0, 0, 0] = 2                                                                 # modified in place: read again, and refused
    with pytest.raises(ValueError, match="<E>"):
        eng.beam_search(p, f, L, case[3], force_words=force)
    assert len(calls) == 3
