"""Pairwise CIDEr-D on the GPU (gic_cider_pairwise): the matrix, the row consensus and the Self-CIDEr against the float64 oracle
(tests/cider_pair_oracle.py), agreement with gic_cider_d, the optional outputs, bit-reproducibility, consensus re-ranking through
Generator.caption / sample_captions for both decoders, and GANInstructor.evaluate_consensus.

Tolerances: matrix and consensus rtol = atol = 1e-5 (the CIDEr-D tolerance of tests/test_gpu_cider.py); self_cider atol =
TOL_SELF_CIDER (4 x the measured error of the float32 restatement of the kernel's lambda_max iteration; tests/test_cider_pair_api.py)."""
import math

import numpy as np
import pytest
import torch

from tests import cider_oracle as CO
from tests import cider_pair_oracle as PO
from tests import test_cider_pair_api as A
from tests import test_constrained_api as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _scorer(corpus, V, dev):
    from gan_image_captioning_amd.cider import CiderD
    return CiderD(corpus, V, dev)


def _on_device(case, dev):
    prob, ref = PO.case_problem(case)
    ids, lengths = torch.from_numpy(prob["ids"]).to(dev), torch.from_numpy(prob["lengths"]).to(dev)
    return prob, ref, _scorer(prob["corpus"], prob["V"], dev), ids, lengths


# ------------------------------------------------------------------------------------------------ 1. the kernel against the oracle
@pytest.mark.parametrize("case", PO.CASES, ids=lambda c: "V%d-B%d-K%d-L%d" % c)
def test_matrix_consensus_and_self_cider_match_the_oracle(dev, case):
    V, B, K, Lmax = case
    prob, (M, cons, sc), scorer, ids, lengths = _on_device(case, dev)
    out = scorer.pairwise(ids, lengths)
    torch.cuda.synchronize()
    got_m, got_c, got_s = out["matrix"].cpu().double().numpy(), out["consensus"].cpu().double().numpy(), out["self_cider"].cpu().double().numpy()
    assert got_m.shape == (B, K, K) and got_c.shape == (B, K) and got_s.shape == (B,)
    err_m, err_c, err_s = np.abs(got_m - M).max(), np.abs(got_c - cons).max(), np.abs(got_s - sc).max()
    print(f"[cider_pair] {case}: max |err| matrix {err_m:.3e} consensus {err_c:.3e} self_cider {err_s:.3e} (tol {PO.TOL_SELF_CIDER:.3e}); "
          f"self_cider {np.round(sc, 4).tolist()}")
    if K > 1:
        off = M - np.stack([np.diag(np.diag(m)) for m in M])
        assert off.max() > 1.0, "no real match in the problem"
    np.testing.assert_allclose(got_m, M, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got_c, cons, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got_s, sc, rtol=0, atol=PO.TOL_SELF_CIDER)
    diag = np.stack([np.diag(m) for m in got_m])
    assert np.array_equal(diag, np.round(np.stack([np.diag(m) for m in M]) / 2.5) * 2.5)                # the diagonal is exact
    if K == 1:
        assert not got_c.any() and not got_s.any()
    assert same_bits(scorer.self_cider(ids, lengths), out["self_cider"])


@pytest.mark.parametrize("case", PO.CASES, ids=lambda c: "V%d-B%d-K%d-L%d" % c)
def test_row_mean_agrees_with_gic_cider_d(dev, case):
    """The K captions as their own references under the existing kernel: the row mean of the matrix, the diagonal included."""
    from gan_image_captioning_amd.cider import RefBatch
    V, B, K, Lmax = case
    prob, _, scorer, ids, lengths = _on_device(case, dev)
    refs = RefBatch.pack([PO.captions(prob, b) for b in range(B)]).to(dev)
    want = scorer.score(ids, lengths, refs)
    got = scorer.pairwise(ids, lengths, want_consensus=False, want_self_cider=False)["matrix"].mean(2)
    torch.cuda.synchronize()
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_each_output_alone_repeat_calls_and_deterministic_mode(E, dev):
    case = PO.CASES[2]                                    # K = 32, L = 64
    _, _, scorer, ids, lengths = _on_device(case, dev)
    full = scorer.pairwise(ids, lengths)
    for name in ("matrix", "consensus", "self_cider"):
        alone = scorer.pairwise(ids, lengths, **{f"want_{k}": k == name for k in ("matrix", "consensus", "self_cider")})
        assert [k for k, v in alone.items() if v is not None] == [name]
        assert same_bits(alone[name], full[name]), name
    runs = [full]
    for det in (True, True, False):
        E.set_deterministic(det)
        try:
            runs.append(scorer.pairwise(ids, lengths))
            torch.cuda.synchronize()
        finally:
            E.set_deterministic(False)
    for other in runs[1:]:
        for name in ("matrix", "consensus", "self_cider"):
            assert same_bits(other[name], full[name]), name
    with pytest.raises(ValueError, match="no output"):
        scorer.pairwise(ids, lengths, want_matrix=False, want_consensus=False, want_self_cider=False)
    with pytest.raises(ValueError, match="1..32"):
        scorer.pairwise(ids.repeat(1, 2, 1)[:, :33], lengths.repeat(1, 2)[:, :33])


def test_a_strided_view_and_lengths_beyond_the_row_are_clamped(dev):
    case = PO.CASES[1]
    prob, (M, _, _), scorer, ids, lengths = _on_device(case, dev)
    wide = torch.full((ids.shape[0], ids.shape[1], ids.shape[2] + 5), 7, dtype=torch.int64, device=dev)
    wide[:, :, :ids.shape[2]] = ids
    got = scorer.pairwise(wide[:, :, :ids.shape[2]], lengths)["matrix"]                     # a view with a row stride: made contiguous
    assert same_bits(got, scorer.pairwise(ids, lengths)["matrix"])
    full = torch.full_like(lengths, ids.shape[2])
    assert same_bits(scorer.pairwise(ids, full + 100)["matrix"], scorer.pairwise(ids, full)["matrix"])
    assert same_bits(scorer.pairwise(ids, -full)["matrix"], scorer.pairwise(ids, full * 0)["matrix"])


# ------------------------------------------------------------------------------------------------ 2. the order, on the pinned cases
def _check_order(E, scorer, df, n, ids, scores, lengths, alphas, lp, w, every_image):
    """Manual composition beams -> pairwise -> engine.rerank, against the oracle on the device's own beams.  Returns the dict."""
    from tests.test_gpu_rerank import check_gather
    pw = scorer.pairwise(ids, lengths, want_matrix=False, want_self_cider=False)
    r = E.rerank(scores, lengths, pw["consensus"].view(-1), 1, w, lp, ids=ids, alphas=alphas)
    torch.cuda.synchronize()
    cons = PO.consensus_of(ids.cpu().numpy(), lengths.cpu().numpy(), df, n)
    np.testing.assert_allclose(pw["consensus"].cpu().double().numpy(), cons, rtol=1e-5, atol=1e-5)
    order, final, gaps = PO.rerank(scores.cpu().numpy(), lengths.cpu().numpy(), cons, w, lp)
    clear = gaps > A.ORDER_GAP
    if every_image:
        assert clear.all(), (lp, w, gaps)
    got = r["order"].cpu().numpy()
    assert np.array_equal(got[clear], order[clear]), (lp, w)
    np.testing.assert_allclose(r["final"].cpu().double().numpy()[clear], final[clear], rtol=1e-5, atol=1e-4)
    assert same_bits(r["d"], pw["consensus"].gather(1, r["order"].long()))
    check_gather({k: (v.cpu() if v is not None else None) for k, v in r.items()}, scores.cpu(), lengths.cpu(), ids.cpu(),
                 alphas.cpu() if alphas is not None else None)
    return r, int(clear.sum())


@pytest.mark.parametrize("case,settings", A.ORDER_CASES, ids=lambda v: T._case_id(v) if isinstance(v, tuple) else None)
def test_order_equals_the_oracle_on_every_image(E, dev, case, settings):
    from tests.test_gpu_constrained import _gpu_beam
    out = _gpu_beam(case, dev)
    ids, scores, lengths = out[0], out[1], out[2]
    alphas = out[3] if len(out) > 3 else None
    corpus, df, n = A.order_table(case)
    V = (T.ATTN_SHAPE if case[0] == "attn" else T.LSTM_SHAPES[case[0]])[2]
    scorer = _scorer(corpus, V, dev)
    moved = False
    for lp, w in settings:
        r, _ = _check_order(E, scorer, df, n, ids, scores, lengths.to(torch.int32), alphas, lp, w, every_image=True)
        moved = moved or r["order"].cpu().tolist() != [list(range(ids.shape[1]))] * ids.shape[0]
    assert moved


# ------------------------------------------------------------------------------------------------ 3. through Generator
def _spy_launches(monkeypatch):
    from gan_image_captioning_amd import _lib
    lib, n = _lib.load(), []
    for name in ("gic_cider_pairwise", "gic_rerank"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (n.append(_name), _real(*a))[1])
    return n


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_caption_with_consensus_is_the_manual_composition(E, dev, kind, monkeypatch):
    from tests.test_gpu_rerank import L as LEN, SEED, _gen
    B, K = 3, 4
    attn = kind == "attention"
    gen = _gen(dev, kind)
    corpus = PO.table_corpus(64)
    df, n = CO.document_frequency(corpus)
    scorer = _scorer(corpus, 64, dev)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(SEED + 21)).to(dev)
    kw = dict(beam_size=K, max_caption_len=LEN, return_beams=True, **(dict(return_alphas=True) if attn else {}))
    launches = _spy_launches(monkeypatch)
    plain = gen.caption(images, **kw)
    off = gen.caption(images, consensus=None, consensus_weight=7.0, **kw)
    torch.cuda.synchronize()
    assert not launches, "consensus=None launched something new"
    assert len(plain) == len(off) == (4 if attn else 3)
    for a, b in zip(plain, off):
        assert torch.equal(a, b)
    compared = 0
    for lp, w in ((0.0, 4.0), (0.7, 2.0), (0.0, 0.0)):
        base = plain if lp == 0.0 else gen.caption(images, length_penalty=lp, **kw)
        del launches[:]
        out = gen.caption(images, length_penalty=lp, consensus=scorer, consensus_weight=w, return_consensus=True, **kw)
        assert launches == ["gic_cider_pairwise", "gic_rerank"]
        best = gen.caption(images, length_penalty=lp, consensus=scorer, consensus_weight=w, **{**kw, "return_beams": False})
        r, c = _check_order(E, scorer, df, n, base[0], base[1], base[2], base[3] if attn else None, lp, w, every_image=False)
        compared += c
        assert len(out) == len(base) + 1 and len(best) == len(base)
        assert torch.equal(out[0], r["ids"]) and same_bits(out[1], r["scores"]) and torch.equal(out[2], r["lengths"])
        if attn:
            assert same_bits(out[3], r["alphas"])                                # the attention maps travel with their captions
        assert same_bits(out[-1][0], r["final"]) and same_bits(out[-1][1], r["d"])
        assert torch.equal(out[1], base[1].gather(1, r["order"].long()))         # scores stay G's log-probabilities
        for a, b in zip(best, out):
            assert torch.equal(a, b[:, 0])
        if w == 0.0:
            assert r["order"].cpu().tolist() == [list(range(K))] * B
    print(f"[cider_pair] caption {kind}: {compared} of {3 * B} orders compared with the oracle")
    with pytest.raises(ValueError, match="one re-ranking at a time"):
        gen.caption(images, consensus=scorer, rerank_disc=object(), **kw)


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_sample_captions_with_consensus_is_the_manual_composition(E, dev, kind, monkeypatch):
    from tests.test_gpu_rerank import L as LEN, SEED, _gen
    B, n_s = 3, 8
    gen = _gen(dev, kind)
    corpus = PO.table_corpus(64)
    df, n = CO.document_frequency(corpus)
    scorer = _scorer(corpus, 64, dev)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(SEED + 22)).to(dev)
    kw = dict(num_samples=n_s, top_k=20, max_caption_len=LEN, seed=5)
    launches = _spy_launches(monkeypatch)
    draw = gen.sample_captions(images, **kw)
    off = gen.sample_captions(images, consensus=None, consensus_weight=3.0, **kw)
    assert not launches
    for a, b in zip(draw, off):
        assert torch.equal(a, b)
    out = gen.sample_captions(images, consensus=scorer, consensus_weight=2.0, **kw)
    assert launches == ["gic_cider_pairwise", "gic_rerank"]
    r, c = _check_order(E, scorer, df, n, draw[0], draw[1], draw[2], None, 0.0, 2.0, every_image=False)
    assert torch.equal(out[0], r["ids"]) and same_bits(out[1], r["scores"]) and torch.equal(out[2], r["lengths"])
    assert [sorted(o) for o in r["order"].cpu().tolist()] == [list(range(n_s))] * B
    print(f"[cider_pair] sample_captions {kind}: {c} of {B} orders compared with the oracle")


# ------------------------------------------------------------------------------------------------ 4. evaluate_consensus
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_evaluate_consensus(dev, kind):
    from gan_image_captioning_amd.tasks import ImageGroups, SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    from tests.test_gpu_constrained import _ATTN, _gen_args
    args = _gen_args(**(_ATTN if kind == "attention" else {}))
    ds = SyntheticCaptionData(6, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    seen, drawn = [], []
    inst.writer.add_scalar = lambda tag, v, step: seen.append((tag, v))
    smp = inst.gen.sample_captions
    inst.gen.sample_captions = lambda *a, **k: (drawn.append(smp(*a, **k)), drawn[-1])[1]
    weight = 2.0
    out = inst.evaluate_consensus("val", num_samples=5, top_k=20, weight=weight)
    assert set(out) == {"cider_d_first", "cider_d_consensus", "self_cider"} and all(math.isfinite(v) for v in out.values())
    assert 0.0 <= out["self_cider"] <= 1.0 and out["cider_d_first"] >= 0.0 and out["cider_d_consensus"] >= 0.0
    assert {t for t, _ in seen} == {"CIDErDFirst_val", "CIDErDConsensus_val", "SelfCIDEr_val"}
    samples = list(drawn)
    assert len(samples) == 2                                                     # six images in batches of four
    assert out == inst.evaluate_consensus("val", num_samples=5, top_k=20, weight=weight)
    # the host recomputation from the samples the evaluation drew
    df, n = CO.document_frequency(ImageGroups(ds).references())
    first, picked, diversity = [], [], []
    replay = lambda images, L, bi: (samples[bi][0], samples[bi][2])             # noqa: E731
    for bi, (ids, lengths, caps) in enumerate(inst._decode_batches("val", replay)):
        ids, lengths, scores = ids.cpu().numpy(), lengths.cpu().numpy(), samples[bi][1].cpu().double().numpy()
        for b, refs in enumerate(caps):
            cand = [ids[b, k, :lengths[b, k]].tolist() for k in range(ids.shape[1])]
            M = PO.pair_matrix(cand, df, n)
            pick = int(np.argsort(-(scores[b] + weight * PO.consensus(M)), kind="stable")[0])
            first.append(CO.cider_d(cand[0], refs, df, n))
            picked.append(CO.cider_d(cand[pick], refs, df, n))
            diversity.append(PO.self_cider(M))
    assert len(first) == 6
    assert abs(out["cider_d_consensus"] - float(np.mean(picked))) <= 1e-4
    assert abs(out["cider_d_first"] - float(np.mean(first))) <= 1e-4
    assert abs(out["self_cider"] - float(np.mean(diversity))) <= 1e-4
