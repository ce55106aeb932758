"""D-guided re-ranking on the GPU: the match term with an image index per caption (gic_disc_match_fwd_grouped), gic_rerank, the forms of
Discriminator.score, and the composed decode of both decoders (Generator.caption / sample_captions with rerank_disc).

Bounds (u = eps = 2^-24, none fitted): the grouped match term (F + 4) u s sum |y q| as tests/disc_cond_oracle.check_match_only, added onto
logits (F + 5) u (|logits before| + s sum |y q|); gic_rerank as tests/rerank_oracle.py states them.  The match kernel reads nothing
of a state but ydrop, so the tests hand it a ydrop of their own (pad columns zero, as every forward leaves them).
Largest err / bound seen on an MI355X: see DESIGN.md section 19."""
import pytest
import torch

from tests import disc_cases as D
from tests import disc_cond_oracle as DC
from tests import rerank_oracle as RR
from tests.rerank_cases import spread

pytestmark = pytest.mark.gpu

R, L, V = 4, 7, 50
FILTERS = {"f40": (24, 16), "f15": (9, 6)}            # F = Fp = 40; F = 15, Fp = 16 (a pad column, F % 4 != 0)
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
SEED = 1913


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


def make_engine(E, shape, dtype, monkeypatch, rep=R):
    monkeypatch.setenv("GIC_DISC_FP_ALIGN", "8")
    nf = FILTERS[shape]
    eng = E.DiscEngine(V, rep, rep, [2, 3], list(nf), E.DTYPE_BY_NAME[dtype])
    assert (eng.F, eng.Fp) == {"f40": (40, 40), "f15": (15, 16)}[shape]
    return eng


def make_ydrop(eng, captions, dtype, gen, rep=R):
    y = torch.randn(captions * rep, eng.Fp, generator=gen).to(TD[dtype])
    y[:, eng.F:] = 0
    return y


INDEX = {"grouped": lambda B, rows: torch.arange(B) // 3, "permuted": lambda B, rows: torch.tensor([4, 2, 5, 0, 3, 1]),
         "repeated-unused": lambda B, rows: torch.tensor([0, 2, 2, 0, 2, 2])}
QROWS = {"grouped": 2, "permuted": 6, "repeated-unused": 3}


# ------------------------------------------------------------------------------------------------ 1. the grouped match term
@pytest.mark.parametrize("kind", list(INDEX))
@pytest.mark.parametrize("accumulate", [False, True], ids=["alone", "acc"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(FILTERS))
def test_grouped_match_element_wise(E, dev, shape, dtype, accumulate, kind, monkeypatch):
    B = 6
    eng = make_engine(E, shape, dtype, monkeypatch)
    gen = torch.Generator().manual_seed(SEED)
    y = make_ydrop(eng, B, dtype, gen)
    rows = QROWS[kind]
    q = torch.randn(rows, eng.F, generator=gen)
    idx = INDEX[kind](B, rows).to(torch.int32)
    before = torch.randn(B * R, generator=gen)
    logits = before.clone().to(dev)
    out = eng.match_logits({"ydrop": y.to(dev)}, q.to(dev), logits=logits, accumulate=accumulate, q_index=idx.to(dev))
    torch.cuda.synchronize()
    assert out is logits
    yd, qd = y[:, :eng.F].double(), q.double()
    ref = RR.match_term_indexed(yd, qd, idx, R)
    mag = RR.match_term_indexed(yd.abs(), qd.abs(), idx, R)
    rep = D.Report()
    if accumulate:
        rep.check("grouped match", logits.cpu(), before.double() + ref, (eng.F + 5) * D.U * (before.double().abs() + mag))
    else:
        rep.check("grouped match", logits.cpu(), ref, (eng.F + 4) * D.U * mag)
    print(f"[rerank] grouped match {shape}-{dtype}-{kind}-{'acc' if accumulate else 'alone'}: err/bound {rep.ratio['grouped match']:.3f}")
    assert not rep.failed, rep.failed


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(FILTERS))
def test_identity_index_is_gic_disc_match_fwd_bit_for_bit(E, dev, shape, dtype, monkeypatch):
    import ctypes as C
    from gan_image_captioning_amd import _lib
    B = 6
    eng = make_engine(E, shape, dtype, monkeypatch)
    gen = torch.Generator().manual_seed(SEED + 1)
    state = {"ydrop": make_ydrop(eng, B, dtype, gen).to(dev)}
    q = torch.randn(B, eng.F, generator=gen).to(dev)
    base = torch.randn(B * R, generator=gen).to(dev)
    for acc in (False, True):
        want = eng.match_logits(state, q, logits=base.clone(), accumulate=acc)
        explicit = eng.match_logits(state, q, logits=base.clone(), accumulate=acc, q_index=torch.arange(B, dtype=torch.int32, device=dev))
        null = base.clone()                           # q_index == NULL through the grouped entry itself
        _lib.check(_lib.load().gic_disc_match_fwd_grouped(C.byref(eng.dims(B, 3)), C.byref(eng._state_struct(state)), q.data_ptr(), B, None,
                                                          eng.match_scale(), int(acc), null.data_ptr(), E.stream_ptr()), "grouped")
        torch.cuda.synchronize()
        assert same_bits(want, explicit) and same_bits(want, null), f"accumulate={acc}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_out_of_range_index_gives_nan_and_reads_nothing(E, dev, dtype, monkeypatch):
    import ctypes as C
    from gan_image_captioning_amd import _lib
    B, rows = 6, 2
    eng = make_engine(E, "f15", dtype, monkeypatch)
    gen = torch.Generator().manual_seed(SEED + 2)
    state = {"ydrop": make_ydrop(eng, B, dtype, gen).to(dev)}
    q = torch.randn(rows + 1, eng.F, generator=gen).to(dev)          # one row more than the call is told about: index `rows` stays in memory
    good = (torch.arange(B) // 3).to(torch.int32)
    # the bad index is q_rows itself: were it dereferenced, the read would still land inside the allocation (a failed assertion, never a
    # fault).  Negative and huge indices take the same branch, one unsigned comparison `(unsigned)index < (unsigned)q_rows` in the kernel.
    d = eng.dims(B, 3)
    for bad_at in (4, 1):
        idx = good.clone()
        idx[bad_at] = rows
        for acc in (0, 1):
            ref, got = torch.zeros(B * R, device=dev), torch.zeros(B * R, device=dev)
            for index, out in ((good, ref), (idx, got)):
                index = index.to(dev)
                _lib.check(_lib.load().gic_disc_match_fwd_grouped(C.byref(d), C.byref(eng._state_struct(state)), q.data_ptr(), rows, index.data_ptr(),
                                                                  eng.match_scale(), acc, out.data_ptr(), E.stream_ptr()), "grouped")
            torch.cuda.synchronize()
            rows_bad = slice(bad_at * R, (bad_at + 1) * R)
            assert bool(torch.isnan(got[rows_bad]).all()), (bad_at, got)
            keep = torch.ones(B * R, dtype=torch.bool, device=dev)
            keep[rows_bad] = False
            assert same_bits(got[keep], ref[keep]) and not bool(torch.isnan(ref).any())


# ------------------------------------------------------------------------------------------------ 2. gic_rerank on synthetic inputs
def run_rerank(E, dev, lm, lengths, d_logits, ids, alphas, rep, lp, w):
    out = E.rerank(lm.to(dev), lengths.to(dev), d_logits.to(dev), rep, w, lp, ids=ids.to(dev) if ids is not None else None,
                   alphas=alphas.to(dev) if alphas is not None else None)
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def check_gather(out, lm, lengths, ids, alphas):
    """Every gathered output is input[order], bit for bit."""
    o = out["order"].long()
    assert same_bits(out["scores"], lm.gather(1, o)) and torch.equal(out["lengths"], lengths.gather(1, o))
    if ids is not None:
        assert torch.equal(out["ids"], ids.gather(1, o[:, :, None].expand_as(ids)))
    if alphas is not None:
        assert same_bits(out["alphas"], alphas.gather(1, o[:, :, None, None].expand_as(alphas)))
    else:
        assert out["alphas"] is None


@pytest.mark.parametrize("K,rep,P", list(RR.synthetic_cases()), ids=lambda v: str(v))
def test_rerank_synthetic(E, dev, K, rep, P):
    lm, lengths, d_logits, ids, alphas = RR.synthetic(K, rep, P)
    worst = 0.0
    for lp in RR.SYN_LP:
        for w in RR.SYN_W:
            ref = RR.rerank(lm, lengths, lp, d_logits, rep, w)
            out = run_rerank(E, dev, lm, lengths, d_logits, ids, alphas, rep, lp, w)
            unclear, ratio = RR.check(ref, out["order"], out["final"], out["d"])
            worst = max(worst, ratio)
            assert 10 * unclear <= RR.SYN_B, f"lp={lp} w={w}: {unclear} of {RR.SYN_B} images are not clear"
            check_gather(out, lm, lengths, ids, alphas)
            if w == 0.0 and lp == 0.0:                 # the input is sorted: the identity, exactly
                assert out["order"].tolist() == [list(range(K))] * RR.SYN_B and same_bits(out["final"], lm)
    print(f"[rerank] K={K} R={rep} P={P}: err/bound {worst:.3f}")


def test_rerank_exact_ties_and_a_nan_logit(E, dev):
    B, K, rep = 3, 5, 4
    gen = torch.Generator().manual_seed(SEED + 3)
    lm = torch.tensor([[-1.5, -2.25, -2.25, -2.25, -7.0], [-3.0] * 5, [-1.0, -2.0, -3.0, -4.0, -5.0]])
    lengths = torch.tensor([[4, 3, 3, 3, 2], [5] * 5, [1, 2, 3, 4, 5]], dtype=torch.int32)
    dl = torch.randn(B, K, rep, generator=gen)
    dl[0, 1:4] = dl[0, 1]                              # image 0: beams 1..3 carry equal inputs -> equal finals -> index order
    dl[1, :] = dl[1, 0]                                # image 1: all five equal
    dl[2, 1, 2] = float("nan")                         # image 2: beam 1 has a NaN logit -> last
    ids = torch.randint(0, V, (B, K, L), generator=gen)
    for lp, w in ((0.0, 0.5), (0.7, -1.0), (0.7, 0.0)):
        ref = RR.rerank(lm, lengths, lp, dl.view(-1), rep, w)
        out = run_rerank(E, dev, lm, lengths, dl.view(-1), ids, None, rep, lp, w)
        RR.check(ref, out["order"], out["final"], out["d"])
        check_gather(out, lm, lengths, ids, None)
        order = out["order"].tolist()
        pos = [order[0].index(k) for k in (1, 2, 3)]
        assert pos == sorted(pos) and pos[2] - pos[0] == 2, order[0]
        assert order[1] == list(range(K))
        if w != 0.0:
            assert order[2][-1] == 1 and bool(torch.isnan(out["final"][2, -1])) and not bool(torch.isnan(out["final"][2, :-1]).any())
        else:
            assert not bool(torch.isnan(out["final"]).any())          # weight 0: D has no say, the NaN logit included
        assert bool(torch.isnan(out["d"][2][order[2].index(1)]))


# ------------------------------------------------------------------------------------------------ 3. the forms of Discriminator.score
def _disc(dev, cond="projection", seed=11):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.discriminator import Discriminator
    args = default_args(vocab_size=64, disc_embed_dim=R, disc_num_rep=R, disc_filter_sizes=[2, 3], disc_num_filters=[24, 16], conditional_gan=1,
                        disc_cond=cond, compute_dtype="fp32", encoder_arch="resnet18", device="cuda")
    torch.manual_seed(seed)
    disc = Discriminator(args).to(dev)
    with torch.no_grad():
        for p in disc.parameters():
            p.mul_(4.0)                                # scores that differ between captions by more than rounding
    return disc.train()


def test_score_forms(dev):
    B, K, C = 3, 5, 512
    gen = torch.Generator().manual_seed(SEED + 4)
    disc = _disc(dev)
    ids = torch.randint(0, 64, (B, K, L), generator=gen).to(dev)
    feats = torch.randn(B, C, generator=gen).to(dev)
    grouped = disc.score(feats, ids)
    repeated = disc.score(feats.repeat_interleave(K, 0), ids.view(B * K, L))
    index = torch.arange(B * K, device=dev) // K
    indexed = disc.score(feats, ids.view(B * K, L), image_index=index)
    perm = torch.randperm(B * K, generator=gen).to(dev)
    shuffled = disc.score(feats, ids.view(B * K, L)[perm], image_index=index[perm].to(torch.int32))
    torch.cuda.synchronize()
    assert grouped.shape == (B, K) and repeated.shape == (B * K,) and disc.training
    assert same_bits(grouped.view(-1), repeated) and same_bits(indexed, repeated)
    # the CPU oracle (fp64), at the tolerance of test_gpu_disc_cond_step's score check
    dp = {k: v.detach().cpu().double() for k, v in disc.state_dict().items()}
    one_hot = torch.nn.functional.one_hot(ids.view(B * K, L).cpu(), 64).double()
    ref = DC.disc_forward(dp, one_hot, feats.cpu().double().repeat_interleave(K, 0), None, R).view(B * K, R).mean(1)
    tol = 1e-4 * ref.abs() + 1e-5 * float(ref.abs().max())
    assert bool(((repeated.cpu().double() - ref).abs() <= tol).all())
    assert bool(((shuffled.cpu().double() - ref[perm.cpu()]).abs() <= tol[perm.cpu()]).all())
    assert float((grouped[:, 0] - grouped[:, 1]).abs().max()) > 0
    # a D without the flag: the captions alone, = the mean of forward()'s eval logits
    plain = _disc(dev, cond="none")
    sc = plain.score(None, ids)
    with torch.no_grad():
        want = plain.eval()(ids.view(B * K, L)).view(B * K, R).mean(1)
    torch.cuda.synchronize()
    assert sc.shape == (B, K) and same_bits(sc.view(-1), want)


# ------------------------------------------------------------------------------------------------ 4. composed decoding
def _gen(dev, kind, seed=4):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.generator import Generator
    kw = dict(decoder="attention", attn_dim=16) if kind == "attention" else dict(gen_num_layers=1)
    args = default_args(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, compute_dtype="fp32", image_size=64, conditional_gan=1,
                        encoder_arch="resnet18", max_seq_len=L, device="cuda", log_file=None, model_dir=None, save_dir=None, **kw)
    torch.manual_seed(seed)
    gen = Generator(args).to(dev).eval()
    spread(gen)
    return gen


def _spy_rerank(E, monkeypatch):
    """Record every engine.rerank call: its inputs and the dict it returns."""
    calls, real = [], E.rerank

    def spy(lm, lengths, d_logits, rep, weight, length_penalty=0.0, ids=None, alphas=None):
        out = real(lm, lengths, d_logits, rep, weight, length_penalty, ids=ids, alphas=alphas)
        calls.append((dict(lm=lm, lengths=lengths, d_logits=d_logits, rep=rep, weight=weight, lp=length_penalty, ids=ids, alphas=alphas), out))
        return out
    monkeypatch.setattr(E, "rerank", spy)
    return calls


def _spy_launches(monkeypatch):
    """Count the launches of gic_rerank itself (the bound symbol)."""
    from gan_image_captioning_amd import _lib
    lib, n = _lib.load(), []
    real = lib.gic_rerank
    monkeypatch.setattr(lib, "gic_rerank", lambda *a: (n.append(1), real(*a))[1])
    return n


@pytest.mark.parametrize("cond", ["projection", "none"])
@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_caption_reranked_against_the_oracle(E, dev, kind, cond, monkeypatch):
    B, K = 3, 5
    attn = kind == "attention"
    gen, disc = _gen(dev, kind), _disc(dev, cond)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(SEED + 5)).to(dev)
    launches = _spy_launches(monkeypatch)
    calls = _spy_rerank(E, monkeypatch)
    kw = dict(beam_size=K, max_caption_len=L, return_beams=True, **(dict(return_alphas=True) if attn else {}))
    plain = gen.caption(images, **kw)
    off = gen.caption(images, rerank_disc=None, rerank_weight=7.0, **kw)
    torch.cuda.synchronize()
    assert not launches and not calls, "rerank_disc=None launched gic_rerank"
    assert len(plain) == len(off) == (4 if attn else 3)
    for a, b in zip(plain, off):
        assert torch.equal(a, b)
    worst, moved = 0.0, False
    for lp, w in ((0.0, 50.0), (0.7, -80.0), (0.0, 0.0)):
        base = plain if lp == 0.0 else gen.caption(images, length_penalty=lp, **kw)
        del calls[:], launches[:]
        out = gen.caption(images, length_penalty=lp, rerank_disc=disc, rerank_weight=w, return_rerank=True, **kw)
        best = gen.caption(images, length_penalty=lp, rerank_disc=disc, rerank_weight=w, **{**kw, "return_beams": False})
        torch.cuda.synchronize()
        assert len(launches) == len(calls) == 2 and len(out) == len(base) + 1 and len(best) == len(base)
        ins, res = calls[0]
        # what the kernel was given: the plain search's beams, bit for bit, and D's logits of them (the CPU oracle's, fp64)
        assert torch.equal(ins["ids"], base[0]) and same_bits(ins["lm"], base[1]) and torch.equal(ins["lengths"], base[2])
        assert (ins["rep"], ins["weight"], ins["lp"]) == (R, w, lp) and (ins["alphas"] is not None) == attn
        if attn:
            assert same_bits(ins["alphas"], base[3])
        dp = {k: v.detach().cpu().double() for k, v in disc.state_dict().items()}
        one_hot = torch.nn.functional.one_hot(base[0].view(B * K, L).cpu(), 64).double()
        if cond == "projection":
            pooled = gen.encoder.last_trunk.float().cpu().double().repeat_interleave(K, 0)
            d_ref = DC.disc_forward(dp, one_hot, pooled, None, R)
        else:
            from oracle import cpu_step as O
            d_ref = O.disc_forward(dp, one_hot, None, R)
        got = ins["d_logits"].cpu().double()
        assert bool(((got - d_ref).abs() <= 1e-4 * d_ref.abs() + 1e-5 * float(d_ref.abs().max())).all()), "D's logits of the beams"
        # the re-rank itself, against the fp64 oracle on the kernel's own f32 inputs
        lm, lengths, dl = ins["lm"].cpu(), ins["lengths"].cpu(), ins["d_logits"].cpu()
        ref = RR.rerank(lm, lengths, lp, dl, R, w)
        order = res["order"].cpu()
        unclear, ratio = RR.check(ref, order, out[-1][0].cpu(), out[-1][1].cpu())
        worst = max(worst, ratio)
        assert 10 * unclear <= B, f"{unclear} of {B} images are not clear"
        got = {"order": order, "scores": out[1].cpu(), "lengths": out[2].cpu(), "ids": out[0].cpu(), "alphas": out[3].cpu() if attn else None}
        check_gather(got, lm, lengths, base[0].cpu(), base[3].cpu() if attn else None)
        for a, b in zip(best, out):
            assert torch.equal(a, b[:, 0])
        if w == 0.0:
            assert order.tolist() == [list(range(K))] * B
        else:
            moved = moved or order.tolist() != [list(range(K))] * B
    assert moved, "the discriminator changed no order under either weight: the test shows nothing"
    print(f"[rerank] caption {kind}-{cond}: err/bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_diverse_and_constrained_searches_rerank_too(E, dev, kind, monkeypatch):
    B, K = 3, 4
    gen, disc = _gen(dev, kind), _disc(dev)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(SEED + 6)).to(dev)
    calls = _spy_rerank(E, monkeypatch)
    for extra in (dict(beam_groups=2, diversity=0.5), dict(no_repeat_ngram=2, min_length=3, suppress_tokens=(1, 3))):
        kw = dict(beam_size=K, max_caption_len=L, return_beams=True, **extra)
        base = gen.caption(images, **kw)
        del calls[:]
        out = gen.caption(images, rerank_disc=disc, rerank_weight=50.0, return_rerank=True, **kw)
        torch.cuda.synchronize()
        ins, res = calls[0]
        assert torch.equal(ins["ids"], base[0])
        ref = RR.rerank(ins["lm"].cpu(), ins["lengths"].cpu(), 0.0, ins["d_logits"].cpu(), R, 50.0)
        unclear, _ = RR.check(ref, res["order"].cpu(), out[-1][0].cpu(), out[-1][1].cpu())
        assert 10 * unclear <= B
        check_gather({"order": res["order"].cpu(), "scores": out[1].cpu(), "lengths": out[2].cpu(), "ids": out[0].cpu(), "alphas": None},
                     base[1].cpu(), base[2].cpu(), base[0].cpu(), None)


@pytest.mark.parametrize("kind", ["lstm", "attention"])
def test_sample_captions_best_of_n_is_a_permutation_of_the_draw(E, dev, kind, monkeypatch):
    B, n = 3, 8
    gen, disc = _gen(dev, kind), _disc(dev)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(SEED + 7)).to(dev)
    calls = _spy_rerank(E, monkeypatch)
    kw = dict(num_samples=n, top_k=20, max_caption_len=L, seed=5)
    draw = gen.sample_captions(images, **kw)
    assert not calls
    out = gen.sample_captions(images, rerank_disc=disc, rerank_weight=50.0, **kw)
    torch.cuda.synchronize()
    ins, res = calls[0]
    assert torch.equal(ins["ids"], draw[0]) and same_bits(ins["lm"], draw[1]) and ins["lp"] == 0.0
    order = res["order"].cpu()
    assert [sorted(o) for o in order.tolist()] == [list(range(n))] * B
    check_gather({"order": order, "scores": out[1].cpu(), "lengths": out[2].cpu(), "ids": out[0].cpu(), "alphas": None},
                 draw[1].cpu(), draw[2].cpu(), draw[0].cpu(), None)
    ref = RR.rerank(ins["lm"].cpu(), ins["lengths"].cpu(), 0.0, ins["d_logits"].cpu(), R, 50.0)
    RR.check(ref, order, res["final"].cpu(), res["d"].cpu())
    f = res["final"].cpu()
    assert bool((f[:, :-1] >= f[:, 1:]).all())


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_same_bits_in_and_out_of_deterministic_mode(E, dev, monkeypatch):
    B, K, P = 6, 8, 4
    eng = make_engine(E, "f15", "bf16", monkeypatch)
    gen = torch.Generator().manual_seed(SEED + 8)
    state = {"ydrop": make_ydrop(eng, B, "bf16", gen).to(dev)}
    q = torch.randn(2, eng.F, generator=gen).to(dev)
    idx = (torch.arange(B) // 3).to(torch.int32).to(dev)
    lm, lengths, d_logits, ids, alphas = RR.synthetic(K, R, P)
    runs = []
    for det in (True, True, False):
        E.set_deterministic(det)
        try:
            m = eng.match_logits(state, q, q_index=idx)
            r = E.rerank(lm.to(dev), lengths.to(dev), d_logits.to(dev), R, 0.5, 0.7, ids=ids.to(dev), alphas=alphas.to(dev))
            torch.cuda.synchronize()
        finally:
            E.set_deterministic(False)
        runs.append((m.cpu(), r["final"].cpu(), r["d"].cpu(), r["order"].cpu(), r["alphas"].cpu()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
