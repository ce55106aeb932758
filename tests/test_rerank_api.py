"""D-guided re-ranking and image-caption retrieval without a GPU: the flags and signatures, the four new entry points' argument checks
(each returns -1 with a message that names the argument, before any launch), the refusals of evaluate_retrieval and
Discriminator.score, and the self-tests of the oracles the GPU tests compare with (tests/rerank_oracle.py, tests/retrieval_oracle.py)."""
import ctypes as C
import inspect
import math

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd.args import default_args
from gan_image_captioning_amd.discriminator import Discriminator
from tests import rerank_oracle as RR
from tests import retrieval_oracle as RO

TINY = dict(vocab_size=50, disc_embed_dim=4, disc_num_rep=4, disc_filter_sizes=[2, 3], disc_num_filters=[24, 16], device="cpu")
NEW = ("gic_disc_match_fwd_grouped", "gic_rerank", "gic_disc_rep_mean", "gic_match_ranks")


# ------------------------------------------------------------------------------------------------ flags, signatures, symbols
def test_flags_exist_with_their_defaults():
    a = default_args()
    assert (a.eval_rerank_weight, a.eval_retrieval, a.eval_retrieval_items) == (0.0, 0, 1000)


def test_new_keywords_and_their_defaults():
    from gan_image_captioning_amd import discriminator
    from gan_image_captioning_amd.engine import DiscEngine
    from gan_image_captioning_amd.generator import Generator
    from gan_image_captioning_amd.training import GANInstructor
    p = inspect.signature(Generator.caption).parameters
    assert (p["rerank_disc"].default, p["rerank_weight"].default, p["return_rerank"].default) == (None, 1.0, False)
    p = inspect.signature(Generator.sample_captions).parameters
    assert (p["rerank_disc"].default, p["rerank_weight"].default) == (None, 1.0)
    p = inspect.signature(Discriminator.score).parameters
    assert list(p) == ["self", "image_features", "ids", "image_index"] and p["image_index"].default is None
    p = inspect.signature(discriminator.rerank).parameters
    assert list(p) == ["disc", "image_features", "ids", "scores", "lengths", "weight", "length_penalty", "alphas"]
    assert (p["weight"].default, p["length_penalty"].default, p["alphas"].default) == (1.0, 0.0, None)
    assert inspect.signature(DiscEngine.match_logits).parameters["q_index"].default is None
    assert inspect.signature(DiscEngine.fwd).parameters["cond_index"].default is None
    p = inspect.signature(GANInstructor.evaluate_retrieval).parameters
    assert (p["what"].default, p["max_items"].default) == ("val", None)


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gic_abi_version() == L.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------ argument checks (host only)
def _dims(B=2, R=4, F=40, Fp=64, dtype=L.F32):
    d = L.DiscDims()
    d.B, d.L, d.V, d.De, d.R, d.nconv, d.F, d.Fp, d.dtype, d.drop_p = B, 7, 50, 4, R, 2, F, Fp, dtype, 0.2
    return d


def _state(ydrop=0x1000):
    s = L.DiscState()
    s.ydrop = ydrop
    return s


def _refused(status, *words):
    assert status == -1
    msg = L.load().gic_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


FAKE = [0x10000 * (i + 1) for i in range(16)]          # distinct non-null addresses 64 KiB apart: never dereferenced (the checks come first)


def test_grouped_match_argument_checks():
    lib = L.load()
    d, st = _dims(), _state()
    q, idx, lg = FAKE[0], FAKE[1], FAKE[2]
    f = lib.gic_disc_match_fwd_grouped
    _refused(f(None, C.byref(st), q, 2, idx, 1.0, 0, lg, None), "null dims")
    _refused(f(C.byref(d), None, q, 2, idx, 1.0, 0, lg, None), "null state")
    _refused(f(C.byref(d), C.byref(st), None, 2, idx, 1.0, 0, lg, None), "null q")
    _refused(f(C.byref(d), C.byref(st), q, 2, idx, 1.0, 0, None, None), "null logits")
    _refused(f(C.byref(d), C.byref(_state(None)), q, 2, idx, 1.0, 0, lg, None), "ydrop")
    _refused(f(C.byref(d), C.byref(st), q, 0, idx, 1.0, 0, lg, None), "q_rows")
    _refused(f(C.byref(d), C.byref(st), q, 3, None, 1.0, 0, lg, None), "q_index", "q_rows=3", "B=2")
    _refused(f(C.byref(_dims(R=0)), C.byref(st), q, 2, idx, 1.0, 0, lg, None), "R=0")
    _refused(f(C.byref(_dims(Fp=36)), C.byref(st), q, 2, idx, 1.0, 0, lg, None), "Fp=36")


def _rerank_args(**kw):
    a = dict(lm=FAKE[0], lengths=FAKE[1], lp=0.0, dl=FAKE[2], R=4, w=0.5, ids=FAKE[3], alphas=FAKE[4], B=3, K=5, L=7, P=4, order=FAKE[5],
             final=FAKE[6], d=FAKE[7], out_ids=FAKE[8], out_lm=FAKE[9], out_len=FAKE[10], out_alphas=FAKE[11])
    a.update(kw)
    return [a[k] for k in ("lm", "lengths", "lp", "dl", "R", "w", "ids", "alphas", "B", "K", "L", "P", "order", "final", "d", "out_ids", "out_lm",
                           "out_len", "out_alphas")] + [None]


def test_rerank_argument_checks():
    f = L.load().gic_rerank
    _refused(f(*_rerank_args(lm=None)), "lm_scores")
    _refused(f(*_rerank_args(lengths=None)), "lengths")
    _refused(f(*_rerank_args(dl=None)), "d_logits")
    _refused(f(*_rerank_args(order=None)), "order")
    for K in (0, 65, -1):
        _refused(f(*_rerank_args(K=K)), f"K={K}")
    for R in (0, -2):
        _refused(f(*_rerank_args(R=R)), f"R={R}")
    _refused(f(*_rerank_args(B=0)), "B=0")
    _refused(f(*_rerank_args(ids=None)), "out_ids")
    _refused(f(*_rerank_args(alphas=None)), "out_alphas")
    # in-place use: an output on (or inside) an input, or on another output
    _refused(f(*_rerank_args(out_lm=FAKE[0])), "out_lm_scores", "aliases", "lm_scores")
    _refused(f(*_rerank_args(out_ids=FAKE[3])), "out_ids", "aliases", "ids")
    _refused(f(*_rerank_args(out_ids=FAKE[3] + 8)), "out_ids", "aliases", "ids")
    _refused(f(*_rerank_args(out_len=FAKE[1])), "out_lengths", "aliases", "lengths")
    _refused(f(*_rerank_args(out_alphas=FAKE[4])), "out_alphas", "aliases", "alphas")
    _refused(f(*_rerank_args(d=FAKE[2])), "d_scores", "aliases", "d_logits")
    _refused(f(*_rerank_args(final=FAKE[5])), "final_scores", "aliases", "order")


def test_rep_mean_argument_checks():
    f = L.load().gic_disc_rep_mean
    d, st = _dims(), _state()
    _refused(f(None, C.byref(st), FAKE[0], FAKE[1], FAKE[2], None), "null dims")
    _refused(f(C.byref(d), None, FAKE[0], FAKE[1], FAKE[2], None), "null state")
    _refused(f(C.byref(d), C.byref(_state(None)), FAKE[0], FAKE[1], FAKE[2], None), "ydrop")
    _refused(f(C.byref(d), C.byref(st), FAKE[0], None, FAKE[2], None), "null ybar")
    _refused(f(C.byref(d), C.byref(st), FAKE[0], FAKE[1], None, None), "logits and lbar")
    _refused(f(C.byref(_dims(R=0)), C.byref(st), FAKE[0], FAKE[1], FAKE[2], None), "R=0")


def test_match_ranks_argument_checks():
    f = L.load().gic_match_ranks
    _refused(f(None, 4, FAKE[1], 4, FAKE[2], FAKE[3], None), "null S")
    _refused(f(FAKE[0], 4, FAKE[1], 4, None, FAKE[3], None), "rank_c2i")
    for N in (0, -3):
        _refused(f(FAKE[0], 4, FAKE[1], N, FAKE[2], FAKE[3], None), f"N={N}")
    _refused(f(FAKE[0], 3, FAKE[1], 4, FAKE[2], FAKE[3], None), "ld=3", "N=4")


# ------------------------------------------------------------------------------------------------ refusals of the module layer
class _Loader:
    """A loader of ``n`` items that must never be iterated: the refusals come first."""

    def __init__(self, n):
        self.dataset = range(n)

    def __iter__(self):
        raise AssertionError("the refusal must come before the first batch")


def _instructor(args, n=40):
    from gan_image_captioning_amd.training import GANInstructor
    inst = GANInstructor.__new__(GANInstructor)
    inst.args, inst.disc = args, Discriminator(args)
    inst.adv_eval_loader = inst.adv_train_loader = _Loader(n)
    return inst


def test_evaluate_retrieval_refusals():
    with pytest.raises(ValueError, match="--disc-cond projection"):
        _instructor(default_args(**TINY)).evaluate_retrieval("val")
    on = dict(disc_cond="projection", conditional_gan=1, **TINY)
    with pytest.raises(ValueError, match="captions-per-image"):
        _instructor(default_args(captions_per_image=5, **on)).evaluate_retrieval("val")
    with pytest.raises(ValueError, match="8192"):
        _instructor(default_args(**on), n=9000).evaluate_retrieval("train")
    with pytest.raises(ValueError, match="8192"):
        _instructor(default_args(**on), n=9000).evaluate_retrieval("val", max_items=8193)


def test_retrieval_is_sized_from_what_the_loader_yields():
    """Under data parallelism both adversarial loaders carry a DistributedSampler: rank 0 sees len / world_size items, not the dataset."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from gan_image_captioning_amd.training import GANInstructor
    ds = list(range(5000))
    shard = DataLoader(ds, batch_size=64, sampler=DistributedSampler(ds, num_replicas=8, rank=0, shuffle=False))
    assert GANInstructor._loader_items(shard) == 625 and GANInstructor._loader_items(DataLoader(ds, batch_size=64)) == 5000
    assert GANInstructor._loader_items(_Loader(40)) == 40
    assert GANInstructor._loader_items([(None, torch.zeros(8, 3)), (None, torch.zeros(5, 3))]) == 13
    # a 9000-item dataset of which this rank yields 625: no refusal for size (the loader is then read: its first batch is the sentinel)
    on = dict(disc_cond="projection", conditional_gan=1, **TINY)
    inst = _instructor(default_args(**on), n=9000)
    inst.adv_eval_loader.sampler = range(625)
    with pytest.raises(AssertionError, match="before the first batch"):
        inst.evaluate_retrieval("val")
    inst.adv_eval_loader.sampler = range(9000)
    with pytest.raises(ValueError, match="8192"):
        inst.evaluate_retrieval("val")


def test_fwd_refuses_an_index_without_q_before_anything_runs():
    from gan_image_captioning_amd.engine import DiscEngine
    eng = DiscEngine(50, 4, 4, [2, 3], [24, 16], L.F32)
    with pytest.raises(ValueError, match="cond_index without cond"):
        eng.fwd(None, None, None, False, cond_index=torch.zeros(2, dtype=torch.int32))
    d = _dims(B=65536)
    _refused(L.load().gic_disc_rep_mean(C.byref(d), C.byref(_state()), FAKE[0], FAKE[1], FAKE[2], None), "B=65536", "65535")


def test_score_refuses_features_for_an_unconditioned_discriminator():
    ids = torch.zeros(2, 3, 6, dtype=torch.int64)
    with pytest.raises(ValueError, match="without --disc-cond projection"):
        Discriminator(default_args(**TINY)).score(torch.zeros(2, 512), ids)
    with pytest.raises(ValueError, match="without --disc-cond projection"):
        Discriminator(default_args(**TINY)).score(None, ids[:, 0], image_index=torch.zeros(2, dtype=torch.int32))
    on = Discriminator(default_args(disc_cond="projection", conditional_gan=1, **TINY))
    with pytest.raises(ValueError, match="needs image_features"):
        on.score(None, ids)
    with pytest.raises(ValueError, match="3 rows for 2 images"):
        on.score(torch.zeros(3, 512), ids)
    with pytest.raises(ValueError, match="image_index must be"):
        on.score(torch.zeros(3, 512), ids[:, 0], image_index=torch.zeros(5, dtype=torch.int32))
    assert on.training                                # (the mode is untouched by a refusal)


def test_caption_refuses_return_rerank_without_a_discriminator():
    from gan_image_captioning_amd.generator import Generator
    gen = Generator.__new__(Generator)
    torch.nn.Module.__init__(gen)
    gen.decoder = object()
    with pytest.raises(ValueError, match="return_rerank needs rerank_disc"):
        gen.caption(None, return_rerank=True)


# ------------------------------------------------------------------------------------------------ the oracles' self-tests
def test_rerank_oracle_ties_nan_and_weight_zero():
    B, K, R = 2, 5, 4
    lm = torch.tensor([[-1.0, -2.0, -2.0, -3.0, -4.0], [-1.0, -1.0, -1.0, -1.0, -1.0]])
    lengths = torch.full((B, K), 3, dtype=torch.int32)
    dl = torch.zeros(B, K, R)
    dl[0, 3] = 5.0                                       # beam 3 of image 0 wins under a positive weight
    dl[1, 2, 1] = float("nan")                           # a NaN logit: that beam goes last
    ref = RR.rerank(lm, lengths, 0.0, dl.view(-1), R, 0.5)
    assert ref["order"].tolist() == [[3, 0, 1, 2, 4], [0, 1, 3, 4, 2]]          # equal finals: the lower input index first; NaN last
    assert ref["final"][0].tolist() == [-0.5, -1.0, -2.0, -2.0, -4.0] and math.isnan(float(ref["final"][1, -1]))
    assert ref["d"][0].tolist() == [5.0, 0.0, 0.0, 0.0, 0.0]
    # weight 0: the identity on an input that is already sorted, whatever D says (the NaN logit included)
    ref0 = RR.rerank(lm, lengths, 0.0, dl.view(-1), R, 0.0)
    assert ref0["order"].tolist() == [list(range(K))] * B and torch.equal(ref0["final"], lm.double())
    assert not torch.isnan(ref0["bound"]).any()
    # a negative weight reverses D's preference; the length penalty divides by len ** lp
    assert RR.rerank(lm, lengths, 0.0, dl.view(-1), R, -1.0)["order"][0].tolist() == [0, 1, 2, 4, 3]
    lens = torch.tensor([[1, 2, 4, 8, 16]] * B, dtype=torch.int32)
    assert torch.allclose(RR.lm_terms(lm, lens, 0.5)[0], lm[0].double() / torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0]).sqrt().double())
    assert float(RR.lm_terms(lm, torch.zeros(B, K, dtype=torch.int32), 0.7)[0, 0]) == -1.0       # max(len, 1)


def test_rerank_oracle_clear_rule_and_check():
    B, K, R = 1, 3, 1
    lengths = torch.ones(B, K, dtype=torch.int32)
    far = RR.rerank(torch.tensor([[-1.0, -2.0, -3.0]]), lengths, 0.0, torch.zeros(3), R, 1.0)
    near = RR.rerank(torch.tensor([[-1.0, -1.0 - 2e-7, -3.0]]), lengths, 0.0, torch.zeros(3), R, 1.0)
    assert RR.clear_images(far) == [True] and RR.clear_images(near) == [False]
    tie = RR.rerank(torch.tensor([[-1.0, -1.0, -3.0]]), lengths, 0.0, torch.zeros(3), R, 1.0)
    assert RR.clear_images(tie) == [True]                # an exact tie is no gap: the index decides
    order = torch.tensor([[0, 1, 2]])
    assert RR.check(far, order, far["final"].float(), far["d"].float())[0] == 0
    with pytest.raises(AssertionError, match="is clear"):
        RR.check(far, torch.tensor([[1, 0, 2]]), far["final"].float()[:, [1, 0, 2]], far["d"].float())
    with pytest.raises(AssertionError, match="above bound"):
        RR.check(far, order, far["final"].float() + 1e-5, far["d"].float())
    # not clear: either order of the two near beams passes as long as the finals are theirs
    swapped = near["final_in"].float()[:, [1, 0, 2]]
    assert RR.check(near, torch.tensor([[1, 0, 2]]), torch.tensor([[-1.0, -1.0 - 2.0 ** -23, -3.0]]), near["d"].float())[0] == 1
    with pytest.raises(AssertionError, match="contradicts"):
        RR.check(near, torch.tensor([[1, 0, 2]]), swapped, near["d"].float())


def test_synthetic_cases_are_clear_in_the_oracle_alone():
    """The GPU test allows at most 1 image in 10 per case to be not clear; with 3 images that is none.  The seed is chosen for it here."""
    for K, R, P in RR.synthetic_cases():
        lm, lengths, d_logits, ids, alphas = RR.synthetic(K, R, P)
        assert bool((lm[:, :-1] >= lm[:, 1:]).all()) and ids.shape == (RR.SYN_B, K, RR.SYN_L) and (alphas is None) == (P == 0)
        for lp in RR.SYN_LP:
            for w in RR.SYN_W:
                ref = RR.rerank(lm, lengths, lp, d_logits, R, w)
                assert all(RR.clear_images(ref)), (K, R, P, lp, w)
                if w == 0.0 and lp == 0.0:
                    assert ref["order"].tolist() == [list(range(K))] * RR.SYN_B


def test_retrieval_oracle_ties_and_nan_count_against():
    S = torch.tensor([[3.0, 1.0, 3.0], [0.0, 2.0, 5.0], [1.0, float("nan"), 4.0]])
    c2i, i2c = RO.ranks_exact(S)
    assert c2i.tolist() == [1, 1, 1]                      # row 0: the tie with column 2; row 1: 5 > 2; row 2: the NaN
    assert i2c.tolist() == [0, 1, 1]                      # column 1: the NaN; column 2: 5 > 4 (3 < 4 is no hit)
    assert [v.tolist() for v in RO.ranks_exact(torch.ones(4, 4))] == [[3] * 4, [3] * 4]        # all equal: every rank is N - 1
    assert [v.tolist() for v in RO.ranks_exact(torch.tensor([[7.0]]))] == [[0], [0]]
    # the bias moves a row as a whole: row ranks are unchanged, column ranks are not
    b = torch.tensor([0.0, 10.0, 0.0])
    c2, i2 = RO.ranks_exact(S, b)
    assert c2.tolist() == c2i.tolist() and i2.tolist() == [1, 1, 1]


def test_retrieval_oracle_duplicated_q_rows_tie():
    g = torch.Generator().manual_seed(3)
    N, F, R = 6, 8, 2
    y = torch.randn(N * R, F, generator=g)
    q = torch.randn(N, F, generator=g)
    q[4] = q[1]                                           # two images with the same projection
    ybar, lbar, yb, lb = RO.rep_mean(y, torch.randn(N * R, generator=g), R, F)
    T, bound = RO.pair_scores(ybar, lbar, q, yb, lb)
    assert torch.equal(T[:, 1], T[:, 4]) and bool((bound > 0).all())
    c2i, _ = RO.ranks_exact(T.float())
    alone = RO.ranks_exact(torch.cat([T[:, :4], T[:, 5:]], 1)[[0, 1, 2, 3, 5]].float())[0]
    assert int(c2i[1]) == int(alone[1]) + 1 and int(c2i[4]) >= 1          # the twin ties with the true image, and a tie counts against
    iv = RO.rank_intervals(T, bound)
    for name, exact in (("c2i", c2i), ("i2c", RO.ranks_exact(T.float())[1])):
        lo, hi = iv[name]
        assert bool((lo <= hi).all()) and bool((hi >= exact).all())
    assert int(iv["c2i"][1][1]) > int(iv["c2i"][0][1])   # the twin lies within the bound: hi counts it, lo does not


def test_recall_and_median_from_known_ranks():
    from gan_image_captioning_amd.metrics import retrieval_summary
    ranks = [0, 0, 3, 4, 9, 10, 50, 7]
    want = {"r1": 2 / 8, "r5": 4 / 8, "r10": 6 / 8, "medr": 1.0 + 0.5 * (4 + 7), "meanr": 1.0 + sum(ranks) / 8}
    assert RO.summary(ranks) == want and retrieval_summary(torch.tensor(ranks, dtype=torch.int32)) == want
    assert RO.summary([2, 0, 1])["medr"] == 2.0 and retrieval_summary([0])["medr"] == 1.0
    assert RO.recall_at([0, 1, 2, 3], 1) == 0.25
