"""Image-caption retrieval on the GPU: gic_disc_rep_mean element by element, gic_match_ranks against the integer oracle (exactly: the
same f32 inputs, one f32 addition and comparisons), and GANInstructor.evaluate_retrieval end to end against rank intervals derived from
the buffers its kernels wrote (tests/retrieval_oracle.py).  Bounds with eps = 2^-24, none fitted: ybar / lbar (R + 2) eps mean_r |.|; a pair
score the f32 GEMM's 2 F eps s sum |ybar||q| plus those of ybar and lbar and one rounding of the sum.
Largest err / bound seen on an MI355X: see DESIGN.md section 19."""
import pytest
import torch

from tests import disc_cases as D
from tests import retrieval_oracle as RO
from tests.rerank_cases import spread

pytestmark = pytest.mark.gpu

V = 50
FILTERS = {"f40": (24, 16), "f15": (9, 6), "f300": (200, 100)}          # f300: Fp = 304, a second workgroup of 64 x 4 columns
FDIMS = {"f40": (40, 40), "f15": (15, 16), "f300": (300, 304)}
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
SEED = 2011


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


# ------------------------------------------------------------------------------------------------ 1. gic_disc_rep_mean
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(FILTERS))
@pytest.mark.parametrize("rep", [1, 3, 64])
@pytest.mark.parametrize("C", [1, 5])
def test_rep_mean_element_wise(E, dev, C, rep, shape, dtype, monkeypatch):
    monkeypatch.setenv("GIC_DISC_FP_ALIGN", "8")
    eng = E.DiscEngine(V, rep, rep, [2, 3], list(FILTERS[shape]), E.DTYPE_BY_NAME[dtype])
    assert (eng.F, eng.Fp) == FDIMS[shape]
    gen = torch.Generator().manual_seed(SEED + rep)
    y = torch.randn(C * rep, eng.Fp, generator=gen).to(TD[dtype])
    y[:, eng.F:] = 7.0                                   # the pad columns must not be read into a result
    logits = torch.randn(C * rep, generator=gen)
    nan = float("nan")
    ybar = torch.full((C + 2, eng.F), nan, device=dev)   # a guard row on either side
    lbar = torch.full((C + 2,), nan, device=dev)
    state = {"ydrop": y.to(dev)}
    out = eng.rep_mean(state, logits.to(dev), ybar=ybar[1:C + 1], lbar=lbar[1:C + 1])
    only = eng.rep_mean(state)                           # without logits: ybar alone
    torch.cuda.synchronize()
    assert out[0].data_ptr() == ybar[1:].data_ptr() and only[1] is None
    assert bool(torch.isnan(ybar[0]).all() and torch.isnan(ybar[-1]).all() and torch.isnan(lbar[0]) and torch.isnan(lbar[-1])), "wrote outside"
    yr, lr, yb, lb = RO.rep_mean(y, logits, rep, eng.F)
    r = D.Report()
    r.check("ybar", ybar[1:C + 1].cpu(), yr, yb)
    r.check("lbar", lbar[1:C + 1].cpu(), lr, lb)
    print(f"[retrieval] rep_mean C={C} R={rep} {shape}-{dtype}: " + "  ".join(f"{k} {v:.3f}" for k, v in r.ratio.items()))
    assert not r.failed, r.failed
    assert same_bits(only[0], ybar[1:C + 1])


# ------------------------------------------------------------------------------------------------ 2. gic_match_ranks
def _ranks(E, dev, S, bias, N, ld):
    buf = torch.full((N + 1, ld), float("nan"))          # a row beyond N and the columns beyond N: never part of a count
    buf[:N, :N] = S
    buf[:N, N:] = float("inf")
    c2i, i2c = E.match_ranks(buf.to(dev), None if bias is None else bias.to(dev), N=N)
    torch.cuda.synchronize()
    return c2i.cpu().long(), i2c.cpu().long()


@pytest.mark.parametrize("N", [1, 2, 37, 130, 300])          # 300: a second tile of 256 columns
def test_match_ranks_equal_the_integer_oracle(E, dev, N):
    gen = torch.Generator().manual_seed(SEED + N)
    S = torch.randn(N, N, generator=gen)
    S += 1.5 * torch.eye(N)                               # a D that has learned something: ranks spread over 0 .. N-1
    bias = torch.randn(N, generator=gen)
    for ld, b in ((N, None), (N + 3, bias), (N, bias)):
        c2i, i2c = _ranks(E, dev, S, b, N, ld)
        rc, ri = RO.ranks_exact(S, b)
        assert torch.equal(c2i, rc) and torch.equal(i2c, ri), f"N={N} ld={ld} bias={b is not None}"
    if N > 2:
        assert len(set(c2i.tolist())) > 2


@pytest.mark.parametrize("N", [2, 37, 130, 300])
def test_match_ranks_ties_duplicates_and_nan(E, dev, N):
    gen = torch.Generator().manual_seed(SEED + 7 * N)
    bias = torch.randn(N, generator=gen)
    # all equal: every comparison is a tie, every rank N - 1 (the bias is per row, so column ranks are not ties there: without it)
    for got in _ranks(E, dev, torch.full((N, N), 0.25), None, N, N):
        assert got.tolist() == [N - 1] * N
    c2i, _ = _ranks(E, dev, torch.full((N, N), 0.25), bias, N, N + 1)
    assert c2i.tolist() == [N - 1] * N
    # duplicated columns (two images with one q row) and rows (two captions with one ybar): they tie exactly, and a tie counts against
    S = torch.randn(N, N, generator=gen)
    a, b = 0, N - 1
    S[:, b] = S[:, a]
    S[N // 2] = S[0] if N > 2 else S[N // 2]
    S[5 % N, 3 % N] = float("nan")
    c2i, i2c = _ranks(E, dev, S, bias, N, N)
    rc, ri = RO.ranks_exact(S, bias)
    assert torch.equal(c2i, rc) and torch.equal(i2c, ri)
    assert int(c2i[a]) >= 1 and int(c2i[b]) >= 1          # each twin image ties with the other
    assert int(c2i[5 % N]) >= 1 or 5 % N == 3 % N         # the NaN counts against its row ...
    assert int(i2c[3 % N]) >= 1 or 5 % N == 3 % N         # ... and its column


def test_ranks_and_means_same_bits_in_and_out_of_deterministic_mode(E, dev, monkeypatch):
    monkeypatch.setenv("GIC_DISC_FP_ALIGN", "8")
    N, rep = 130, 3
    eng = E.DiscEngine(V, rep, rep, [2, 3], [9, 6], E.DTYPE_BY_NAME["bf16"])
    gen = torch.Generator().manual_seed(SEED + 99)
    y = torch.randn(5 * rep, eng.Fp, generator=gen).to(torch.bfloat16)
    y[:, eng.F:] = 0
    logits = torch.randn(5 * rep, generator=gen).to(dev)
    S, bias = torch.randn(N, N, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)
    runs = []
    for det in (True, True, False):
        E.set_deterministic(det)
        try:
            yb, lb = eng.rep_mean({"ydrop": y.to(dev)}, logits)
            c2i, i2c = E.match_ranks(S, bias)
            torch.cuda.synchronize()
        finally:
            E.set_deterministic(False)
        runs.append((yb.cpu(), lb.cpu(), c2i.cpu(), i2c.cpu()))
    for other in runs[1:]:
        assert same_bits(runs[0][0], other[0]) and same_bits(runs[0][1], other[1])
        assert torch.equal(runs[0][2], other[2]) and torch.equal(runs[0][3], other[3])


# ------------------------------------------------------------------------------------------------ 3. evaluate_retrieval end to end
R = 4


def _instructor(n_items=37, batch=8, seed=17, **kw):
    from gan_image_captioning_amd.args import default_args
    from gan_image_captioning_amd.tasks import SyntheticCaptionData
    from gan_image_captioning_amd.training import GANInstructor
    base = dict(vocab_size=64, gen_embed_dim=32, gen_hidden_dim=64, gen_num_layers=1, compute_dtype="fp32", image_size=64, conditional_gan=1,
                encoder_arch="resnet18", max_seq_len=8, adv_eval_batch_size=batch, adv_train_batch_size=batch, num_workers=0,
                disc_embed_dim=R, disc_num_rep=R, disc_filter_sizes=[2, 3], disc_num_filters=[24, 16], disc_cond="projection", device="cuda",
                log_file=None, model_dir=None, save_dir=None)
    base.update(kw)
    args = default_args(**base)
    torch.manual_seed(seed)
    ds = SyntheticCaptionData(n_items, 64, image_size=64, caption_len=8)
    inst = GANInstructor(args, ds, ds)
    if inst.disc.cond == "projection":
        with torch.no_grad():
            for p in inst.disc.parameters():
                p.mul_(4.0)                              # scores that differ between pairs by more than rounding
    spread(inst.gen)                                     # a trunk under which images differ (tests/rerank_cases.py)
    inst.gen.eval()
    inst.disc.eval()
    return inst


def _capture(inst):
    """Record what evaluate_retrieval's kernels wrote per batch: q (img_proj_fwd), ydrop and the base logits (the forward-only D pass)."""
    den = inst.disc.engine()
    got = {"q": [], "y": [], "logits": [], "fwd": 0, "proj": 0, "mean": 0}
    fwd, proj, mean = den.fwd, den.img_proj_fwd, den.rep_mean

    def fwd_spy(*a, **k):
        assert k.get("forward_only") is True and k.get("cond") is None
        logits, st = fwd(*a, **k)
        got["y"].append(st["ydrop"].clone())
        got["logits"].append(logits.clone())
        got["fwd"] += 1
        return logits, st

    def proj_spy(*a, **k):
        q, pooled = proj(*a, **k)
        got["q"].append(q.clone())
        got["proj"] += 1
        return q, pooled

    def mean_spy(*a, **k):
        got["mean"] += 1
        return mean(*a, **k)
    den.fwd, den.img_proj_fwd, den.rep_mean = fwd_spy, proj_spy, mean_spy
    return got


@pytest.fixture(scope="module")
def inst37():
    return _instructor()


@pytest.mark.parametrize("max_items", [30, None])
def test_evaluate_retrieval_ranks_lie_in_their_intervals(E, dev, inst37, max_items, monkeypatch):
    inst = inst37
    den = inst.disc.engine()
    saved = (den.fwd, den.img_proj_fwd, den.rep_mean)
    got = _capture(inst)
    ranks = {}
    real = E.match_ranks
    monkeypatch.setattr(E, "match_ranks", lambda S, b=None, N=None: ranks.setdefault("r", real(S, b, N)))
    seen = []
    inst.writer.add_scalar = lambda tag, v, step: seen.append(tag)
    try:
        out = inst.evaluate_retrieval("val", max_items=max_items)
    finally:
        den.fwd, den.img_proj_fwd, den.rep_mean = saved
    N = 37 if max_items is None else max_items
    batches = -(-N // 8)
    assert out["n"] == N and (got["fwd"], got["proj"], got["mean"]) == (batches,) * 3
    assert set(out["c2i"]) == set(out["i2c"]) == {"r1", "r5", "r10", "medr", "meanr"}
    assert {f"Retr_{d}_{m}_val" for d in ("c2i", "i2c") for m in ("R1", "R5", "R10", "MedR", "MeanR")} <= set(seen)
    y, logits, q = torch.cat(got["y"]).cpu(), torch.cat(got["logits"]).cpu(), torch.cat(got["q"]).cpu()
    assert y.shape[0] == N * R and q.shape == (N, den.F) and got["y"][-1].shape[0] == (N - 8 * (batches - 1)) * R      # the ragged last batch
    ybar, lbar, yb, lb = RO.rep_mean(y, logits, R, den.F)
    T, bound = RO.pair_scores(ybar, lbar, q, yb, lb)
    iv = RO.rank_intervals(T, bound)
    c2i, i2c = (t.cpu().long() for t in ranks["r"])
    wide = 0
    for name, gpu in (("c2i", c2i), ("i2c", i2c)):
        lo, hi = iv[name]
        assert bool(((lo <= gpu) & (gpu <= hi)).all()), f"{name}: a rank outside its interval: {gpu.tolist()} lo {lo.tolist()} hi {hi.tolist()}"
        wide = max(wide, int((lo != hi).sum()))
        best, worst = RO.summary(lo.tolist()), RO.summary(hi.tolist())
        for k in ("r1", "r5", "r10"):
            assert worst[k] <= out[name][k] <= best[k], (name, k)
        for k in ("medr", "meanr"):
            assert best[k] <= out[name][k] <= worst[k], (name, k)
        assert out[name] == RO.summary(gpu.tolist())
        assert len(set(gpu.tolist())) > 3, "every item has the same rank: the test shows nothing"
    assert 10 * wide <= N, f"{wide} of {N} items have lo != hi"
    print(f"[retrieval] evaluate_retrieval N={N}: items with lo != hi {wide}; c2i {out['c2i']}; i2c {out['i2c']}")


class _Shard:
    """A loader as one rank of a data-parallel run sees it: the dataset is longer than what the sampler, and the loader, yield."""

    def __init__(self, loader, announced, given):
        self.dataset, self.sampler, self._loader, self._given = loader.dataset, range(announced), loader, given

    def __iter__(self):
        n = 0
        for images, captions, *rest in self._loader:
            k = min(captions.shape[0], self._given - n)
            if k <= 0:
                return
            yield (images[:k], captions[:k], *rest)
            n += k


def test_evaluate_retrieval_sizes_itself_from_what_the_loader_yields(dev, inst37):
    keep = inst37.adv_eval_loader
    inst37.writer.add_scalar = lambda *a, **k: None
    try:
        inst37.adv_eval_loader = _Shard(keep, 19, 19)         # 37 items in the dataset, this rank's shard has 19
        assert inst37.evaluate_retrieval("val", max_items=30)["n"] == 19
        assert inst37.evaluate_retrieval("val", max_items=10)["n"] == 10
        inst37.adv_eval_loader = _Shard(keep, 19, 11)         # a loader that ends early: the items seen are ranked
        out = inst37.evaluate_retrieval("val")
        assert out["n"] == 11 and out["c2i"]["r10"] >= 10 / 11
        whole = inst37.evaluate_retrieval("val", max_items=11)
    finally:
        inst37.adv_eval_loader = keep
    assert whole["n"] == 11 and whole["c2i"] == out["c2i"] and whole["i2c"] == out["i2c"]


def test_eval_retrieval_flag_calls_it_from_the_epoch_loop(dev):
    inst = _instructor(n_items=10, batch=4, eval_retrieval=1, eval_retrieval_items=7, adv_epochs=1, pretrain_epochs=0)
    calls = []
    real = inst.evaluate_retrieval
    inst.evaluate_retrieval = lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1]
    inst.adv_loop = lambda what: (0.0, 0.0)               # the flag's dispatch is under test, not the adversarial steps
    inst._run()
    assert calls == [(("val",), {"max_items": 7})]
    off = _instructor(n_items=10, batch=4, adv_epochs=1, pretrain_epochs=0)
    off.evaluate_retrieval = lambda *a, **k: calls.append("off")
    off.adv_loop = lambda what: (0.0, 0.0)
    off._run()
    assert len(calls) == 1


def test_evaluate_retrieval_refusals(dev, inst37):
    with pytest.raises(ValueError, match="--disc-cond projection"):
        _instructor(n_items=4, batch=4, disc_cond="none").evaluate_retrieval("val")
    inst37.args.captions_per_image = 5
    try:
        with pytest.raises(ValueError, match="captions-per-image"):
            inst37.evaluate_retrieval("val")
    finally:
        inst37.args.captions_per_image = 1

    class Big:
        dataset = range(9000)
    keep, inst37.adv_eval_loader = inst37.adv_eval_loader, Big()
    try:
        with pytest.raises(ValueError, match="8192"):
            inst37.evaluate_retrieval("val")
    finally:
        inst37.adv_eval_loader = keep
