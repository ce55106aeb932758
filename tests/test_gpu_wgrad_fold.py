"""The backward pass's folded launches (csrc/gemm.hip's weight-gradient extras, csrc/decoder.hip, csrc/disc.hip), at the smallest shapes
at which each new path can go wrong, through DecoderEngine.sample_bwd / DiscEngine.bwd with caller-owned, guarded buffers exactly as
tests/test_gpu_decoder_stages.py and tests/test_gpu_disc_stages.py drive them (their helpers and the fp64 references and derived bounds of
tests/decoder_cases.py / tests/disc_cases.py are used by import):

  * the bias gradients d_b_out, d_b_ih / d_b_hh and the highway's hw_b as column sums of the A operand of the weight-gradient product that
    streams that matrix anyway (GemmDesc.a_sum / a_sum2);
  * dW_ih | dW_hh of a layer as ONE product over xh = [x | h] with two output matrices (GemmDesc.C2 / n_split), where din sits on a tile
    boundary, and the two products as before where it does not;
  * split-K over all of that: f32 atomics into C, C2 and both bias sums over the one zero-fill launch;
  * no zero fill of dc in front of the fused BPTT chain (LstmBwdStepArgs.dc_zero): dc holds NaN before every call here;
  * the row-wise embedding scatter: colliding rows, and ids outside [0, V) in the buffer the backward reads (the forward stores its
    tokens clamped, so the test overwrites entries of the caller-owned ids buffer between forward and backward: the teacher-forced
    backward hands the same kernel a caller's captions).
Which route ran is read from gic_debug_wgrad_launches before and after every backward: the output layer's fold is one launch of the
folding form, a layer whose din is a multiple of the tile adds one launch with two output matrices, any other layer none.
The folds exist in bf16 compute mode; the f32 parity mode keeps the separate launches at every site (tests/test_wgrad_fold_select.py) and
runs here for what is common to both modes: dc_zero, the scatter, and the same checks on the launches it keeps.

Every stage is held to the bound decoder_cases / disc_cases derive for it from the kernel's own upstream buffers.  Each folded bias
gradient is also compared with gic_colsum of the same buffer: two f32 sums of the same K numbers in different orders, held to the
reordering bound K 2^-24 sum |a| per column (computed here; the largest ratio is printed).  In deterministic mode every site keeps
the launches it had: d_b_ih == d_b_hh bit for bit, two runs bit-identical."""
import ctypes

import pytest
import torch

from gan_image_captioning_amd import _lib as L
from tests import decoder_cases as D
from tests import disc_cases as DC
from tests import test_gpu_decoder_stages as S
from tests import test_gpu_disc_stages as SD
from tests.decoder_cases import Case, TD, U

pytestmark = pytest.mark.gpu


def _both(name, B, L_, V, E, H, NL, **kw):
    return [Case(name, B, L_, V, E, H, NL, dt, "", **kw) for dt in ("f32", "bf16")]


CASES = (
    # K = B L = 15: one ragged K tile; 4H = 160: a ragged M tile; din = E = 64 on a tile boundary: the merged two-matrix launch
    _both("merge", 3, 5, 72, 64, 40, 1)
    # din = 72 is off a tile boundary: the two products and the column-sum pass, as before
    + _both("offtile", 3, 5, 72, 72, 64, 1)
    # K = 540: 9 K tiles (bf16) over 6 tiles of 64 x 64: split-K four ways, atomics into C, C2 and both bias sums over the zero fill
    + _both("splitk", 27, 20, 72, 64, 40, 1)
    # two layers: layer 1 has din = H = 40 (the fallback), layer 0 merges
    + _both("nl2", 3, 5, 72, 64, 40, 2)
    # V = 8 over 18 scattered rows: many rows share a token; the backward reads ids of -1, V and V + 5 (RAW_IDS) and clamps them
    + _both("collide", 6, 4, 8, 64, 40, 1, force=True)
)
RAW_IDS = {(0, 0): -1, (2, 1): 8, (4, 2): 13, (5, 0): -6}          # (b, t) -> id, t <= L - 2: rows the scatter reads; V = 8
# layers that take the one-product launch with two output matrices, in bf16 mode (din % 64 == 0); the f32 mode folds nothing
MERGED_LAYERS = {"merge": 1, "offtile": 0, "splitk": 1, "nl2": 1, "collide": 1}


def wgrad_launches():
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    L.load().gic_debug_wgrad_launches(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def note(tag, rep):
    """Print a report's ratios and fail on any flagged stage (nothing is recorded in another module's tables)."""
    print(f"[wgrad fold] {tag}: " + "  ".join(f"{s} {r:.3f}" for s, r in rep.ratio.items() if r > 0))
    assert not rep.failed, f"{tag}: {rep.failed}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E():
    from gan_image_captioning_amd import engine
    return engine


def gpu_colsum(a, dtype, dev):
    """gic_colsum of a [rows, cols] CPU tensor (the bits a kernel left), on the GPU."""
    rows, cols = a.shape
    a = a.contiguous().to(dev)
    out = torch.full((cols,), float("nan"), device=dev)
    L.check(L.load().gic_colsum(a.data_ptr(), S.DT[dtype], cols, rows, cols, out.data_ptr(), 0, None), "gic_colsum")
    torch.cuda.synchronize()
    return out.cpu()


def assert_reordered(what, got, a, dtype, dev, base=None):
    """`got` (- base) against gic_colsum(a) within K 2^-24 sum |a| per column (+ the rounding of the accumulation onto `base`)."""
    K = a.shape[0]
    ref = gpu_colsum(a, dtype, dev).double()
    bound = K * U * a.double().abs().sum(0)
    diff = got.double().reshape(-1) - ref
    if base is not None:
        diff = diff - base.double().reshape(-1)
        bound = bound + 2 * U * (base.double().reshape(-1).abs() + ref.abs())
    worst = float((diff.abs() / bound.clamp_min(1e-300)).max())
    print(f"[wgrad fold] {what}: |folded - colsum| / (K u sum|a|) = {worst:.4f}")
    assert bool((diff.abs() <= bound).all()), f"{what}: {worst:.3f} of the reordering bound"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_decoder_backward_folds(E, dev, case):
    c, NL = case, case.NL
    P, X = D.data(case)
    eng = S.make_engine(E, case)
    params = [p.to(dev) for p in P]
    g = S.alloc_state(case, dev)
    S.forward(eng, case, params, X, g, dev)
    S.assert_guards(case, g)
    img = S.shadow_cpu(eng)
    if img["wout"] is None:
        img["wout"] = P[-2]
    st = S.state_cpu(case, g)
    assert D.select(case)["bwd"] == "fused"
    if case.name == "collide":
        assert D.repeats(st["ids"], c.L) >= 8, "the scattered rows must collide"
        # ids outside [0, V) where the scatter reads them: only the scatter looks at ids in the backward, and the reference
        # (decoder_cases.run_backward) forms d_embed from the clamped ids
        for (b, t), v in RAW_IDS.items():
            g["ids"].view[b, t] = v
            st["ids"][b, t] = v
        torch.cuda.synchronize()
        assert int(((st["ids"][:, :c.L - 1] < 0) | (st["ids"][:, :c.L - 1] >= c.V)).sum()) == len(RAW_IDS)
    # deterministic mode off: dc holds NaN before the call (alloc_bwd), sentinel rows are checked by S.backward
    n0 = wgrad_launches()
    w, grads = S.backward(E, eng, case, params, P, X, g, dev)
    n1 = wgrad_launches()
    bf = case.dtype == "bf16"
    assert (n1[0] - n0[0], n1[1] - n0[1]) == ((1 + MERGED_LAYERS[case.name], MERGED_LAYERS[case.name]) if bf else (0, 0)), \
        f"{case.id}: folded / two-matrix launches {n1[0] - n0[0]} / {n1[1] - n0[1]}"
    for t in grads:
        assert bool(torch.isfinite(t).all()), f"{case.id}: a gradient is not finite"
    rep = D.Report()
    D.run_backward(case, P, img, X, st, w, grads, rep)
    assert {"d_w_out", "d_b_out", "dc", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "d_embed"} <= set(rep.ratio)
    note(case.id, rep)
    BL = c.B * c.L
    assert_reordered(f"{case.id} d_b_out", grads[2 + 4 * NL], w["dlogits"].reshape(BL, c.V), case.dtype, dev)
    for l in range(NL):
        a = w["dgates"][l].reshape(BL, 4 * c.H)
        assert_reordered(f"{case.id} d_b_ih[{l}]", grads[3 + 4 * l], a, case.dtype, dev)
        assert_reordered(f"{case.id} d_b_hh[{l}]", grads[4 + 4 * l], a, case.dtype, dev)
    # deterministic mode: the parent's launches; d_b_ih == d_b_hh exactly (run_backward, det=True), two runs bit-identical
    runs = []
    for _ in range(2):
        wd, gd = S.backward(E, eng, case, params, P, X, g, dev, det=True)
        assert wgrad_launches() == n1, f"{case.id}: the deterministic mode launched the folding form"
        repd = D.Report()
        D.run_backward(case, P, img, X, st, wd, gd, repd, det=True)
        assert {"d_embed", "d_b_ih == d_b_hh"} <= set(repd.ratio)
        note(case.id + " det", repd)
        runs.append(gd)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{case.id}: two deterministic runs differ"


# B = 2, L = 6, V = 24, R = De = 3 and two filter widths (the smallest the engine's tests drive: disc_cases' det-cap3 with two captions)
DISC = DC.Case("hwb", 2, 6, 3, 3, (2, 3), (24, 16), "bf16", "mfma", "small1", "lds", exact=False, V=24)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_disc_highway_bias_fold(E, dev, accumulate, monkeypatch):
    case = DISC
    gen = torch.Generator().manual_seed(SD.ROUND_SEED + int(accumulate))
    P = DC.make_params(case, "rounding", gen)
    X = DC.make_inputs(case, gen, soft=False, train=True)
    eng = SD.make_engine(E, case, monkeypatch)
    params = [p.to(dev) for p in P]
    g = SD.alloc_state(case, dev)
    SD.forward(eng, case, params, X, g, dev)
    SD.assert_guards(case, g)
    img = SD.shadow_cpu(eng)
    if img["emb"] is None:
        img["emb"] = P[0]
    st = SD.cpu(g)
    n0 = wgrad_launches()
    w, grads, G0, _ = SD.backward(E, eng, case, params, P, X, g, dev, True, False, accumulate, gen)
    n1 = wgrad_launches()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 0), "the highway weight gradient did not take the folding form"
    rep = DC.Report()
    DC.run_backward(case, P, img, X, st, SD.cpu(w), grads, G0, None, rep)
    assert any(k.split(".")[0] == "hw_b" for k in rep.ratio), sorted(rep.ratio)
    note(case.id, rep)
    i_hw_b = 1 + 2 * len(case.fs) + 1
    assert tuple(P[i_hw_b].shape) == (case.F,)
    dh = SD.cpu(w)["dh"][:, :case.F]
    assert_reordered(f"{case.id} hw_b {'accumulate' if accumulate else 'overwrite'}", grads[i_hw_b], dh, case.dtype, dev,
                     base=G0[i_hw_b] if accumulate else None)
