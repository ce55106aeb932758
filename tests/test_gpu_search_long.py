"""Searches that run long, on the GPU against the float64 oracles: the cases of tests/search_cases.py, which tests/test_search_cases.py
shows to mix finished and live beams for many steps, to reorder their parents past step 2 and to stop image by image.

f32: ids, lengths and scores of every image whose selections the oracle decides by >= 1e-4, compared as tests/test_gpu_beam.py's
_check_vs_oracle and tests/test_gpu_diverse_beam.py's _compare do (in order where the final order is decided by >= 1e-4 too, else as
sets); the number of images compared must be at least the number the case table records.  bf16: the same problems under the existing
invariants -- every score equals the teacher-forced rescoring of its own ids (LSTM: forward_tf, rtol = atol = 1e-2; attention: the
float64 log-probability within 2e-2 |ref| + 0.05 per token: the tolerances of the existing rescoring tests), every group is sorted, PAD
stands behind <E> and behind nothing else, and the attention maps sum to one up to the length and are zero past it (in f32 they are
the oracle's).

Images compared / search steps those images ran in the oracle, per case (the LSTM problems hold 16 images, L = 12, the attention
problems 24, L = 10; a plain search of alpha = 0.7 selects as that of alpha = 0 does); tests/search_cases.py carries the same figures
and both tests assert them:
    generic k2 16/157  k3 16/169  k5 16/165  k8 15/167  k4g2 16/172  k6g3 16/187  k8g4 16/181  k8g8 16/189
    fused1  k2 16/139  k3 16/159  k5 16/169  k8 16/180  k4g2 16/181  k6g3 16/184  k8g4 16/191  k8g8 16/184
    fused2  k2 16/154  k3 16/157  k5 16/181  k8 16/184  k4g2 16/185  k6g3 16/186  k8g4 15/173  k8g8 15/176
    attn    k2 23/188  k3 23/195  k5 24/220  k8 23/224  k4g2 24/220  k6g3 24/235  k8g4 24/220  k8g8 21/208
    wide    k2 24/173  k3 24/185  k5 24/196  k8 24/198  k4g2 24/220  k6g3 24/235  k8g4 24/236  k8g8 23/228"""
import pytest
import torch

from tests import attn_beam_oracle as AO
from tests import search_cases as S
from tests.test_gpu_attn_beam import _check_alphas

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _run(case, dt, dev):
    """(engine, parameters and inputs on the device, outputs): the attention decoder's outputs end with its alphas."""
    from gan_image_captioning_amd import engine
    name, search, seed, bias = case[:4]
    B, L = S.shape(name)[:2]
    k = search[1]
    prob = S.problem(name, seed, bias)
    params, ins = [p.to(dev) for p in prob[0]], [t.to(dev) for t in prob[1:]]
    if name in S.LSTM_PROBLEMS:
        eng, kw = engine.DecoderEngine(*S.shape(name)[2:], dt), {}
        assert eng.beam_fused(B, k) == (name != "generic")
    else:
        eng, kw = engine.AttnDecoderEngine(*S.shape(name)[2:], dt), dict(want_alphas=True)
    if search[0] == "beam":
        out = eng.beam_search(params, *ins, L, k, length_penalty=search[2], **kw)
    else:
        out = eng.diverse_beam_search(params, *ins, L, k, search[2], search[3], **kw)
    torch.cuda.synchronize()
    return eng, params, ins, out


def _group_order(scores, lengths, G, alpha):
    kg = scores.shape[1] // G
    norm = scores.cpu().double() / lengths.cpu().double() ** alpha
    for g in range(G):
        n = norm[:, g * kg:(g + 1) * kg]
        assert (n[:, :-1] >= n[:, 1:] - 1e-6 * n.abs()[:, 1:]).all()


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_f32_matches_oracle(dev, case):
    name, search, seed, bias, comparable, want_steps = case
    B, L = S.shape(name)[:2]
    k, G = search[1], S.groups_of(search)
    alpha = search[2] if search[0] == "beam" else 0.0
    rtol, atol = (1e-5, 1e-6) if search[0] == "beam" else (1e-4, 1e-5)        # (those of _check_vs_oracle / _compare)
    _, _, _, out = _run(case, 0, dev)
    ids, sc, ln = out[0].cpu(), out[1].cpu().double(), out[2].cpu().long()
    assert ids.shape == (B, k, L)
    attn = name in S.ATTN_PROBLEMS
    if attn:
        _check_alphas(out[3], out[2])
        al = out[3].cpu().double()
    _group_order(out[1], out[2], G, alpha)
    ref = S.oracle(name, search, seed, bias)
    rid, rsc, rlen, margins = ref["ids"], ref["scores"], ref["lengths"], ref["margins"]
    kg = k // G
    ok = [b for b, (sel, _) in enumerate(margins) if sel >= 1e-4]
    steps = 0
    for b in ok:
        steps += len(ref["trace"][b])
        for g in range(G):
            s = slice(g * kg, (g + 1) * kg)
            if margins[b][1] >= 1e-4:
                assert torch.equal(ids[b, s], rid[b, s]), (b, g)
                assert torch.equal(ln[b, s], rlen[b, s]), (b, g)
                torch.testing.assert_close(sc[b, s], rsc[b, s], rtol=rtol, atol=atol)
            else:
                assert sorted(zip(ids[b, s].tolist(), ln[b, s].tolist())) == sorted(zip(rid[b, s].tolist(), rlen[b, s].tolist())), (b, g)
                torch.testing.assert_close(sc[b, s].sort().values, rsc[b, s].sort().values, rtol=rtol, atol=atol)
            if attn:                                         # each returned beam's maps are those of the oracle's beam with its ids
                for j in range(g * kg, (g + 1) * kg):
                    r = next(i for i in range(g * kg, (g + 1) * kg) if torch.equal(rid[b, i], ids[b, j]))
                    torch.testing.assert_close(al[b, j], ref["alphas"][b, r], rtol=1e-4, atol=1e-6)
    print(f"{S.case_id(case)}: {len(ok)} of {B} images, {steps} steps compared")
    assert len(ok) >= comparable and steps >= want_steps, \
        f"{len(ok)} images, {steps} steps compared; the case table records {comparable}, {want_steps}"


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_bf16_invariants(dev, case):
    name, search, seed, bias = case[:4]
    B, L = S.shape(name)[:2]
    k, G = search[1], S.groups_of(search)
    alpha = search[2] if search[0] == "beam" else 0.0
    eng, params, ins, out = _run(case, 1, dev)
    ids, scores, lengths = out[:3]
    _group_order(scores, lengths, G, alpha)
    pos = torch.arange(L, device=dev)[None]
    for j in range(k):
        row, n = ids[:, j], lengths[:, j].long()
        assert (n >= 1).all() and (n <= L).all()
        assert (row[pos >= n[:, None]] == S.PAD).all()                                   # PAD behind the caption
        last = row.gather(1, (n - 1)[:, None])[:, 0]
        assert ((last == S.EOS) | (n == L)).all()                                        # which ends with <E> unless it ran to L
        inner = torch.where(pos < (n - 1)[:, None], row, torch.zeros_like(row))
        assert (inner != S.EOS).all()                                                    # and holds no <E> before its end
    if name in S.ATTN_PROBLEMS:
        # (the attention decoder's rescoring tests: the float64 log-probability within 2e-2 |ref| + 0.05 per token)
        _check_alphas(out[3], lengths)
        ref = AO.sequence_logprob(*S.problem(name, seed, bias), ids.cpu(), lengths.cpu())
        got = scores.cpu().double()
        tol = 2e-2 * ref.abs() + 0.05 * lengths.cpu().double()
        assert ((got - ref).abs() <= tol).all(), (got - ref).abs().max()
        return
    for j in range(k):
        row, n = ids[:, j], lengths[:, j].long()
        pred, _ = eng.forward_tf(params, *ins, row[:, :-1].contiguous(), n.cpu(), 1.0, pretrain=True)
        logp = torch.log_softmax(pred.float(), dim=-1)
        T = pred.shape[1]
        lp = logp.gather(2, row[:, :T, None])[..., 0]
        lp = torch.where(pos[:, :T] < n[:, None], lp, torch.zeros_like(lp))
        torch.testing.assert_close(lp.sum(1), scores[:, j], rtol=1e-2, atol=1e-2)
