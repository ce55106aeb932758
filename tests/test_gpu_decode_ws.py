"""What every caption-decode head (csrc/decode.hip) writes, reads and leaves behind, on the GPU: every case of
tests/decode_ws_cases.py through the engine wrappers as they are, inside the Harness of tests/decode_ws.py -- banded workspaces of
exactly ``*_ws_bytes`` bytes, banded pre-filled outputs, banded inputs -- on three prior contents of the workspaces: zeros, what a
finished twin search left, typed poison.  After each call: bands intact, inputs and weights bit-equal, no pre-fill left in an
output, tokens / lengths / scores legal; the run on zeros against the head's float64 oracle under the head's own criterion (f32); the
two other runs bit-identical to it."""
import pytest
import torch

from tests import decode_ws as W
from tests import decode_ws_cases as WC
from tests import forced_beam_oracle as FO
from tests.test_decode_ws import case_layouts, case_poison

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _engines(d, dt, n):
    from gan_image_captioning_amd import engine
    if d.attn:
        return [engine.AttnDecoderEngine(d.V, d.E, d.H, d.C, d.P, d.A, dt) for _ in range(n)]
    return [engine.DecoderEngine(d.V, d.E, d.H, d.NL, dt) for _ in range(n)]


class _Side:
    """One problem of a case on the device: its own engines (one engine holds one set of weight images), banded inputs, watched
    weights, and ``run(ws=None)``: the head through the engine wrappers."""

    def __init__(self, h, tag, case, dt, pb, dev):
        d, K = WC.MODELS[case.model]
        head = WC.HEADS[case.head]
        act = torch.bfloat16 if dt == W.BF16 else torch.float32
        engs = _engines(d, dt, len(pb.members))
        params = [[h.watch(f"{tag} member {m} weight {i}", t.to(dev)) for i, t in enumerate(p)] for m, p in enumerate(pb.members)]
        feats = [h.put(f"{tag} features {m}", f) for m, f in enumerate(pb.feats)]
        fmaps = [h.put(f"{tag} feature map {m}", f.to(act)) for m, f in enumerate(pb.fmaps)] if d.attn else None
        maps = (fmaps[0],) if d.attn else ()
        kw = dict(head.cons) if head.cons is not WC.C_OFF else {}
        if head.alphas:
            kw["want_alphas"] = True
        eng = engs[0]
        if head.kind == "beam" and head.groups > 1:
            self.run = lambda ws=None: eng.diverse_beam_search(params[0], feats[0], *maps, d.L, K, head.groups, head.diversity, length_penalty=head.lp,
                                                               ws=ws, **kw)
        elif head.kind == "beam":
            self.run = lambda ws=None: eng.beam_search(params[0], feats[0], *maps, d.L, K, length_penalty=head.lp, ws=ws, **kw)
        elif head.kind == "forced":
            force = h.put(f"{tag} force words", pb.force)
            self.run = lambda ws=None: eng.beam_search(params[0], feats[0], *maps, d.L, K, length_penalty=head.lp, force_words=force, ws=ws, **kw)
        elif head.kind == "sample":
            draw = dict(seed=pb.seed) if head.philox else dict(noise_u=h.put(f"{tag} noise_u", pb.noise_u))
            self.run = lambda ws=None: eng.sample_captions(params[0], feats[0], *maps, d.L, K, top_k=head.top_k, top_p=head.top_p, ws=ws, **draw, **kw)
        elif head.kind == "ens-beam":
            self.run = lambda ws=None: eng.ensemble_beam_search(list(zip(engs, params)), feats, fmaps, d.L, K, None, head.mode, ws=ws)
        else:
            noise = h.put(f"{tag} noise_u", pb.noise_u)
            self.run = lambda ws=None: eng.ensemble_sample_captions(list(zip(engs, params)), feats, fmaps, d.L, K, None, head.mode,
                                                                    top_k=head.top_k, top_p=head.top_p, noise_u=noise, ws=ws)
        self.engs = engs


def _against_oracle(case, what, got, pb):
    """Check 4: the criterion and the tolerances of the head's own GPU test (named at each branch), on every image or row."""
    d, K = WC.MODELS[case.model]
    head = WC.HEADS[case.head]
    want = WC.oracle(case)
    if head.kind == "forced":          # tests/test_gpu_forced_beam.py::test_f32_matches_oracle
        W.compare_forced(what, got, want, pb.force.tolist(), K, WC.PAD, FO.absent_mask, want[5] if head.alphas else None)
    elif head.kind == "beam":
        if head.cons is not WC.C_OFF or head.groups > 1:          # tests/test_gpu_diverse_beam.py::_compare, test_gpu_constrained.py
            rtol, atol = 1e-4, 1e-5
        elif d.attn:                   # tests/test_gpu_attn_beam.py::_check_vs_oracle
            rtol, atol = 1e-4, 1e-6
        else:                          # tests/test_gpu_beam.py::_check_vs_oracle
            rtol, atol = 1e-5, 1e-6
        al = (got["alphas"], want[3]) if head.alphas else (None, None)
        W.compare_beam(what, got, want[:3], want[-1], K, head.groups, rtol, atol, *al)
    elif head.kind == "ens-beam":      # tests/test_gpu_ensemble.py::compare
        W.compare_beam(what, got, want[:3], want[-1], K, 1, 1e-5, WC.ensemble_atol(case, pb.members))
    elif head.kind == "ens-sample":    # tests/test_gpu_ensemble.py::test_sampling_matches_oracle
        W.compare_rows(what, got, want, WC.ensemble_atol(case, pb.members))
    else:                              # tests/test_gpu_sample.py::test_lstm_f32_matches_oracle, test_gpu_constrained.py
        W.compare_rows(what, got, want, 1e-4)


@pytest.mark.parametrize("dt", [W.F32, W.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_head_keeps_the_workspace_contract(dev, case, dt):
    from gan_image_captioning_amd import engine
    d, K = WC.MODELS[case.model]
    head = WC.HEADS[case.head]
    what = f"{case.id} ({'bf16' if dt else 'f32'})"
    extra = []
    if head.alphas:
        extra.append(((d.B, K, d.L, d.P), torch.float32))
    if head.kind == "forced":
        extra.append(((d.B, K), torch.int32))
    h = W.Harness(engine, dev, W.OutSpec(d.V, d.L, WC.PAD, dead_ok=head.kind == "forced"), extra)
    pb = WC.problem(case)
    main, twin = _Side(h, "the call's", case, dt, pb, dev), _Side(h, "the twin's", case, dt, WC.problem(case, twin=True), dev)
    fused_rows = 0 if d.attn else main.engs[0].fused_rollout_rows()
    assert W.is_fused(d, K, fused_rows) == (d.attn or (d.V == 68 and d.B * K <= 512)), fused_rows
    got = W.run_priors(h, what, main.run, twin.run, case_poison(case, dt, fused_rows))
    lay = case_layouts(case, dt, fused_rows)
    assert [b.nbytes for b in h.ws] == [l[1] for l in lay if l is not None], what          # the workspaces the head asked for
    assert set(got) == {"ids", "scores", "lengths"} | ({"alphas"} if head.alphas else set()) | ({"met"} if head.kind == "forced" else set())
    live = got["lengths"][got["lengths"] > 0]
    if case.term == "ends":            # the launches after the last image finished ran on a finished state
        assert int(live.max()) < d.L, f"{what}: lengths {got['lengths'].tolist()}"
    elif dt == W.F32:
        assert bool((live == d.L).all()), f"{what}: lengths {got['lengths'].tolist()}"
    if dt == W.F32:
        _against_oracle(case, what, got, pb)


@pytest.mark.parametrize("model", ["lstm1", "generic", "attn"])
@pytest.mark.parametrize("head", ["beam-lp0", "cbeam", "forced", "sample-seed-k5", "ens-beam"])
def test_a_reused_caller_workspace_gives_the_fresh_call(dev, model, head):
    """``ws=`` as callers use it, through the engine's own ``_aligned_ws``: one banded buffer of ``ws_bytes`` bytes goes through a
    finished search on other weights and then through the call, which returns the bits of the same call on a workspace of its own."""
    from gan_image_captioning_amd import engine
    case = WC.Case(model, head, "runs")
    d, K = WC.MODELS[model]
    h = W.Harness(engine, dev, W.OutSpec(d.V, d.L, WC.PAD))          # (places the inputs; no call goes through its substitutes)
    main, twin = _Side(h, "the call's", case, W.F32, WC.problem(case), dev), _Side(h, "the twin's", case, W.F32, WC.problem(case, twin=True), dev)
    fused_rows = 0 if d.attn else main.engs[0].fused_rollout_rows()
    ws = W.Banded(case_layouts(case, W.F32, fused_rows)[0][1], dev, "the caller's workspace")
    used, real = [], engine._aligned_ws

    def spy(buf, n, dv):
        out = real(buf, n, dv)
        if buf is not None:
            used.append(out.data_ptr())
        return out

    fresh = main.run()
    engine._aligned_ws = spy
    try:
        twin.run(ws.live)
        again = main.run(ws.live)
    finally:
        engine._aligned_ws = real
    torch.cuda.synchronize()
    assert used == [ws.live.data_ptr()] * 2, f"{case.id}: the searches did not run in the caller's workspace"
    assert ws.breach() is None, f"{case.id}: a write outside the caller's workspace: {ws.breach()}"
    assert len(fresh) == len(again)
    for a, b in zip(fresh, again):
        assert torch.equal(a, b), f"{case.id}: the call on a reused workspace differs from the call on its own"
