"""The long-search cases of tests/search_cases.py, on the float64 oracles alone (no GPU): what makes each case worth running on the
device.  These are conditions on the reference; a case that misses one gets another seed or <E> bias, never a lower floor."""
import pytest

from tests import search_cases as S


def test_the_table_covers_every_search_of_every_problem():
    problems = list(S.LSTM_PROBLEMS) + list(S.ATTN_PROBLEMS)
    assert problems == ["generic", "fused1", "fused2", "attn", "wide"]
    assert len(S.CASES) == len(S.TABLE) == len(problems) * len(S.SEARCHES) == 60
    assert {c[:2] for c in S.CASES} == {(p, s) for p in problems for s in S.SEARCHES}
    # the attention problems: ORACLE_SHAPE's and WIDE_SHAPE's dimensions (tests/test_gpu_attn_beam.py), L = 10
    assert S.ATTN_PROBLEMS["attn"][1:] == (10, 64, 16, 32, 40, 49, 24) and S.ATTN_PROBLEMS["wide"][1:] == (10, 64, 8, 16, 136, 70, 264)
    assert {s[1:] for s in S.PLAIN} == {(k, a) for k in (2, 3, 5, 8) for a in (0.0, 0.7)}
    assert [s[1:] for s in S.DIVERSE] == [(4, 2, 1.0), (6, 3, 2.0), (8, 4, 0.5), (8, 8, 0.7)]
    for name, (B, L, V, E, H, NL) in S.LSTM_PROBLEMS.items():
        assert (B, L, E, H) == (16, 12, 8, 16)
        # the fused step kernels take V % 4 == 0, E % 8 == 0, H % 8 == 0 (gicap.h); V = 68 is one full tile and a ragged tile of 4
        assert (V, V % 4 == 0) == ((50, False) if name == "generic" else (68, True))


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_case_is_eligible(case):
    name, search, seed, bias, comparable, steps = case
    B, L = S.shape(name)[:2]
    k = search[1]
    e = S.eligibility(name, search, seed, bias)
    print(f"{S.case_id(case)}: {e}")
    assert e["comparable"] == comparable, "the table records the number of comparable images"
    assert e["compared_steps"] == steps, "and the number of search steps those images ran"
    assert 4 * e["comparable"] >= 3 * B, "at least 3/4 of the images have a selection margin >= 1e-4"
    assert e["mean_len"] >= L / 2, "the mean caption length is >= L / 2"
    assert e["mixed"] >= 1, "an image holds a beam that finished before step L - 3 beside one that ran to L without <E>"
    assert e["early"] >= 1 and e["late"] >= 1, "an image finishes entirely before L while another does not"
    if S.groups_of(search) < k:
        assert e["moved"] >= 1, "at some step t >= 2 the chosen parents are not the identity permutation"
    else:
        assert e["moved"] == 0                             # one beam per group: its parent is itself, at every step
    assert e["tokens"] >= 20, ">= 20 distinct tokens are returned over the batch"
    assert S.eligible(name, search, e)


def test_trace_matches_the_returned_beams():
    """The parent trace the oracles report is the one their outputs were built from: an image's trace has one entry per step that
    ran, and the steps that ran are those up to the image's longest beam."""
    for case in (S.CASES[0], S.CASES[7], S.CASES[len(S.SEARCHES) + 9], S.CASES[-1]):
        name, search, seed, bias = case[:4]
        r = S.oracle(name, search, seed, bias)
        for b, pars in enumerate(r["trace"]):
            assert len(pars) == int(r["lengths"][b].max()), (S.case_id(case), b)      # (a beam that never ends has length L)
            assert all(len(p) == search[1] and set(p) <= set(range(search[1])) for p in pars)
