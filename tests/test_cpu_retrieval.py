"""tt_topk_mips without a GPU: its declared limits come back as status codes before any launch, the
workspace query, metrics.retrieval_metrics on hand-worked cases, and the conditions under which the
fp64 oracle's band rule (tests/retrieval_oracle.py) means something for the GPU cases' inputs."""
import ctypes as C
import math

import pytest
import torch

import retrieval_oracle as ro

FAKE = 1 << 20  # never dereferenced: every call here must return before any launch
F32, BF16 = 2, 3


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd import _lib
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


def _call(lib, M=8, N=100, E=64, k=10, splits=0, q_dtype=F32, c_dtype=F32, ldq=None, ldc=None, queries=FAKE,
          items=FAKE, ids=FAKE, scores=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    rc = lib.tt_topk_mips(queries, q_dtype, E if ldq is None else ldq, items, c_dtype, E if ldc is None else ldc, None,
                          M, N, E, k, splits, ids, scores, ws, ws_bytes, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(E=0), "E must"), (dict(E=16), "E must"), (dict(E=48), "E must"), (dict(E=160), "E must"), (dict(E=-32), "E must"),
    (dict(k=0), "k must"), (dict(k=257), "k must"), (dict(k=-1), "k must"),
    (dict(M=0), "M must"), (dict(M=-5), "M must"),
    (dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(N=-1), "N must"),
    (dict(splits=-1), "splits must"), (dict(splits=65), "splits must"),
    (dict(q_dtype=0), "q_dtype"), (dict(c_dtype=1), "c_dtype"),
    (dict(ldq=63), "ldq"), (dict(ldc=32), "ldc"),
    (dict(queries=None), "null"), (dict(items=None), "null"), (dict(ids=None), "null"), (dict(scores=None), "null"),
    (dict(ws=None), "null"), (dict(ws_bytes=8 * 10 * 8 - 1, splits=1), "ws_bytes"),
])
def test_limits_are_status_codes(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_topk_mips") and word in msg, (kw, msg)


def test_limit_values_exist(lib):
    from two_tower_recommender_model_amd import _lib

    assert _lib.TT_TOPK_MAX_K == 256
    assert "tt_topk_mips" in _lib.COMPUTE_ENTRY_POINTS
    assert lib.tt_num_entry_points() == len(_lib.COMPUTE_ENTRY_POINTS)


def test_workspace_query(lib):
    ws = lib.tt_topk_mips_workspace_bytes
    for S, M, k in [(1, 1, 1), (2, 40, 100), (7, 40, 100), (64, 4096, 256), (3, 129, 17)]:
        assert ws(M, 100000, k, S) == S * M * k * 8
    # splits = 0: the library's choice, between 1 and 64 lists per query, more when M is small
    auto_small, auto_large = ws(16, 1 << 22, 100, 0), ws(1 << 16, 1 << 22, 100, 0)
    assert auto_small % (16 * 100 * 8) == 0 and 1 <= auto_small // (16 * 100 * 8) <= 64
    assert auto_small // (16 * 100 * 8) > auto_large // ((1 << 16) * 100 * 8) >= 1
    assert ws(16, 1, 100, 0) == 16 * 100 * 8  # one item: one split
    for bad in [(0, 100, 10, 1), (8, 0, 10, 1), (8, 1 << 31, 10, 1), (8, 100, 0, 1), (8, 100, 257, 1), (8, 100, 10, 65),
                (8, 100, 10, -1)]:
        assert ws(*bad) == 0, bad


# ---- metrics.retrieval_metrics ------------------------------------------------------------------


def _metrics(pred, targets, k):
    from two_tower_recommender_model_amd.metrics import retrieval_metrics

    vals = torch.tensor([v for t in targets for v in t], dtype=torch.int64)
    offs = torch.tensor([0] + list(torch.tensor([len(t) for t in targets]).cumsum(0)), dtype=torch.int64)
    return retrieval_metrics(torch.tensor(pred, dtype=torch.int64), vals, offs, k)


def _d(rank):
    return 1.0 / math.log2(rank + 1)


def test_retrieval_metrics_all_some_none():
    r = _metrics([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], [[4, 3, 2, 1], [6, 99, 8], [50, 51]], 4)
    pq = r["per_query"]
    assert pq["recall_at_k"].tolist() == [1.0, 2 / 3, 0.0]
    assert pq["precision_at_k"].tolist() == [1.0, 0.5, 0.0]
    # query 1: hits at ranks 2 and 4; ideal = 3 relevant at ranks 1..3
    want = (_d(2) + _d(4)) / (_d(1) + _d(2) + _d(3))
    assert pq["ndcg_at_k"][0] == 1.0 and pq["ndcg_at_k"][2] == 0.0
    assert abs(float(pq["ndcg_at_k"][1]) - want) < 1e-15
    assert abs(r["recall_at_k"] - (1 + 2 / 3) / 3) < 1e-15 and abs(r["precision_at_k"] - 0.5) < 1e-15
    assert abs(r["ndcg_at_k"] - (1 + want) / 3) < 1e-15
    assert r["queries"] == 3 and r["empty_queries"] == 0 and r["k"] == 4


def test_retrieval_metrics_padding_and_empty_targets():
    # padded lists: precision over the valid ids only; a -1 never hits (nor an id 0 target by accident)
    r = _metrics([[5, 6, -1, -1], [-1, -1, -1, -1], [1, 2, 3, 4]], [[6, 0], [3], []], 4)
    pq = r["per_query"]
    assert pq["recall_at_k"][0] == 0.5 and pq["precision_at_k"][0] == 0.5
    assert abs(float(pq["ndcg_at_k"][0]) - _d(2) / (_d(1) + _d(2))) < 1e-15
    assert pq["recall_at_k"][1] == 0.0 and pq["precision_at_k"][1] == 0.0 and pq["ndcg_at_k"][1] == 0.0
    # the empty target set is left out of the means and counted
    assert math.isnan(float(pq["recall_at_k"][2])) and r["queries"] == 2 and r["empty_queries"] == 1
    assert abs(r["recall_at_k"] - 0.25) < 1e-15 and abs(r["precision_at_k"] - 0.25) < 1e-15


def test_retrieval_metrics_k_smaller_than_the_list_and_known_ndcg():
    pred = [[7, 1, 8, 2, 3, 9]]
    r6 = _metrics(pred, [[1, 2, 3]], 6)
    r3 = _metrics(pred, [[1, 2, 3]], 3)
    assert r6["recall_at_k"] == 1.0 and r6["precision_at_k"] == 0.5
    assert abs(r6["ndcg_at_k"] - (_d(2) + _d(4) + _d(5)) / (_d(1) + _d(2) + _d(3))) < 1e-15
    assert abs(r3["recall_at_k"] - 1 / 3) < 1e-15 and abs(r3["precision_at_k"] - 1 / 3) < 1e-15
    assert abs(r3["ndcg_at_k"] - _d(2) / (_d(1) + _d(2) + _d(3))) < 1e-15
    # more relevant ids than k: the ideal ordering fills all k ranks
    r2 = _metrics([[1, 7]], [[1, 2, 3, 4]], 2)
    assert r2["recall_at_k"] == 0.25 and abs(r2["ndcg_at_k"] - _d(1) / (_d(1) + _d(2))) < 1e-15
    assert math.isnan(_metrics([[1, 2]], [[]], 2)["recall_at_k"])


# ---- the oracle's own conditions ----------------------------------------------------------------


@pytest.mark.parametrize("i", range(len(ro.CASES)))
def test_oracle_band_is_not_vacuous(i):
    """At most 25 % of a case's queries have another item within the tolerance band of the k-th
    best score, so the band rule decides nearly every id of the GPU test."""
    M, N, E, k = ro.CASES[i]
    Q, Cm = ro.case_inputs(i)
    s, tol = ro.exact_scores(Q, Cm)
    assert (tol > 0).all() and float((tol / s.abs().clamp(min=1e-3)).median()) < 1e-3
    assert ro.band_fraction(s, tol, k) <= 0.25
    ids, v = ro.expected_topk(s, k)
    ro.check_band(ids, v.to(torch.float32), s, tol, k)  # the exact answer passes its own rule


def test_oracle_band_is_not_vacuous_l2():
    M, N, E, k = ro.L2_CASE
    Q, Cm = ro.make_inputs(M, N, E, 77)
    b = ro.l2_bias64(Cm).to(torch.float32)
    s, tol = ro.exact_scores(Q, Cm, b)
    assert ro.band_fraction(s, tol, k) <= 0.25
    # the biased inner product orders the items as the ascending L2 distance does
    q, c = ro.bf16_round(Q), ro.bf16_round(Cm)
    d = torch.cdist(q, c) ** 2
    want = torch.sort(d, dim=1, stable=True).indices[:, :k]
    got = ro.expected_topk(q @ c.T + ro.l2_bias64(Cm), k)[0]
    assert (torch.sort(want, 1).values == torch.sort(got, 1).values).float().mean() > 0.99


def test_oracle_rule_rejects_wrong_answers():
    M, N, E, k = 8, 300, 32, 10
    Q, Cm = ro.make_inputs(M, N, E, 5)
    s, tol = ro.exact_scores(Q, Cm)
    ids, v = ro.expected_topk(s, k)
    bad = ids.clone()
    bad[3, k - 1] = torch.sort(s[3], descending=True).indices[k + 40]  # a clearly worse item
    with pytest.raises(AssertionError):
        ro.check_band(bad, s.gather(1, bad).to(torch.float32), s, tol, k)
    with pytest.raises(AssertionError):  # right ids, a score off by 1e-3
        ro.check_band(ids, (v + 1e-3).to(torch.float32), s, tol, k)
    with pytest.raises(AssertionError):  # two entries swapped: not sorted
        sw = ids.clone()
        sw[:, [0, 1]] = ids[:, [1, 0]]
        ro.check_band(sw, s.gather(1, sw).to(torch.float32), s, tol, k)
