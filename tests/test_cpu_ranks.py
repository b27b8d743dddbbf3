"""tt_target_ranks without a GPU: the bindings (beside, not among, the counted entry points), its
declared limits as status codes before any launch, the workspace query, and metrics.rank_metrics
against metrics.retrieval_metrics on lists whose ranks are known by construction."""
import math

import pytest
import torch

FAKE = 1 << 20  # never dereferenced: every call here must return before any launch
F32, BF16 = 2, 3
NAMES = ("tt_target_ranks_workspace_bytes", "tt_target_ranks")


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd import _lib
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


def test_bindings_and_pinned_constants(lib):
    from two_tower_recommender_model_amd import _lib

    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.RANK_ENTRY_POINTS
        assert name not in _lib.COMPUTE_ENTRY_POINTS and name not in _lib.IVF_ENTRY_POINTS
        assert name not in _lib.TOPK_LARGE_ENTRY_POINTS
        assert getattr(lib, name).argtypes is not None
    assert sorted(_lib.RANK_ENTRY_POINTS) == sorted(NAMES)
    assert lib.tt_num_entry_points() == 55 == len(_lib.COMPUTE_ENTRY_POINTS)
    assert lib.tt_abi_version() == 4


def _call(lib, M=8, N=100, E=64, T=20, L=0, splits=0, q_dtype=F32, c_dtype=F32, ldq=None, ldc=None, queries=FAKE,
          items=FAKE, tv=FAKE, to=FAKE, allow=None, xv=None, xo=None, ranks=FAKE, scores=None, ws=FAKE, ws_bytes=1 << 50):
    rc = lib.tt_target_ranks(queries, q_dtype, E if ldq is None else ldq, items, c_dtype, E if ldc is None else ldc, None,
                             M, N, E, tv, to, T, allow, xv, xo, L, splits, ranks, scores, ws, ws_bytes, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(E=0), "E must"), (dict(E=48), "E must"), (dict(E=160), "E must"),
    (dict(M=0), "M must"), (dict(M=(1 << 30) + 1), "M must"),
    (dict(N=0), "N must"), (dict(N=1 << 31), "N must"),
    (dict(splits=65), "splits must"), (dict(splits=-1), "splits must"),
    (dict(xv=FAKE, L=5), "excl_values"), (dict(xo=FAKE), "excl_values"),
    (dict(T=-1), "T_cap must"), (dict(L=-1), "L_cap must"), (dict(L=5), "L_cap must"),
    (dict(q_dtype=0), "q_dtype"), (dict(c_dtype=1), "c_dtype"), (dict(ldq=63), "ldq"), (dict(ldc=32), "ldc"),
    (dict(queries=None), "null"), (dict(items=None), "null"), (dict(tv=None), "null"), (dict(to=None), "null"),
    (dict(ranks=None), "null"), (dict(ws=None), "null"),
    (dict(ws_bytes=100), "ws_bytes"),
])
def test_limits_are_status_codes(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_target_ranks") and word in msg, (kw, msg)


def test_workspace_query(lib):
    ws = lib.tt_target_ranks_workspace_bytes
    for bad in [(0, 100, 20, 0, 0), (8, 0, 20, 0, 0), (8, 1 << 31, 20, 0, 0), (8, 100, 20, 0, 65), (8, 100, 20, 0, -1),
                (8, 100, -1, 0, 0), (8, 100, 20, -1, 0), ((1 << 30) + 1, 100, 20, 0, 1)]:
        assert ws(*bad) == 0, bad
    # the per-split counts are the only part that grows with the splits: 4 bytes a target each
    M, N, T, L = 1000, 1 << 20, 8000, 30000
    one = ws(M, N, T, L, 1)
    assert one > 0 and ws(M, N, T, L, 5) - one == 4 * 4 * T
    assert ws(M, 10 ** 8, T, L, 3) == ws(M, N, T, L, 3)  # independent of N at fixed splits
    # the header's figure, 4 (S + 1) T + 4 L + 16 (T / 8 + L / 16 + 2 M), up to the parts' alignment
    S = 3
    approx = 4 * (S + 1) * T + 4 * L + 16 * (T // 8 + L // 16 + 2 * M)
    assert approx <= ws(M, N, T, L, S) <= approx + 8 * 256
    # no targets, no exclusions: still a valid (small) workspace
    assert 0 < ws(1, 1, 0, 0, 1) <= 2048
    auto = ws(16, 1 << 22, 100, 0, 0)
    assert ws(16, 1 << 22, 100, 0, 1) < auto <= ws(16, 1 << 22, 100, 0, 64)  # few queries: several splits


# ---- rank_metrics ---------------------------------------------------------------------------------


def _permutation_case():
    """Random permutations as the prediction lists (M = 50, N = 400), jagged targets (0..12 a query),
    some of them marked ineligible: (lists [M, N], target values, offsets, ranks with -1 marks)."""
    M, N = 50, 400
    g = torch.Generator().manual_seed(4242)
    lists = torch.stack([torch.randperm(N, generator=g) for _ in range(M)])
    pos = torch.empty(M, N, dtype=torch.int64)
    pos.scatter_(1, lists, torch.arange(N).repeat(M, 1))  # pos[m, id] = the id's column
    vals, offs, ranks = [], [0], []
    for m in range(M):
        n = int(torch.randint(0, 13, (1,), generator=g)) if m not in (0, 7) else (0 if m == 0 else 12)
        t = torch.randperm(N, generator=g)[:n]
        for j, v in enumerate(t.tolist()):
            dead = (m * 31 + j) % 9 == 0  # ineligible: never in the list, rank -1
            vals.append(N + 5 + j if dead else v)
            ranks.append(-1 if dead else int(pos[m, v]))
        offs.append(offs[-1] + n)
    return lists, torch.tensor(vals, dtype=torch.int64), torch.tensor(offs, dtype=torch.int64), \
        torch.tensor(ranks, dtype=torch.int64)


def test_rank_metrics_equal_retrieval_metrics():
    from two_tower_recommender_model_amd.metrics import rank_metrics, retrieval_metrics

    lists, vals, offs, ranks = _permutation_case()
    M = lists.shape[0]
    ks = (1, 10, 100)
    got = rank_metrics(ranks, offs, ks=ks)
    assert got["ks"] == ks
    for k in ks:
        ref = retrieval_metrics(lists, vals, offs, k)
        a, b = got["per_query"]["recall_at_k"][k], ref["per_query"]["recall_at_k"]
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()]), k
        a, b = got["per_query"]["ndcg_at_k"][k], ref["per_query"]["ndcg_at_k"]
        assert torch.equal(a.isnan(), b.isnan()) and float((a[~a.isnan()] - b[~b.isnan()]).abs().max()) <= 1e-12, k
        assert got["recall_at_k"][k] == pytest.approx(ref["recall_at_k"], abs=1e-15)
        assert abs(got["ndcg_at_k"][k] - ref["ndcg_at_k"]) <= 1e-12
        assert (got["queries"], got["empty_queries"]) == (ref["queries"], ref["empty_queries"])

    # MRR, the mean and median rank and the counts by a hand-written loop
    rr, elig, empty = [], [], 0
    for m in range(M):
        r = ranks[offs[m]:offs[m + 1]].tolist()
        if not r:
            empty += 1
            continue
        ok = [x for x in r if x >= 0]
        elig += ok
        rr.append(1.0 / (1 + min(ok)) if ok else 0.0)
    assert empty >= 1 and got["empty_queries"] == empty and got["queries"] == M - empty
    assert got["ineligible_targets"] == int((ranks < 0).sum()) > 0
    assert abs(got["mrr"] - sum(rr) / len(rr)) <= 1e-12
    assert abs(got["mean_rank"] - sum(elig) / len(elig)) <= 1e-9
    assert got["median_rank"] == sorted(elig)[(len(elig) - 1) // 2]
    per = got["per_query"]["reciprocal_rank"]
    assert int(per.isnan().sum()) == empty and torch.allclose(per[~per.isnan()], torch.tensor(rr, dtype=torch.float64))


def test_rank_metrics_edges():
    from two_tower_recommender_model_amd.metrics import rank_metrics

    # offsets that start past 0 (a chunk's view); a query with only ineligible targets; no targets at all
    ranks = torch.tensor([99, 98, 0, 5, -1, -1, 3], dtype=torch.int64)
    offs = torch.tensor([2, 4, 6, 6, 7], dtype=torch.int64)
    got = rank_metrics(ranks, offs, ks=(1, 4))
    assert got["queries"] == 3 and got["empty_queries"] == 1 and got["ineligible_targets"] == 2
    assert got["recall_at_k"][1] == pytest.approx((0.5 + 0 + 0) / 3) and got["recall_at_k"][4] == pytest.approx((0.5 + 0 + 1) / 3)
    idcg2 = 1 + 1 / math.log2(3)
    assert got["ndcg_at_k"][4] == pytest.approx((1 / idcg2 + 0 + 1 / math.log2(5)) / 3)
    assert got["mrr"] == pytest.approx((1 + 0 + 0.25) / 3)
    assert got["mean_rank"] == pytest.approx(8 / 3) and got["median_rank"] == 3
    none = rank_metrics(torch.zeros(0, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    assert none["queries"] == 0 and none["empty_queries"] == 3 and math.isnan(none["mrr"]) and math.isnan(none["mean_rank"])
    assert math.isnan(none["recall_at_k"][10])


def test_lifecycle_checks_before_any_device_work():
    from two_tower_recommender_model_amd import lifecycle as lc

    z = torch.zeros(4, 64)
    with pytest.raises(ValueError, match="metric"):
        lc.target_ranks(z, z, torch.zeros(0, dtype=torch.int64), torch.zeros(5, dtype=torch.int64), metric="cosine")
    with pytest.raises(ValueError, match="M \\+ 1"):
        lc.target_ranks(z, z, torch.zeros(0, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
