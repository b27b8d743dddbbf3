"""tt_topk_mips_large on the GPU (ops.topk_mips_large; lifecycle.retrieve / evaluate_retrieval at
k > 256): the fp64 band rule (tests/retrieval_oracle.py), the selection exactly against the scores the
existing kernel gives ("own scores": tt_topk_mips over 256-row item chunks, sorted by the total order
on the CPU), prefix and agreement with tt_topk_mips(_filtered), split invariance, ties that send the
radix select into the index digits, adversarial stream orders, shape edges, strides, guard words,
filters, and the lifecycle entry points."""
import math

import pytest
import torch

import retrieval_filter_oracle as fo
import retrieval_oracle as ro

pytestmark = pytest.mark.gpu


def _large(Q, Cm, k, device, bias=None, splits=None, items_dtype=torch.float32, allow=None, exclude=None):
    from two_tower_recommender_model_amd import ops

    if allow is not None:
        allow = ops.pack_allow_mask(allow.to(device))
    if exclude is not None:
        v, o = exclude
        o = o.to(device)
        exclude = (ops.sort_exclusions(v.to(device), o, Cm.shape[0]), o)
    ids, sc = ops.topk_mips_large(Q.to(device), Cm.to(device).to(items_dtype), k,
                                  bias=None if bias is None else bias.to(device), splits=splits, allow=allow,
                                  exclude=exclude)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


def _small(Q, Cm, k, device, bias=None, allow=None, exclude=None):
    from two_tower_recommender_model_amd import ops

    if allow is not None:
        allow = ops.pack_allow_mask(allow.to(device))
    if exclude is not None:
        v, o = exclude
        o = o.to(device)
        exclude = (ops.sort_exclusions(v.to(device), o, Cm.shape[0]), o)
    ids, sc = ops.topk_mips(Q.to(device), Cm.to(device), k, bias=None if bias is None else bias.to(device),
                            allow=allow, exclude=exclude)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


_OWN = {}


def _self_scores(Q, Cm, device, bias=None, key=None):
    """The existing kernel's own score of every pair: item chunks of at most 256 rows, k = the chunk.
    Computed once per `key` and shared."""
    if key is not None and key in _OWN:
        return _OWN[key]
    M, N = Q.shape[0], Cm.shape[0]
    full = torch.empty(M, N, dtype=torch.float32)
    for lo in range(0, N, 256):
        hi = min(N, lo + 256)
        ids, sc = _small(Q, Cm[lo:hi], hi - lo, device, bias=None if bias is None else bias[lo:hi])
        assert (torch.sort(ids, 1).values == torch.arange(hi - lo)).all()
        full[:, lo:hi].scatter_(1, ids, sc)
    if key is not None:
        _OWN[key] = full
    return full


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _assert_exact(got, full, k):
    """ids and score bits against the stable descending sort of the own scores; -1 / -inf past N."""
    N = full.shape[1]
    kk = min(k, N)
    want_ids, want_sc = ro.expected_topk(full, k)
    assert torch.equal(got[0][:, :kk], want_ids)
    assert torch.equal(got[1][:, :kk].view(torch.int32), want_sc.view(torch.int32))
    assert (got[0][:, kk:] == -1).all() and (got[1][:, kk:] == float("-inf")).all()


# ---- 1. fp64 band rule --------------------------------------------------------------------------

BAND_CASES = [(17, 3000, 32, 257, 2000), (24, 6000, 64, 1000, 2001), (20, 4000, 96, 3000, 2010),
              (16, 9000, 128, 8192, 2011), (12, 8300, 64, 8192, 2004)]


@pytest.mark.parametrize("items_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M, N, E, k, seed", BAND_CASES)
def test_scores_and_selection_vs_fp64(device, M, N, E, k, seed, items_dtype):
    Q, Cm = ro.make_inputs(M, N, E, seed)
    s, tol = ro.exact_scores(Q, Cm)
    frac = ro.band_fraction(s, tol, k)
    assert frac <= 0.25, frac
    ids, sc = _large(Q, Cm, k, device, items_dtype=items_dtype)
    err = ((sc.double() - s.gather(1, ids)).abs() / tol.gather(1, ids)).max()
    print(f"case {(M, N, E, k)} {items_dtype}: band fraction {frac:.4f}, max score error {float(err):.4f} of the bound")
    ro.check_band(ids, sc, s, tol, k)


def test_l2_bias_vs_fp64(device):
    from two_tower_recommender_model_amd import lifecycle as lc

    M, N, E, k = 24, 6000, 64, 1000
    Q, Cm = ro.make_inputs(M, N, E, 2001)
    bias = lc.l2_bias(Cm.to(device)).cpu()
    s, tol = ro.exact_scores(Q, Cm, bias)
    frac = ro.band_fraction(s, tol, k)
    assert frac <= 0.25, frac
    ids, sc = _large(Q, Cm, k, device, bias=bias)
    print(f"l2 case: band fraction {frac:.4f}")
    ro.check_band(ids, sc, s, tol, k)


# ---- 2. exact against own scores ----------------------------------------------------------------


@pytest.mark.parametrize("k", [257, 1000, 4999, 5000])
def test_selection_exact_vs_own_scores(device, k):
    M, N, E = 40, 5000, 64
    Q, Cm = ro.make_inputs(M, N, E, 2021)
    full = _self_scores(Q, Cm, device, key="exact")
    _assert_exact(_large(Q, Cm, k, device), full, k)


# ---- 3. prefix and agreement with the sorted-list kernels ---------------------------------------


def _filter_inputs(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    allow = torch.rand(N, generator=g) < 0.5
    lists = [torch.randint(0, N, (200,), generator=g).tolist() if m % 3 else [] for m in range(M)]
    return allow, fo.csr(lists)


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
def test_prefix_and_agreement(device, filtered):
    M, N, E = 40, 5000, 64
    Q, Cm = ro.make_inputs(M, N, E, 2021)
    kw = {}
    if filtered:
        allow, excl = _filter_inputs(M, N, 2031)
        kw = dict(allow=allow, exclude=excl)
    ref256 = _small(Q, Cm, 256, device, **kw)
    for k in (257, 3000):
        got = _large(Q, Cm, k, device, **kw)
        assert _same((got[0][:, :256], got[1][:, :256].contiguous()), ref256), k
    assert _same(_large(Q, Cm, 100, device, **kw), _small(Q, Cm, 100, device, **kw))


# ---- 4. split invariance ------------------------------------------------------------------------


@pytest.mark.parametrize("bias", [False, True])
def test_split_invariance(device, bias):
    """S = 2: 10,000 items per pool of 6032 keys, the pools prune. S = 64: 384 items per split, no
    split holds k."""
    M, N, E, k = 20, 20000, 64, 3000
    Q, Cm = ro.make_inputs(M, N, E, 2041)
    b = ro.l2_bias64(Cm).to(torch.float32) if bias else None
    ref = _large(Q, Cm, k, device, bias=b, splits=1)
    for S in (2, 7, 64, None):
        assert _same(_large(Q, Cm, k, device, bias=b, splits=S), ref), S
    assert _same(_large(Q, Cm, k, device, bias=b, splits=7), ref)


# ---- 5. ties ------------------------------------------------------------------------------------


def test_identical_rows_select_on_the_index_digits(device):
    """Every key has the same upper 32 bits: the select decides in the index digits."""
    M, N, E, k = 12, 3000, 64, 1000
    Q, Cm = ro.make_inputs(M, 1, E, 2051)
    for S in (1, 3):
        ids, sc = _large(Q, Cm.repeat(N, 1), k, device, splits=S)
        assert (ids == torch.arange(k)).all(), S
        assert (sc == sc[:, :1]).all()


def test_duplicate_rows_lowest_index_first(device):
    """700 copies of a dominant row from item 1300 on: they straddle the boundary between the two
    splits (item 1536 of 3000) and the k-th place (k = 300): the 300 lowest copies, ascending."""
    M, N, E, k = 17, 3000, 64, 300
    g = torch.Generator().manual_seed(2052)
    u = torch.randn(E, generator=g) * 0.5
    Q = u + 0.05 * torch.randn(M, E, generator=g)
    Cm = torch.randn(N, E, generator=g) * 0.5
    Cm[1300:2000] = 2.0 * u
    for S in (2, 1, None):
        ids, sc = _large(Q, Cm, k, device, splits=S)
        assert (ids == torch.arange(1300, 1300 + k)).all(), S
        assert (sc == sc[:, :1]).all()


def test_zero_queries_return_the_first_k(device):
    M, N, E, k = 20, 3000, 32, 700
    _, Cm = ro.make_inputs(M, N, E, 2053)
    for S in (None, 3):
        ids, sc = _large(torch.zeros(M, E), Cm, k, device, splits=S)
        assert (ids == torch.arange(k)).all()
        assert (sc.view(torch.int32) == 0).all()  # +0.0


# ---- 6. monotone stream -------------------------------------------------------------------------


@pytest.mark.parametrize("reverse", [False, True])
def test_monotone_stream(device, reverse):
    """The ramp of test_gpu_retrieval.test_monotone_stream: score(m, n) = (m + 1) n exactly. Ascending,
    every item is a candidate and a query's pool prunes about 8 times at S = 1 (16384 items through
    2 k + 32 = 4032 places); descending, nothing passes after the first prune."""
    M, N, E, k = 40, 16384, 64, 2000
    n = torch.arange(N)
    Cm = torch.zeros(N, E)
    Cm[:, 0], Cm[:, 1] = (n & 63).float(), (n >> 6).float()
    Q = torch.zeros(M, E)
    Q[:, 0], Q[:, 1] = torch.arange(1, M + 1).float(), 64.0 * torch.arange(1, M + 1)
    if reverse:
        Cm = Cm.flip(0)
    want = torch.arange(k) if reverse else torch.arange(N - 1, N - 1 - k, -1)
    for S in (1, None):
        ids, sc = _large(Q, Cm, k, device, splits=S)
        assert (ids == want).all()
        assert torch.equal(sc, torch.arange(1, M + 1).float()[:, None] * (N - 1 - torch.arange(k)).float())


# ---- 7. edges -----------------------------------------------------------------------------------


@pytest.mark.parametrize("M, N, k, S", [
    (5, 1, 257, None), (5, 300, 300, None), (5, 301, 300, 1), (5, 299, 300, 3), (1, 9000, 8192, None),
    (129, 3000, 500, None), (33, 3000, 500, 2), (9, 8192, 8192, 1), (9, 8193, 8192, 1), (9, 16385, 8192, 1),
    (9, 769, 257, 3),
])
def test_shape_edges(device, M, N, k, S):
    E = 64
    Q, Cm = ro.make_inputs(M, N, E, 2600 + M + N + k)
    s, tol = ro.exact_scores(Q, Cm)
    got = _large(Q, Cm, k, device, splits=S)
    ro.check_band(got[0], got[1], s, tol, k)
    _assert_exact(got, _self_scores(Q, Cm, device), k)


# ---- 8. strides ---------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("col", [8, 3])
def test_strided_items(device, dtype, col):
    """A column slice of a wider buffer (aligned: 16-byte loads; misaligned: element loads) whose
    other columns hold a sentinel that would win every comparison."""
    from two_tower_recommender_model_amd import ops

    M, N, E, k = 20, 3000, 64, 700
    Q, Cm = ro.make_inputs(M, N, E, 2061)
    wide = torch.full((N, E + 16), 1e30, dtype=dtype, device=device)
    wide[:, col:col + E] = Cm.to(device).to(dtype)
    qwide = torch.full((M, E + 5), 1e30, device=device)
    qwide[:, 2:2 + E] = Q.to(device)
    ids, sc = ops.topk_mips_large(qwide[:, 2:2 + E], wide[:, col:col + E], k)
    torch.cuda.synchronize()
    assert _same((ids.cpu(), sc.cpu()), _large(Q, Cm, k, device, items_dtype=dtype))


# ---- 9. guards ----------------------------------------------------------------------------------


def test_guard_words_and_uninitialised_workspace(device):
    """Nothing is written past ids, scores or a workspace of exactly the size the query asks for,
    and what the workspace held before the call does not matter."""
    from two_tower_recommender_model_amd import _lib

    lib = _lib.load()
    M, N, E, k, S = 37, 4000, 64, 700, 3
    Q, Cm = ro.make_inputs(M, N, E, 2062)
    q, c = Q.to(device), Cm.to(device)
    nws = lib.tt_topk_mips_large_workspace_bytes(M, N, k, S)
    assert nws == S * M * (2 * k + 32) * 8
    out = []
    for fill in (0xFF, 0x00):
        ids = torch.full((M * k + 32,), -77, dtype=torch.int64, device=device)
        sc = torch.full((M * k + 32,), -77.0, device=device)
        ws = torch.full((nws + 256,), fill, dtype=torch.uint8, device=device)
        ws[nws:] = 0xAB
        _lib.check(lib.tt_topk_mips_large(q.data_ptr(), _lib.TT_F32, E, c.data_ptr(), _lib.TT_F32, E, None, M, N, E, k,
                                          S, None, None, None, ids.data_ptr(), sc.data_ptr(), ws.data_ptr(), nws,
                                          _lib.stream_handle(device)))
        torch.cuda.synchronize()
        assert (ids[M * k:] == -77).all() and (sc[M * k:] == -77.0).all() and (ws[nws:] == 0xAB).all()
        out.append((ids[:M * k].view(M, k).cpu(), sc[:M * k].view(M, k).cpu()))
    assert _same(out[0], out[1])
    assert _same(out[0], _large(Q, Cm, k, device))


# ---- 10. filters --------------------------------------------------------------------------------

FILTER_SHAPE = (24, 6000, 64, 1000)


def _filter_case(name, device):
    M, N, E, k = FILTER_SHAPE
    Q, Cm = ro.make_inputs(M, N, E, 2001)
    g = torch.Generator().manual_seed(2071)
    allow, lists, lead = None, None, 0
    if name == "mask_half":
        allow = torch.rand(N, generator=g) < 0.5
    elif name in ("mask_k_minus_1", "mask_exactly_k"):
        allow = torch.zeros(N, dtype=torch.bool)
        allow[torch.randperm(N, generator=g)[:k - 1 if name == "mask_k_minus_1" else k]] = True
    elif name in ("own_top_500", "together", "offsets_not_from_0"):
        top = _large(Q, Cm, 500, device)[0]
        lists = [row + torch.randint(0, N, (50,), generator=g).tolist() for row in top.tolist()]
        if name == "together":
            allow = torch.rand(N, generator=g) < 0.5
        if name == "offsets_not_from_0":
            lead = 37
    elif name == "empty_values":
        lists = [[] for _ in range(M)]
    return Q, Cm, k, allow, lists, lead


@pytest.mark.parametrize("name", ["mask_half", "mask_k_minus_1", "mask_exactly_k", "own_top_500", "together",
                                  "empty_values", "offsets_not_from_0"])
def test_filters_exact_vs_own_scores(device, name):
    M, N, E, k = FILTER_SHAPE
    Q, Cm, k, allow, lists, lead = _filter_case(name, device)
    full = _self_scores(Q, Cm, device, key="filters")
    elig = fo.eligibility(M, N, allow, lists)
    if name == "mask_k_minus_1":
        assert (elig.sum(1) == k - 1).all()
    if name == "mask_exactly_k":
        assert (elig.sum(1) == k).all()
    if name != "empty_values":
        assert fo.differs_fraction(full, elig, k) > 0.9
    ids, sc = _large(Q, Cm, k, device, allow=allow, exclude=None if lists is None else fo.csr(lists, lead))
    fo.check_exact(ids, sc, full, elig, k)


# ---- 11. lifecycle ------------------------------------------------------------------------------


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_retrieve_large_k(device, metric):
    from two_tower_recommender_model_amd import lifecycle as lc

    M, N, E, k = 24, 6000, 64, 1000
    Q, Cm = ro.make_inputs(M, N, E, 2001)
    q, c = Q.to(device), Cm.to(device)
    bias = lc.l2_bias(c) if metric == "l2" else None
    labels, sc = lc.retrieve(q, c, k=k, metric=metric)
    torch.cuda.synchronize()
    s, tol = ro.exact_scores(Q, Cm, None if bias is None else bias.cpu())
    assert ro.band_fraction(s, tol, k) <= 0.25
    ro.check_band(labels.cpu() - 1, sc.cpu(), s, tol, k)
    assert _same((labels.cpu() - 1, sc.cpu()), _large(Q, Cm, k, device, bias=None if bias is None else bias.cpu()))
    # seen lists (labels, unsorted) through a chunked call's offset views: equal to the single call
    g = torch.Generator().manual_seed(2081)
    seen = [(labels[m, :300].cpu()[torch.randperm(300, generator=g)]).tolist() if m % 4 else [] for m in range(M)]
    sv, so = fo.csr(seen)
    one = lc.retrieve(q, c, k=k, metric=metric, seen_values=sv, seen_offsets=so)
    chunked = lc.retrieve(q, c, k=k, metric=metric, seen_values=sv, seen_offsets=so, query_chunk=7)
    torch.cuda.synchronize()
    assert _same((one[0].cpu(), one[1].cpu()), (chunked[0].cpu(), chunked[1].cpu()))
    for m in range(M):
        assert not (set(one[0][m].tolist()) & set(seen[m]))
        if seen[m]:
            assert torch.equal(one[0][m, :k - 300].cpu(), labels[m, 300:].cpu())


def _metrics_by_formula(ids, targets, k):
    rec, prec, ndcg = [], [], []
    for row, t in zip(ids.tolist(), targets):
        if not t:
            continue
        row = row[:k]
        valid = [i for i in row if i >= 0]
        hits = [1 if (i >= 0 and i in t) else 0 for i in row]
        rec.append(sum(hits) / len(t))
        prec.append(sum(hits) / len(valid) if valid else 0.0)
        dcg = sum(h / math.log2(r + 2) for r, h in enumerate(hits))
        idcg = sum(1 / math.log2(r + 2) for r in range(min(len(t), k)))
        ndcg.append(dcg / idcg)
    n = len(rec)
    return sum(rec) / n, sum(prec) / n, sum(ndcg) / n


def test_evaluate_retrieval_large_k(device):
    from two_tower_recommender_model_amd import lifecycle as lc
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    N, D, layers, k = [500, 3000], 32, [32, 32], 1000
    st = FusedTwoTowerStep(N, [D, D], [0], [1], layers, 64, device, seed=9)
    g = torch.Generator().manual_seed(2090)
    for t in (0, 1):
        st.tables.table_view(t).copy_((torch.randn(N[t], D, generator=g) * 0.5).to(device))
    user_rows = torch.randperm(N[0], generator=g)[:60]
    targets = [set((torch.randperm(N[1], generator=g)[:int(n)] + 1).tolist())
               for n in torch.randint(0, 60, (60,), generator=g)]
    targets[3] = set()
    tv = torch.tensor([v for t in targets for v in sorted(t)], dtype=torch.int64)
    to = torch.tensor([0] + [len(t) for t in targets], dtype=torch.int64).cumsum(0)
    res = lc.evaluate_retrieval(st, user_rows, tv, to, k=k)
    labels, sc = lc.retrieve_fused(st, user_rows, k=k)
    torch.cuda.synchronize()
    labels = labels.cpu()
    assert labels.shape == (60, k) and labels.min() >= 1 and labels.max() <= N[1]
    assert (torch.sort(labels, 1).values.diff(dim=1) > 0).all() and (sc.cpu().diff(dim=1) <= 0).all()
    rec, prec, ndcg = _metrics_by_formula(labels, targets, k)
    assert res["queries"] == sum(1 for t in targets if t) and res["empty_queries"] == sum(1 for t in targets if not t)
    assert abs(res["recall_at_k"] - rec) < 1e-12 and abs(res["precision_at_k"] - prec) < 1e-12
    assert abs(res["ndcg_at_k"] - ndcg) < 1e-12
    assert 0.0 < rec < 1.0
