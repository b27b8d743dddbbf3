"""tt_topk_mips_filtered on the GPU (ops.topk_mips with allow / exclude, lifecycle.retrieve* with
allow / seen lists). The rule is exact (tests/retrieval_filter_oracle.py): the kernel's own score of
every pair comes from the unfiltered tt_topk_mips over item chunks of at most 256 rows with k = the
chunk; each query's denied items are removed on the CPU, the rest sorted by the total order and
padded with (-1, -inf); ids and score bits of the filtered call must equal that."""
import math

import pytest
import torch

import retrieval_filter_oracle as fo
import retrieval_oracle as ro

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _unfiltered(Q, Cm, k, device, splits=None):
    from two_tower_recommender_model_amd import ops

    ids, sc = ops.topk_mips(Q.to(device), Cm.to(device), k, splits=splits)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


def _self_scores(Q, Cm, device):
    """The kernel's own score of every pair: item chunks of at most 256 rows, k = the chunk."""
    M, N = Q.shape[0], Cm.shape[0]
    full = torch.empty(M, N, dtype=torch.float32)
    for lo in range(0, N, 256):
        hi = min(N, lo + 256)
        ids, sc = _unfiltered(Q, Cm[lo:hi], hi - lo, device)
        assert (torch.sort(ids, 1).values == torch.arange(hi - lo)).all()
        full[:, lo:hi].scatter_(1, ids, sc)
    return full


def _words(allow, device, tail_ones=False):
    """The packed mask of bool [N]; the bits past N of the last word zero, or all ones."""
    from two_tower_recommender_model_amd import ops

    w = ops.pack_allow_mask(allow.to(device))
    N = allow.numel()
    if tail_ones and N % 32:
        w[-1] |= torch.tensor(-(1 << (N % 32)), dtype=torch.int32, device=device)  # bits N % 32 .. 31
    return w


def _exclude(lists, N, device, lead=0):
    """(sorted int32 values, int64 offsets [M + 1]) on the device; with `lead` the offsets start at
    `lead` and are a view into a longer tensor."""
    from two_tower_recommender_model_amd import ops

    vals, offs = fo.csr(lists, lead=lead)
    if lead:
        offs = torch.cat([torch.tensor([0, 1, 2]), offs]).to(device)[3:]
        assert offs.storage_offset() == 3 and int(offs[0]) == lead
    else:
        offs = offs.to(device)
    return ops.sort_exclusions(vals.to(device), offs, N), offs


def _filtered(c, device, splits=None, lead=0, tail_ones=False):
    from two_tower_recommender_model_amd import ops

    N = c["Cm"].shape[0]
    allow = None if c["allow"] is None else _words(c["allow"], device, tail_ones)
    exclude = None if c["lists"] is None else _exclude(c["lists"], N, device, lead)
    ids, sc = ops.topk_mips(c["Q"].to(device), c["Cm"].to(device), c["k"], splits=splits, allow=allow, exclude=exclude)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


def _check_case(c, device, splits=(None,), **kw):
    M, N = c["Q"].shape[0], c["Cm"].shape[0]
    full = _self_scores(c["Q"], c["Cm"], device)
    elig = fo.eligibility(M, N, c["allow"], c["lists"])
    out = None
    for S in splits:
        out = _filtered(c, device, splits=S, **kw)
        fo.check_exact(out[0], out[1], full, elig, c["k"])
    return out, full, elig


def _raw(lib, q, c, k, S, allow, xv, xo, device):
    from two_tower_recommender_model_amd import _lib

    M, E = q.shape
    N = c.shape[0]
    ids = torch.empty(M, k, dtype=torch.int64, device=device)
    sc = torch.empty(M, k, dtype=torch.float32, device=device)
    nws = lib.tt_topk_mips_workspace_bytes(M, N, k, S)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    _lib.check(lib.tt_topk_mips_filtered(q.data_ptr(), _lib.TT_F32, E, c.data_ptr(), _lib.TT_F32, E, None, M, N, E, k, S,
                                         _lib.ptr(allow), _lib.ptr(xv), _lib.ptr(xo), ids.data_ptr(), sc.data_ptr(),
                                         ws.data_ptr(), nws, _lib.stream_handle(device)))
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


# ---- 1. no-op equivalence -----------------------------------------------------------------------


def test_noop_filters_equal_the_unfiltered_call(device):
    from two_tower_recommender_model_amd import _lib

    lib = _lib.load()
    M, N, E, k = 40, 3000, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 100)
    q, c = Q.to(device), Cm.to(device)
    ones = _words(torch.ones(N, dtype=torch.bool), device)
    xv = torch.full((4,), 5, dtype=torch.int32, device=device)  # never inside a segment
    xo = torch.full((M + 1,), 2, dtype=torch.int64, device=device)  # every list empty
    for S in (1, 7, None):
        ref = _unfiltered(Q, Cm, k, device, splits=S)
        assert _same(_raw(lib, q, c, k, S or 0, None, None, None, device), ref), S
        assert _same(_raw(lib, q, c, k, S or 0, ones, xv, xo, device), ref), S
        assert _same(_raw(lib, q, c, k, S or 0, ones, None, None, device), ref), S
        assert _same(_raw(lib, q, c, k, S or 0, None, xv, xo, device), ref), S
    case = dict(Q=Q, Cm=Cm, k=k, allow=torch.ones(N, dtype=torch.bool), lists=[[] for _ in range(M)])
    assert _same(_filtered(case, device), ref)


# ---- 2. a query's own top k excluded ------------------------------------------------------------


def test_own_topk_excluded_gives_the_next_k(device):
    """The unfiltered ranks 100..199 are the filtered top 100 once ranks 0..99 are denied: a denied
    item that raised a threshold (or was only dropped from the output) would lose some of them."""
    c = fo.case_own_topk()
    k = c["k"]
    ids2, sc2 = _unfiltered(c["Q"], c["Cm"], 2 * k, device)
    case = dict(c, lists=ids2[:, :k].tolist())
    for S in (1, 2, None):
        ids, sc = _filtered(case, device, splits=S)
        assert torch.equal(ids, ids2[:, k:]) and torch.equal(_bits(sc), _bits(sc2[:, k:])), S


# ---- 3. mask only -------------------------------------------------------------------------------


@pytest.mark.parametrize("tail_ones", [False, True])
def test_mask_half(device, tail_ones):
    _check_case(fo.case_mask_half(), device, splits=(None, 1, 3), tail_ones=tail_ones)


@pytest.mark.parametrize("tail_ones", [False, True])
def test_mask_leaves_only_the_last_item(device, tail_ones):
    c = fo.case_mask_last_only()
    (ids, sc), _, _ = _check_case(c, device, splits=(None, 1), tail_ones=tail_ones)
    N = c["Cm"].shape[0]
    assert (ids[:, 0] == N - 1).all() and (ids[:, 1:] == -1).all() and (sc[:, 1:] == float("-inf")).all()


@pytest.mark.parametrize("tail_ones", [False, True])
def test_mask_of_zeros_returns_nothing(device, tail_ones):
    (ids, sc), _, _ = _check_case(fo.case_mask_none(), device, splits=(None, 2), tail_ones=tail_ones)
    assert (ids == -1).all() and (sc == float("-inf")).all()


# ---- 4. exclusion list shapes -------------------------------------------------------------------


@pytest.mark.parametrize("lead", [0, 5])
def test_list_shapes(device, lead):
    """Empty, one item, many, duplicates and out-of-range values, a run across the split boundary,
    all N items, fewer than k left; with lead = 5 the offsets are a view that starts at 5."""
    c = fo.case_list_shapes()
    (ids, sc), _, elig = _check_case(c, device, splits=(2, None, 1), lead=lead)
    left = elig.sum(1)
    assert (ids[left == 0] == -1).all()
    short = (left > 0) & (left < c["k"])
    assert short.any() and ((ids[short] >= 0).sum(1) == left[short]).all()


# ---- 5. mask and lists together -----------------------------------------------------------------


@pytest.mark.parametrize("E, k", fo.TOGETHER)
def test_mask_and_lists_together(device, E, k):
    _check_case(fo.case_together(E, k), device, splits=(None, 2))


# ---- 6. ties ------------------------------------------------------------------------------------


def test_ties_lowest_eligible_index_first(device):
    c = fo.case_ties()
    k = c["k"]
    for S in (2, 1, None):
        (ids, sc), _, elig = _check_case(c, device, splits=(S,))
        for m in range(ids.shape[0]):
            copies = [n for n in fo.TIE_DUP if elig[m, n]]
            assert len(copies) in (9, 10)
            assert ids[m, :len(copies)].tolist() == copies, (S, m)
            assert (sc[m, :len(copies)] == sc[m, 0]).all()


# ---- 7. adversarial order -----------------------------------------------------------------------


@pytest.mark.parametrize("reverse", [False, True])
def test_monotone_stream(device, reverse):
    c = fo.case_monotone(reverse)
    M, N, k = c["Q"].shape[0], c["Cm"].shape[0], c["k"]
    (ids, sc), _, _ = _check_case(c, device, splits=(1, None))
    # odd items only, the last 50 denied: forward the best is item N - 51 (odd), reversed item 1
    want = torch.arange(1, 2 * k, 2) if reverse else torch.arange(N - 51, N - 51 - 2 * k, -2)
    assert (ids == want).all()
    rank = (N - 1 - want) if reverse else want  # the ramp value of the item
    assert torch.equal(sc, torch.arange(1, M + 1).float()[:, None] * rank.float())


# ---- 8. shape edge ------------------------------------------------------------------------------


def test_query_129_alone_has_a_list(device):
    c = fo.case_edge_129()
    (ids, _), _, _ = _check_case(c, device, splits=(None, 1))
    assert not (set(ids[128].tolist()) & set(c["lists"][128]))


# ---- 9. split invariance ------------------------------------------------------------------------


def test_split_invariance(device):
    c = fo.case_split_invariance()
    (ref, _, _) = _check_case(c, device, splits=(1,))
    for S in (2, 7, 64, None):
        assert _same(_filtered(c, device, splits=S), ref), S
    assert _same(_filtered(c, device, splits=7), ref)


# ---- 10. guard words ----------------------------------------------------------------------------


def test_guard_words(device):
    """Nothing is written past ids, scores or the workspace the size query asks for, and nothing of
    the mask or the lists is written at all."""
    from two_tower_recommender_model_amd import _lib

    lib = _lib.load()
    c = fo.case_split_invariance()
    M, N, E, k, S = c["Q"].shape[0], c["Cm"].shape[0], 64, c["k"], 3
    q, cm = c["Q"].to(device), c["Cm"].to(device)
    allow = _words(c["allow"], device)
    xv, xo = _exclude(c["lists"], N, device)
    allow0, xv0, xo0 = allow.clone(), xv.clone(), xo.clone()
    nws = lib.tt_topk_mips_workspace_bytes(M, N, k, S)
    assert nws == S * M * k * 8
    ids = torch.full((M * k + 32,), -77, dtype=torch.int64, device=device)
    sc = torch.full((M * k + 32,), -77.0, device=device)
    ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=device)
    _lib.check(lib.tt_topk_mips_filtered(q.data_ptr(), _lib.TT_F32, E, cm.data_ptr(), _lib.TT_F32, E, None, M, N, E, k, S,
                                         allow.data_ptr(), xv.data_ptr(), xo.data_ptr(), ids.data_ptr(), sc.data_ptr(),
                                         ws.data_ptr(), nws, _lib.stream_handle(device)))
    torch.cuda.synchronize()
    assert (ids[M * k:] == -77).all() and (sc[M * k:] == -77.0).all() and (ws[nws:] == 0xAB).all()
    assert torch.equal(allow, allow0) and torch.equal(xv, xv0) and torch.equal(xo, xo0)
    ref = _filtered(c, device)
    assert torch.equal(ids[:M * k].view(M, k).cpu(), ref[0]) and torch.equal(sc[:M * k].view(M, k).cpu(), ref[1])


# ---- 11. end to end -----------------------------------------------------------------------------


def _metrics_by_formula(labels, targets, k):
    rec, prec, ndcg = [], [], []
    for row, t in zip(labels.tolist(), targets):
        if not t:
            continue
        valid = [i for i in row[:k] if i > 0]
        hits = [1 if (i > 0 and i in t) else 0 for i in row[:k]]
        rec.append(sum(hits) / len(t))
        prec.append(sum(hits) / len(valid) if valid else 0.0)
        dcg = sum(h / math.log2(r + 2) for r, h in enumerate(hits))
        ndcg.append(dcg / sum(1 / math.log2(r + 2) for r in range(min(len(t), k))))
    n = len(rec)
    return sum(rec) / n, sum(prec) / n, sum(ndcg) / n


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_evaluate_retrieval_with_seen_items(device, metric):
    from two_tower_recommender_model_amd import lifecycle as lc
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    N, D, layers, k, U = [500, 700], 32, [32, 32], 20, 150
    st = FusedTwoTowerStep(N, [D, D], [0], [1], layers, 64, device, seed=9)
    g = torch.Generator().manual_seed(91)
    for t in (0, 1):
        st.tables.table_view(t).copy_((torch.randn(N[t], D, generator=g) * 0.5).to(device))
    user_rows = torch.randperm(N[0], generator=g)[:U]
    item_emb = lc.export_fused(st, "candidate")[1]

    # today's call, and its first 100: a user's seen set is most of the unfiltered top k / 2 (the
    # training positives a trained model ranks first), some random items and labels outside 1..N
    base_labels, base_sc = lc.retrieve_fused(st, user_rows, k=100, metric=metric, item_emb=item_emb)
    today = lc.retrieve_fused(st, user_rows, k=k, metric=metric, item_emb=item_emb)
    torch.cuda.synchronize()
    base_labels, base_sc = base_labels.cpu(), base_sc.cpu()
    assert torch.equal(today[0].cpu(), base_labels[:, :k])
    seen = []
    for u in range(U):
        if u % 7 == 0:
            seen.append([])
            continue
        rnd = (torch.randint(0, N[1], (int(torch.randint(0, 50, (1,), generator=g)),), generator=g) + 1).tolist()
        seen.append(base_labels[u, :k // 2:2].tolist() + rnd + [0, N[1] + 1, N[1] + 40, -3])
    sv, so = fo.csr(seen)
    targets = []
    for u in range(U):  # held-out items: a few the user has not seen
        cand = (torch.randperm(N[1], generator=g)[:int(torch.randint(0, 30, (1,), generator=g))] + 1).tolist()
        targets.append(set(cand) - set(seen[u]) | set(base_labels[u, 1:k:4].tolist()) - set(seen[u]))
    targets[3] = set()
    tv = torch.tensor([v for t in targets for v in sorted(t)], dtype=torch.int64)
    to = torch.tensor([0] + [len(t) for t in targets], dtype=torch.int64).cumsum(0)

    labels, sc = lc.retrieve_fused(st, user_rows, k=k, metric=metric, item_emb=item_emb, seen_values=sv, seen_offsets=so)
    chunked = lc.retrieve_fused(st, user_rows, k=k, metric=metric, item_emb=item_emb, seen_values=sv, seen_offsets=so,
                                query_chunk=16)
    torch.cuda.synchronize()
    labels, sc = labels.cpu(), sc.cpu()
    assert torch.equal(chunked[0].cpu(), labels) and torch.equal(_bits(chunked[1].cpu()), _bits(sc))
    changed = 0
    for u in range(U):
        assert not (set(labels[u].tolist()) & set(seen[u])), u
        # exactly the unfiltered list (same score bits) without the seen items
        keep = [j for j in range(100) if int(base_labels[u, j]) not in seen[u]][:k]
        assert labels[u].tolist() == base_labels[u, keep].tolist(), u
        assert torch.equal(_bits(sc[u]), _bits(base_sc[u, keep])), u
        changed += labels[u].tolist() != base_labels[u, :k].tolist()
    assert changed >= 0.75 * U

    res = lc.evaluate_retrieval(st, user_rows, tv, to, k=k, metric=metric, item_emb=item_emb, seen_values=sv,
                                seen_offsets=so)
    rec, prec, ndcg = _metrics_by_formula(labels, targets, k)
    assert res["queries"] == sum(1 for t in targets if t) and res["empty_queries"] == sum(1 for t in targets if not t)
    assert abs(res["recall_at_k"] - rec) < 1e-12 and abs(res["precision_at_k"] - prec) < 1e-12
    assert abs(res["ndcg_at_k"] - ndcg) < 1e-12

    # an item mask (bool over the rows, or packed) on top; with everything None, today's result
    allow = torch.rand(N[1], generator=g) < 0.5
    a1 = lc.retrieve_fused(st, user_rows, k=k, metric=metric, item_emb=item_emb, allow=allow, seen_values=sv, seen_offsets=so)
    a2 = lc.retrieve_fused(st, user_rows, k=k, metric=metric, item_emb=item_emb, allow=_words(allow, device),
                           seen_values=sv.to(device), seen_offsets=so.to(device), query_chunk=64)
    torch.cuda.synchronize()
    assert _same((a1[0].cpu(), a1[1].cpu()), (a2[0].cpu(), a2[1].cpu()))
    got = a1[0].cpu()
    assert allow[(got - 1).clamp(min=0)][got > 0].all() and (got > 0).all()
    none = lc.evaluate_retrieval(st, user_rows, tv, to, k=k, metric=metric, item_emb=item_emb, allow=None,
                                 seen_values=None, seen_offsets=None)
    old = lc.evaluate_retrieval(st, user_rows, tv, to, k=k, metric=metric, item_emb=item_emb)
    for key in ("recall_at_k", "precision_at_k", "ndcg_at_k", "queries", "empty_queries", "k"):
        assert none[key] == old[key]
