"""tt_target_ranks on the GPU (ops.target_ranks, lifecycle.target_ranks / evaluate_ranks). The rule is
exact wherever an exact oracle exists (tests/rank_cases.py): a target's rank is its column in the
complete order that ops.topk_mips_large(k = N) returns, its score that column's bits; at larger N the
columns of ops.topk_mips(k = 256), and the fp64 band."""
import pytest
import torch

import rank_cases as rc
import retrieval_filter_oracle as fo
import retrieval_oracle as ro

pytestmark = pytest.mark.gpu

SPLITS = (1, 3, 64, None)


def _bits(x):
    return x.view(torch.int32)


def _order(Q, C, device, bias=None, allow=None, exclude=None):
    """Each query's complete order of its eligible items, from the selection kernels: (ids, scores) [M, N]."""
    from two_tower_recommender_model_amd import ops

    ids, sc = ops.topk_mips_large(Q, C, C.shape[0], bias=bias, allow=allow, exclude=exclude)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


def _ranks(Q, C, tv, to, device, **kw):
    from two_tower_recommender_model_amd import ops

    r, s = ops.target_ranks(Q, C, tv.to(device), to.to(device), return_scores=True, **kw)
    torch.cuda.synchronize()
    return r.cpu(), s.cpu()


def _check(got, want, what=""):
    bad = (got[0] != want[0]).nonzero().flatten().tolist()
    assert not bad, f"{what}: ranks differ at {bad[:8]}: {got[0][bad[:8]].tolist()} vs {want[0][bad[:8]].tolist()}"
    assert torch.equal(_bits(got[1]), _bits(want[1])), f"{what}: score bits differ"


def _words(allow, device):
    from two_tower_recommender_model_amd import ops

    return ops.pack_allow_mask(allow.to(device))


def _exclude(lists, N, device, lead=0):
    from two_tower_recommender_model_amd import ops

    vals, offs = fo.csr(lists, lead=lead)
    if lead:
        offs = torch.cat([torch.tensor([0, 1, 2]), offs]).to(device)[3:]
    else:
        offs = offs.to(device)
    return ops.sort_exclusions(vals.to(device), offs, N), offs


# ---- 1. the full-order oracle ---------------------------------------------------------------------


@pytest.mark.parametrize("items_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rank_is_the_column_of_the_full_order(device, shape, with_bias, items_bf16):
    M, N, E = shape
    Q, C = ro.make_inputs(M, N, E, 5000 + N)
    targets = rc.jagged_targets(M, N, 5100 + N, most=40 if M == 130 else 12)
    if M == 130:
        n = [len(t) for t in targets]
        assert 0 in n and rc.R in n and rc.R + 1 in n and max(n) > 2 * rc.R + 1 and any(x >= N for t in targets for x in t)
    tv, to = rc.csr(targets)
    Q, C = Q.to(device), C.to(device)
    if items_bf16:
        C = C.to(torch.bfloat16)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.3).to(device) if with_bias else None
    want = rc.expected_from_order(*_order(Q, C, device, bias=bias), targets)
    assert int((want[0] < 0).sum()) == sum(1 for t in targets for x in t if not 0 <= x < N)
    for S in SPLITS:
        _check(_ranks(Q, C, tv, to, device, bias=bias, splits=S), want, f"splits={S}")


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_every_query_has_T_targets(device, T):
    """The scan compares only the target slots that some query of a 16-query tile uses: 1, 2, 4 or 8."""
    M, N, E = 37, 1037, 64
    Q, C = ro.make_inputs(M, N, E, 5201)
    targets = rc.band_targets(M, N, T, 5202 + T)
    tv, to = rc.csr(targets)
    Q, C = Q.to(device), C.to(device)
    want = rc.expected_from_order(*_order(Q, C, device), targets)
    for S in (1, 3):
        _check(_ranks(Q, C, tv, to, device, splits=S), want, f"T={T} splits={S}")


def test_strided_rows_and_bf16_queries(device):
    M, N, E = 40, 3000, 96
    Q, C = ro.make_inputs(M, N, E, 5301)
    targets = rc.jagged_targets(M, N, 5302, most=12)
    tv, to = rc.csr(targets)
    Qw = torch.zeros(M, E + 40, device=device)
    Cw = torch.zeros(N, E + 7, device=device)  # rows that 16-byte loads cannot fetch
    Qw[:, :E], Cw[:, :E] = Q.to(device), C.to(device)
    want = rc.expected_from_order(*_order(Q.to(device), C.to(device), device), targets)
    _check(_ranks(Qw[:, :E], Cw[:, :E], tv, to, device), want, "strided")
    # bf16 queries that are exactly the rounded fp32 ones: the same scores
    _check(_ranks(Q.to(device).to(torch.bfloat16), C.to(device), tv, to, device), want, "bf16 queries")


# ---- 2. ties --------------------------------------------------------------------------------------


def test_ties_follow_the_index_rule(device):
    M, N, E = 20, 2000, 64
    Q, C = ro.make_inputs(M, N, E, 5401)
    # item 700's row also at a lower and a higher index; items 300 and 1300 identical
    C[40], C[1990], C[1300] = C[700], C[700], C[300]
    targets = [[700, 40, 1990, 300, 1300] + ([5, 1999] if m % 2 else []) for m in range(M)]
    tv, to = rc.csr(targets)
    Q, C = Q.to(device), C.to(device)
    want = rc.expected_from_order(*_order(Q, C, device), targets)
    for S in SPLITS:
        got = _ranks(Q, C, tv, to, device, splits=S)
        _check(got, want, f"splits={S}")
    r = got[0].view(-1).tolist()
    at = 0
    for ts in targets:
        by = dict(zip(ts, r[at:at + len(ts)]))
        at += len(ts)
        # equal scores, consecutive ranks in index order (nothing else ties with them in this data)
        assert by[40] + 1 == by[700] and by[700] + 1 == by[1990] and by[300] + 1 == by[1300]
    assert torch.equal(_bits(got[1][0:1]), _bits(got[1][1:2])) and torch.equal(_bits(got[1][3:4]), _bits(got[1][4:5]))


# ---- 3. filters -----------------------------------------------------------------------------------


def _filter_case():
    M, N, E = 37, 1037, 64  # the mask's last word is partial
    Q, C = ro.make_inputs(M, N, E, 5501)
    targets = rc.jagged_targets(M, N, 5502, most=20)
    return M, N, E, Q, C, targets


@pytest.mark.parametrize("kind", ["half", "sparse", "zeros"])
def test_allow_masks(device, kind):
    M, N, E, Q, C, targets = _filter_case()
    g = torch.Generator().manual_seed(5503)
    allow = {"half": torch.rand(N, generator=g) < 0.5, "sparse": torch.rand(N, generator=g) < 0.03,
             "zeros": torch.zeros(N, dtype=torch.bool)}[kind]
    if kind != "zeros":
        allow[N - 1] = True  # a bit of the partial word
    tv, to = rc.csr(targets)
    Q, C, w = Q.to(device), C.to(device), _words(allow, device)
    want = rc.expected_from_order(*_order(Q, C, device, allow=w), targets)
    for S in SPLITS:
        _check(_ranks(Q, C, tv, to, device, allow=w, splits=S), want, f"{kind} splits={S}")
    denied = torch.tensor([not (0 <= x < N and bool(allow[x])) for t in targets for x in t])
    assert torch.equal(want[0] < 0, denied) and denied.any()
    if kind == "zeros":
        assert (want[0] == -1).all()


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("masked", [False, True])
def test_seen_segments(device, lead, masked):
    """Segments with duplicates and out-of-range values, one that holds its query's target, and items
    above and below each target in the unfiltered order; with `lead`, both offset arrays are views
    that do not start at 0."""
    M, N, E, Q, C, targets = _filter_case()
    g = torch.Generator().manual_seed(5504)
    Qd, Cd = Q.to(device), C.to(device)
    order = _order(Qd, Cd, device)[0]
    lists = []
    for m in range(M):
        l = torch.randint(0, N, (int(torch.randint(0, 60, (1,), generator=g)),), generator=g).tolist()
        ts = [t for t in targets[m] if 0 <= t < N]
        if ts and m % 3 != 2:
            col = int((order[m] == ts[0]).nonzero())
            l += order[m, max(0, col - 3):col].tolist() + order[m, col + 1:col + 4].tolist()  # above and below
        if len(ts) > 1 and m % 4 == 1:
            l.append(ts[1])  # the query's own target
        l += l[:5] + [N, N + 3, -1, -70]  # duplicates, out of range
        lists.append(l if m % 5 else [])
    assert any(set(l) & set(t) for l, t in zip(lists, targets))
    allow = _words(torch.rand(N, generator=g) < 0.6, device) if masked else None
    excl = _exclude(lists, N, device, lead=lead)
    tv, to = rc.csr(targets, lead=lead)
    if lead:
        to = torch.cat([torch.tensor([0, 0, 0]), to]).to(device)[3:]
        assert to.storage_offset() == 3 and int(to[0]) == lead and int(excl[1][0]) == lead
    want = rc.expected_from_order(*_order(Qd, Cd, device, allow=allow, exclude=excl), targets)
    for S in SPLITS:
        got = _ranks(Qd, Cd, tv, to, device, allow=allow, exclude=excl, splits=S)
        # the positions before the first offset belong to no query: not written
        assert (got[0][:lead] == -1).all() and (got[1][:lead] == float("-inf")).all()
        _check((got[0][lead:], got[1][lead:]), want, f"splits={S}")
    seen = torch.tensor([x in set(l) for l, t in zip(lists, targets) for x in t])
    assert (want[0][seen] == -1).all() and seen.any()


def test_chunked_calls_fill_one_output(device):
    from two_tower_recommender_model_amd import ops

    M, N, E, Q, C, targets = _filter_case()
    g = torch.Generator().manual_seed(5505)
    lists = [torch.randint(0, N, (30,), generator=g).tolist() for _ in range(M)]
    Q, C = Q.to(device), C.to(device)
    excl = _exclude(lists, N, device)
    tv, to = rc.csr(targets)
    tv, to = tv.to(device), to.to(device)
    whole = ops.target_ranks(Q, C, tv, to, exclude=excl, return_scores=True)
    ranks = torch.full_like(whole[0], -5)
    scores = torch.full_like(whole[1], -5.0)
    for lo, hi in [(0, 1), (1, 20), (20, M)]:
        ops.target_ranks(Q[lo:hi], C, tv, to[lo:hi + 1], exclude=(excl[0], excl[1][lo:hi + 1]), out=(ranks, scores),
                         return_scores=True)
    torch.cuda.synchronize()
    assert torch.equal(ranks, whole[0]) and torch.equal(_bits(scores), _bits(whole[1]))


# ---- 4. larger N: the columns of the small-k lists, and the fp64 band --------------------------------


def test_small_k_equivalence(device):
    from two_tower_recommender_model_amd import ops

    M, N, E, k = 64, 50000, 64, 256
    Q, C = ro.make_inputs(M, N, E, 5601)
    Q, C = Q.to(device), C.to(device)
    ids, sc = ops.topk_mips(Q, C, k)
    torch.cuda.synchronize()
    ids, sc = ids.cpu(), sc.cpu()
    g = torch.Generator().manual_seed(5602)
    targets = [ids[m, [0, 1, 17, 128, 255]].tolist() + torch.randint(0, N, (m % 6,), generator=g).tolist() for m in range(M)]
    tv, to = rc.csr(targets)
    for S in (None, 7):
        r, s = _ranks(Q, C, tv, to, device, splits=S)
        at = 0
        for m, ts in enumerate(targets):
            for t in ts:
                col = (ids[m] == t).nonzero().flatten().tolist()
                if col:
                    assert int(r[at]) == col[0] and torch.equal(_bits(s[at:at + 1]), _bits(sc[m, col[0]:col[0] + 1])), (m, t)
                else:
                    assert int(r[at]) >= k and float(s[at]) <= float(sc[m, k - 1]), (m, t)
                at += 1


@pytest.mark.parametrize("case", rc.BAND_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_fp64_band(device, case):
    """The issue's band rule. The fp64 reference alone (CPU) gives shares of exactly decided targets of
    0.95, 0.78, 1.0 and 0.87 for the four cases and a widest band of 4, so the band hides little."""
    M, N, E, T, seed = case
    Q, C = ro.make_inputs(M, N, E, seed)
    targets = rc.band_targets(M, N, T, seed)
    lo, hi = rc.band(Q, C, targets)
    tv, to = rc.csr(targets)
    r, _ = _ranks(Q.to(device), C.to(device), tv, to, device)
    exact = float((lo == hi).float().mean())
    print(f"band case {case}: exactly decided {exact:.3f}, widest band {int((hi - lo).max())}")
    assert exact >= 0.7 and int((hi - lo).max()) <= 8
    assert ((r >= lo) & (r <= hi)).all(), ((r < lo) | (r > hi)).nonzero().flatten().tolist()[:8]


# ---- 5. guard words -------------------------------------------------------------------------------


def test_guard_words(device):
    """Nothing is written past ranks, scores or the workspace the size query asks for, nothing before
    the first offset, and no input is written at all."""
    from two_tower_recommender_model_amd import _lib

    lib = _lib.load()
    M, N, E, Q, C, targets = _filter_case()
    g = torch.Generator().manual_seed(5701)
    lists = [torch.randint(0, N, (25,), generator=g).tolist() for _ in range(M)]
    lead, S = 4, 3
    q, cm = Q.to(device), C.to(device)
    allow = _words(torch.rand(N, generator=g) < 0.7, device)
    xv, xo = _exclude(lists, N, device)
    tv, to = rc.csr(targets, lead=lead)
    tv, to = tv.to(device), to.to(device)
    T, L = tv.numel(), xv.numel()
    keep = [t.clone() for t in (q, cm, allow, xv, xo, tv, to)]
    nws = lib.tt_target_ranks_workspace_bytes(M, N, T, L, S)
    assert nws > 0
    ranks = torch.full((T + 32,), -77, dtype=torch.int64, device=device)
    sc = torch.full((T + 32,), -77.0, device=device)
    ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=device)
    _lib.check(lib.tt_target_ranks(q.data_ptr(), _lib.TT_F32, E, cm.data_ptr(), _lib.TT_F32, E, None, M, N, E, tv.data_ptr(),
                                   to.data_ptr(), T, allow.data_ptr(), xv.data_ptr(), xo.data_ptr(), L, S, ranks.data_ptr(),
                                   sc.data_ptr(), ws.data_ptr(), nws, _lib.stream_handle(device)))
    torch.cuda.synchronize()
    assert (ranks[T:] == -77).all() and (sc[T:] == -77.0).all() and (ws[nws:] == 0xAB).all()
    assert (ranks[:lead] == -77).all() and (sc[:lead] == -77.0).all()
    for a, b in zip(keep, (q, cm, allow, xv, xo, tv, to)):
        assert torch.equal(a, b)
    want = rc.expected_from_order(*_order(q, cm, device, allow=allow, exclude=(xv, xo)), targets)
    _check((ranks[lead:T].cpu(), sc[lead:T].cpu()), want, "raw call")
    # without the scores output
    ranks2 = torch.full((T,), -77, dtype=torch.int64, device=device)
    _lib.check(lib.tt_target_ranks(q.data_ptr(), _lib.TT_F32, E, cm.data_ptr(), _lib.TT_F32, E, None, M, N, E, tv.data_ptr(),
                                   to.data_ptr(), T, allow.data_ptr(), xv.data_ptr(), xo.data_ptr(), L, S, ranks2.data_ptr(),
                                   None, ws.data_ptr(), nws, _lib.stream_handle(device)))
    torch.cuda.synchronize()
    assert torch.equal(ranks2, ranks[:T])


def test_bad_offsets_give_empty_segments(device):
    """Target offsets that decrease or point past T_cap, and the same for the exclusion offsets: the
    query's segment is empty, the others are served as usual."""
    M, N, E, Q, C, targets = _filter_case()
    g = torch.Generator().manual_seed(5801)
    lists = [torch.randint(0, N, (10,), generator=g).tolist() for _ in range(M)]
    Q, C = Q.to(device), C.to(device)
    xv, xo = _exclude(lists, N, device)
    tv, to = rc.csr(targets)
    good = _ranks(Q, C, tv, to, device, exclude=(xv, xo))
    to_bad, xo_bad = to.clone(), xo.clone()
    to_bad[10] = tv.numel() + 1000  # queries 9 and 10 lose their segments
    to_bad[20] = -3  # and 19 and 20
    xo_bad[6] = xv.numel() + 50  # queries 5 and 6 have no exclusions now
    got = _ranks(Q, C, tv, to_bad, device, exclude=(xv, xo_bad.to(device)))
    nox = _ranks(Q, C, tv, to, device)
    for m in range(M):
        a, b = int(to[m]), int(to[m + 1])
        if m in (9, 10, 19, 20):
            assert (got[0][a:b] == -1).all() and (got[1][a:b] == float("-inf")).all(), m
        else:
            ref = nox if m in (5, 6) else good
            assert torch.equal(got[0][a:b], ref[0][a:b]) and torch.equal(_bits(got[1][a:b]), _bits(ref[1][a:b])), m


# ---- 6. end to end --------------------------------------------------------------------------------


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_evaluate_ranks_equals_evaluate_retrieval(device, metric):
    from two_tower_recommender_model_amd import lifecycle as lc
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    N, D, layers, U = [500, 700], 32, [32, 32], 150
    st = FusedTwoTowerStep(N, [D, D], [0], [1], layers, 64, device, seed=9)
    g = torch.Generator().manual_seed(92)
    for t in (0, 1):
        st.tables.table_view(t).copy_((torch.randn(N[t], D, generator=g) * 0.5).to(device))
    user_rows = torch.randperm(N[0], generator=g)[:U]
    item_emb = lc.export_fused(st, "candidate")[1]
    top = lc.retrieve_fused(st, user_rows, k=40, metric=metric, item_emb=item_emb)[0].cpu()
    seen, targets = [], []
    for u in range(U):
        rnd = (torch.randint(0, N[1], (int(torch.randint(0, 40, (1,), generator=g)),), generator=g) + 1).tolist()
        seen.append([] if u % 7 == 0 else top[u, :20:2].tolist() + rnd + [0, N[1] + 1, -3])
        cand = (torch.randperm(N[1], generator=g)[:int(torch.randint(0, 25, (1,), generator=g))] + 1).tolist()
        # held-out items: near the top, anywhere, one the user has seen, one label outside 1..N
        targets.append(sorted(set(cand) | set(top[u, 1:40:5].tolist()) | set(seen[u][:1]) | ({N[1] + 9} if u % 11 == 0 else set())))
    targets[3] = []
    sv, so = fo.csr(seen)
    tv, to = rc.csr(targets, dtype=torch.int64)
    for kw in (dict(), dict(seen_values=sv, seen_offsets=so), dict(seen_values=sv, seen_offsets=so, query_chunk=16),
               dict(allow=torch.rand(N[1], generator=g) < 0.5, seen_values=sv, seen_offsets=so, query_chunk=64)):
        got = lc.evaluate_ranks(st, user_rows, tv, to, ks=(10, 100), metric=metric, item_emb=item_emb, **kw)
        for k in (10, 100):
            ref = lc.evaluate_retrieval(st, user_rows, tv, to, k=k, metric=metric, item_emb=item_emb, **kw)
            assert got["recall_at_k"][k] == ref["recall_at_k"], (kw.keys(), k)
            assert abs(got["ndcg_at_k"][k] - ref["ndcg_at_k"]) <= 1e-12
            a, b = got["per_query"]["recall_at_k"][k].cpu(), ref["per_query"]["recall_at_k"].cpu()
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()])
            assert (got["queries"], got["empty_queries"]) == (ref["queries"], ref["empty_queries"])
        assert got["ineligible_targets"] >= sum(1 for t in targets if N[1] + 9 in t)
        assert 0.0 < got["mrr"] <= 1.0 and got["mean_rank"] >= 0
    # the ranks themselves, chunked or not, and the seen target's -1
    r1 = lc.target_ranks(_user_emb(st, user_rows, device), item_emb, tv, to, metric=metric, seen_values=sv, seen_offsets=so)
    r2 = lc.target_ranks(_user_emb(st, user_rows, device), item_emb, tv, to, metric=metric, seen_values=sv, seen_offsets=so,
                         query_chunk=33)
    torch.cuda.synchronize()
    assert torch.equal(r1, r2)
    r1 = r1.cpu()
    for u in range(U):
        for j, t in enumerate(targets[u]):
            if t in seen[u] or not 1 <= t <= N[1]:
                assert int(r1[int(to[u]) + j]) == -1, (u, t)


def _user_emb(st, user_rows, device):
    from two_tower_recommender_model_amd import lifecycle as lc, ops

    towers = lc._tower_views(st.params, [st.in_q, st.in_c], st.layer_sizes)
    x = st.tables.table_view(0)[user_rows.to(device)]
    for w, b in towers[0]:
        x = ops.linear_fwd([x], [w.contiguous()], [b], relu=True)[0]
    return x
