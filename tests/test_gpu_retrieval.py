"""tt_topk_mips on the GPU (ops.topk_mips, lifecycle.retrieve / retrieve_fused / evaluate_retrieval):
scores and selection against the fp64 oracle's band rule (tests/retrieval_oracle.py), the selection
exactly against the kernel's own scores, split invariance, ties, adversarial stream orders, shape
edges with guard words, the L2 bias, and the end-to-end retrieval metrics of a small fused step."""
import math

import pytest
import torch

import retrieval_oracle as ro

pytestmark = pytest.mark.gpu

QTILE, CHUNK = 128, 128  # queries per workgroup, items per staged chunk at E = 64 (csrc/retrieval.hip)


def _topk(Q, Cm, k, device, bias=None, splits=None, items_dtype=torch.float32):
    from two_tower_recommender_model_amd import ops

    ids, sc = ops.topk_mips(Q.to(device), Cm.to(device).to(items_dtype), k,
                            bias=None if bias is None else bias.to(device), splits=splits)
    torch.cuda.synchronize()
    return ids.cpu(), sc.cpu()


def _self_scores(Q, Cm, device, bias=None):
    """The kernel's own score of every pair: item chunks of at most 256 rows, k = the chunk."""
    M, N = Q.shape[0], Cm.shape[0]
    full = torch.empty(M, N, dtype=torch.float32)
    for lo in range(0, N, 256):
        hi = min(N, lo + 256)
        ids, sc = _topk(Q, Cm[lo:hi], hi - lo, device, bias=None if bias is None else bias[lo:hi])
        assert (torch.sort(ids, 1).values == torch.arange(hi - lo)).all()
        full[:, lo:hi].scatter_(1, ids, sc)
    return full


# ---- 1. scores and selection against fp64 -------------------------------------------------------


@pytest.mark.parametrize("items_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(ro.CASES)))
def test_scores_and_selection_vs_fp64(device, i, items_dtype):
    M, N, E, k = ro.CASES[i]
    Q, Cm = ro.case_inputs(i)
    s, tol = ro.exact_scores(Q, Cm)
    frac = ro.band_fraction(s, tol, k)
    assert frac <= 0.25, frac
    ids, sc = _topk(Q, Cm, k, device, items_dtype=items_dtype)
    err = ((sc.double() - s.gather(1, ids)).abs() / tol.gather(1, ids)).max()
    print(f"case {ro.CASES[i]} {items_dtype}: band fraction {frac:.3f}, max score error {float(err):.4f} of the bound")
    ro.check_band(ids, sc, s, tol, k)


# ---- 2. selection exact -------------------------------------------------------------------------


def test_selection_exact_vs_own_scores(device):
    """Position independence: the full run equals, bit for bit, the CPU sort (total order) of the
    scores the kernel itself gives for the same pairs in 256-row item chunks."""
    M, N, E, k = 40, 1037, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 21)
    full = _self_scores(Q, Cm, device)
    want_ids, want_sc = ro.expected_topk(full, k)
    ids, sc = _topk(Q, Cm, k, device)
    assert torch.equal(ids, want_ids)
    assert torch.equal(sc.view(torch.int32), want_sc.view(torch.int32))


# ---- 3. split invariance ------------------------------------------------------------------------


@pytest.mark.parametrize("bias", [False, True])
def test_split_invariance(device, bias):
    M, N, E, k = 40, 3000, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 31)
    b = ro.l2_bias64(Cm).to(torch.float32) if bias else None
    ref = _topk(Q, Cm, k, device, bias=b, splits=1)
    for S in (2, 7, None, 64):
        got = _topk(Q, Cm, k, device, bias=b, splits=S)
        assert torch.equal(got[0], ref[0]), S
        assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), S
    again = _topk(Q, Cm, k, device, bias=b, splits=7)
    assert torch.equal(again[0], ref[0]) and torch.equal(again[1].view(torch.int32), ref[1].view(torch.int32))


# ---- 4. ties ------------------------------------------------------------------------------------


def test_duplicate_rows_lowest_index_first(device):
    """13 copies of one dominant row, straddling the boundary between two splits (item 640 of 1037
    at splits = 2) and the k-th place (k = 10): the 10 lowest indices, in ascending order."""
    M, N, E, k = 17, 1037, 64, 10
    g = torch.Generator().manual_seed(41)
    u = torch.randn(E, generator=g) * 0.5
    Q = u + 0.05 * torch.randn(M, E, generator=g)
    Cm = torch.randn(N, E, generator=g) * 0.5
    dup = list(range(635, 642)) + list(range(900, 906))
    Cm[dup] = 2.0 * u
    for S in (2, 1, None):
        ids, sc = _topk(Q, Cm, k, device, splits=S)
        assert (ids == torch.tensor(dup[:k])).all(), S
        assert (sc == sc[:, :1]).all()


def test_zero_queries_return_the_first_k(device):
    M, N, E, k = 20, 700, 32, 100
    _, Cm = ro.make_inputs(M, N, E, 42)
    for S in (None, 3):
        ids, sc = _topk(torch.zeros(M, E), Cm, k, device, splits=S)
        assert (ids == torch.arange(k)).all()
        assert (sc.view(torch.int32) == 0).all()  # +0.0


def test_fp32_items_equal_their_bf16_roundings(device):
    M, N, E, k = 33, 2000, 96, 50
    Q, Cm = ro.make_inputs(M, N, E, 43)
    a = _topk(Q, Cm, k, device)
    b = _topk(Q, Cm, k, device, items_dtype=torch.bfloat16)
    c = _topk(Q.to(torch.bfloat16), Cm, k, device)
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1].view(torch.int32), x[1].view(torch.int32))


# ---- 5. adversarial order -----------------------------------------------------------------------


@pytest.mark.parametrize("reverse", [False, True])
def test_monotone_stream(device, reverse):
    """Every item beats every earlier one (the filter never rejects; every candidate buffer overflows
    and prunes all the way), and the reverse. (n / N) v is not strictly increasing once rounded to
    bf16, so the ramp is built from exactly representable digits: c_n = (n & 63, n >> 6, 0, ...),
    q_m = (m + 1) (1, 64, 0, ...), score = (m + 1) n exactly."""
    M, N, E, k = 40, 3000, 64, 100
    n = torch.arange(N)
    Cm = torch.zeros(N, E)
    Cm[:, 0], Cm[:, 1] = (n & 63).float(), (n >> 6).float()
    Q = torch.zeros(M, E)
    Q[:, 0], Q[:, 1] = torch.arange(1, M + 1).float(), 64.0 * torch.arange(1, M + 1)
    if reverse:
        Cm = Cm.flip(0)
    want = torch.arange(k) if reverse else torch.arange(N - 1, N - 1 - k, -1)
    for S in (1, None):
        ids, sc = _topk(Q, Cm, k, device, splits=S)
        assert (ids == want).all()
        assert torch.equal(sc, torch.arange(1, M + 1).float()[:, None] * (N - 1 - torch.arange(k)).float())


# ---- 6. edges -----------------------------------------------------------------------------------


@pytest.mark.parametrize("M, N, k, S", [
    (5, 1, 1, None), (5, 1, 7, None), (5, 30, 30, None), (5, 31, 30, None), (5, 12, 30, 3),
    (1, 500, 20, None), (QTILE + 1, 300, 10, None), (33, 300, 10, 2),
    (9, CHUNK + 1, 16, 1), (9, 3 * 2 * CHUNK + 1, 16, 3), (9, 2 * CHUNK, 256, 2), (9, 65, 16, 1), (9, 385, 16, 3),
])
def test_shape_edges(device, M, N, k, S):
    E = 64
    Q, Cm = ro.make_inputs(M, N, E, 600 + M + N + k)
    s, tol = ro.exact_scores(Q, Cm)
    ids, sc = _topk(Q, Cm, k, device, splits=S)
    ro.check_band(ids, sc, s, tol, k)
    # and exactly the total-order sort of the kernel's own scores
    want_ids, want_sc = ro.expected_topk(_self_scores(Q, Cm, device), k)
    kk = min(k, N)
    assert torch.equal(ids[:, :kk], want_ids) and torch.equal(sc[:, :kk], want_sc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("col", [8, 3])
def test_strided_items(device, dtype, col):
    """A column slice of a wider buffer (aligned: 16-byte loads; misaligned: element loads) whose
    other columns hold a sentinel that would win every comparison."""
    from two_tower_recommender_model_amd import ops

    M, N, E, k = 20, 700, 64, 40
    Q, Cm = ro.make_inputs(M, N, E, 61)
    wide = torch.full((N, E + 16), 1e30, dtype=dtype, device=device)
    wide[:, col:col + E] = Cm.to(device).to(dtype)
    qwide = torch.full((M, E + 5), 1e30, device=device)
    qwide[:, 2:2 + E] = Q.to(device)
    ids, sc = ops.topk_mips(qwide[:, 2:2 + E], wide[:, col:col + E], k)
    torch.cuda.synchronize()
    ref = _topk(Q, Cm, k, device, items_dtype=dtype)
    assert torch.equal(ids.cpu(), ref[0]) and torch.equal(sc.cpu(), ref[1])


def test_guard_words(device):
    """Nothing is written past ids, scores or the workspace the size query asks for."""
    from two_tower_recommender_model_amd import _lib

    lib = _lib.load()
    M, N, E, k, S = 37, 900, 64, 100, 3
    Q, Cm = ro.make_inputs(M, N, E, 62)
    q, c = Q.to(device), Cm.to(device)
    nws = lib.tt_topk_mips_workspace_bytes(M, N, k, S)
    assert nws == S * M * k * 8
    ids = torch.full((M * k + 32,), -77, dtype=torch.int64, device=device)
    sc = torch.full((M * k + 32,), -77.0, device=device)
    ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=device)
    _lib.check(lib.tt_topk_mips(q.data_ptr(), _lib.TT_F32, E, c.data_ptr(), _lib.TT_F32, E, None, M, N, E, k, S,
                                ids.data_ptr(), sc.data_ptr(), ws.data_ptr(), nws, _lib.stream_handle(device)))
    torch.cuda.synchronize()
    assert (ids[M * k:] == -77).all() and (sc[M * k:] == -77.0).all() and (ws[nws:] == 0xAB).all()
    ref = _topk(Q, Cm, k, device)
    assert torch.equal(ids[:M * k].view(M, k).cpu(), ref[0]) and torch.equal(sc[:M * k].view(M, k).cpu(), ref[1])


# ---- 7. bias / L2 -------------------------------------------------------------------------------


def test_l2_metric(device):
    """metric="l2": the k smallest fp64 L2 distances of the bf16-rounded rows, by the band rule on
    q.c - 0.5 |c|^2 (the same order: |q - c|^2 = |q|^2 - 2 (q.c - 0.5 |c|^2))."""
    from two_tower_recommender_model_amd import lifecycle as lc

    M, N, E, k = ro.L2_CASE
    Q, Cm = ro.make_inputs(M, N, E, 77)
    bias = lc.l2_bias(Cm.to(device))
    b64 = ro.l2_bias64(Cm)
    assert torch.allclose(bias.cpu().double(), b64, rtol=2.0 ** -23, atol=0)
    s, tol = ro.exact_scores(Q, Cm, bias.cpu())
    assert ro.band_fraction(s, tol, k) <= 0.25
    labels, sc = lc.retrieve(Q.to(device), Cm.to(device), k=k, metric="l2", query_chunk=16)
    torch.cuda.synchronize()
    ids = labels.cpu() - 1
    ro.check_band(ids, sc.cpu(), s, tol, k)
    # the same rule stated on the distances
    q, c = ro.bf16_round(Q), ro.bf16_round(Cm)
    d = (q * q).sum(1, keepdim=True) - 2.0 * (q @ c.T + b64)
    dk = torch.sort(d, dim=1).values[:, k - 1:k]
    got = torch.zeros(M, N, dtype=torch.bool).scatter_(1, ids, True)
    assert (got | ~(d < dk - 2 * tol)).all() and not (got & (d > dk + 2 * tol)).any()
    dot_labels, _ = lc.retrieve(Q.to(device), Cm.to(device), k=k, metric="dot")
    assert not torch.equal(dot_labels.cpu(), labels.cpu())


# ---- 8. end to end ------------------------------------------------------------------------------


def _fp64_tower(x, layers):
    """The tower on bf16-rounded operands in fp64, layer by layer as the GPU runs it (fp32 outputs,
    rounded to bf16 as the next layer's operand). Returns (embeddings fp64, safe [rows] bool): a row
    is safe when no activation lies within the fp32 accumulation bound of a bf16 rounding boundary
    (or of the ReLU's zero), so that the GPU's bf16 operands equal the reference's exactly; the bound
    is (K + 1) 2^-24 (sum |x||w| + |b|) per element, as in retrieval_oracle."""
    safe = torch.ones(x.shape[0], dtype=torch.bool)
    x = x.to(torch.float64)
    for w, b in layers:
        xb, wb = ro.bf16_round(x), ro.bf16_round(w)
        b = b.to(torch.float64)
        pre = xb @ wb.T + b
        bound = (xb.shape[1] + 1) * ro.U * (xb.abs() @ wb.abs().T + b.abs())
        x = pre.clamp(min=0)
        # distance of each output to the nearest bf16 rounding boundary (midpoint of neighbours)
        r = ro.bf16_round(x)
        p2 = 2.0 ** torch.floor(torch.log2(r.abs().clamp(min=1e-300)))
        ulp = torch.where(r.abs() == p2, p2 * 2.0 ** -8, p2 * 2.0 ** -7)  # the finer spacing at a power of two
        dist = ulp / 2 - (x - r).abs()
        safe &= ((pre.abs() > bound) & ((x == 0) | (dist > bound))).all(1)
    return x, safe


def _metrics_by_formula(ids, targets, k):
    rec, prec, ndcg = [], [], []
    for row, t in zip(ids.tolist(), targets):
        row = [i for i in row[:k]]
        valid = [i for i in row if i >= 0]
        hits = [1 if (i >= 0 and i in t) else 0 for i in row]
        if not t:
            continue
        rec.append(sum(hits) / len(t))
        prec.append(sum(hits) / len(valid) if valid else 0.0)
        dcg = sum(h / math.log2(r + 2) for r, h in enumerate(hits))
        idcg = sum(1 / math.log2(r + 2) for r in range(min(len(t), k)))
        ndcg.append(dcg / idcg)
    n = len(rec)
    return sum(rec) / n, sum(prec) / n, sum(ndcg) / n, rec, prec


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_evaluate_retrieval_end_to_end(device, metric):
    from two_tower_recommender_model_amd import lifecycle as lc
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    N, D, layers, k = [500, 700], 32, [32, 32], 20
    st = FusedTwoTowerStep(N, [D, D], [0], [1], layers, 64, device, seed=9)
    g = torch.Generator().manual_seed(90)
    # table rows randn * 0.5, redrawn until every row is safe (see _fp64_tower): the reference's bf16
    # operands are then the GPU's, and the band rule's tolerance is the score kernel's alone
    towers = lc._tower_views(st.params.cpu(), [st.in_q, st.in_c], st.layer_sizes)
    for t in (0, 1):
        rows = torch.randn(N[t], D, generator=g) * 0.5
        for _ in range(40):
            safe = _fp64_tower(rows, towers[t])[1]
            if safe.all():
                break
            rows[~safe] = torch.randn(int((~safe).sum()), D, generator=g) * 0.5
        assert safe.all()
        st.tables.table_view(t).copy_(rows.to(device))
    user_rows = torch.randperm(N[0], generator=g)[:150]
    targets = [set((torch.randperm(N[1], generator=g)[:int(n)] + 1).tolist())
               for n in torch.randint(0, 60, (150,), generator=g)]
    targets[3] = set()
    tv = torch.tensor([v for t in targets for v in sorted(t)], dtype=torch.int64)
    to = torch.tensor([0] + [len(t) for t in targets], dtype=torch.int64).cumsum(0)

    res = lc.evaluate_retrieval(st, user_rows, tv, to, k=k, metric=metric)
    labels, sc = lc.retrieve_fused(st, user_rows, k=k, metric=metric)
    torch.cuda.synchronize()
    labels, sc = labels.cpu(), sc.cpu()
    assert labels.min() >= 1 and labels.max() <= N[1]

    # the metric dict is the formulas applied to the retrieved labels
    rec, prec, ndcg, rec_q, prec_q = _metrics_by_formula(labels, targets, k)
    assert res["queries"] == sum(1 for t in targets if t) and res["empty_queries"] == sum(1 for t in targets if not t)
    assert abs(res["recall_at_k"] - rec) < 1e-12 and abs(res["precision_at_k"] - prec) < 1e-12
    assert abs(res["ndcg_at_k"] - ndcg) < 1e-12

    # the same towers in fp64 on the bf16-rounded operands, torch.topk, the formulas
    uq = _fp64_tower(st.tables.table_view(0).cpu()[user_rows], towers[0])[0]
    ci = _fp64_tower(st.tables.table_view(1).cpu(), towers[1])[0]
    bias = ro.l2_bias64(ci).to(torch.float32) if metric == "l2" else None
    s, tol = ro.exact_scores(uq, ci, bias)
    frac = ro.band_fraction(s, tol, k)
    print(f"{metric}: band fraction {frac:.3f}")
    assert frac <= 0.25
    ro.check_band(labels - 1, sc, s, tol, k)

    # wherever no band item decides a hit, recall and precision equal the reference's
    want_ids = ro.expected_topk(s, k)[0] + 1
    _, _, _, rec_w, prec_w = _metrics_by_formula(want_ids, targets, k)
    tau = ro.kth_best(s, k).unsqueeze(1)
    inband = (s - tau).abs() <= tol
    j = compared = 0
    for m, t in enumerate(targets):
        if not t:
            continue
        band_items = set((inband[m].nonzero().flatten() + 1).tolist())
        if len(band_items) <= 1 or not (band_items & t):
            assert rec_q[j] == rec_w[j] and prec_q[j] == prec_w[j], m
            compared += 1
        j += 1
    print(f"{metric}: {compared} of {res['queries']} queries compared with the reference's recall / precision")
    assert compared >= 0.75 * res["queries"], compared
