"""Oracle and cases of filtered top-k retrieval (tt_topk_mips_filtered).

The rule is exact, not a tolerance: given the score of every pair (on the GPU: the kernel's own,
from unfiltered tt_topk_mips over item chunks with k = the chunk), a query's expected list is its
ELIGIBLE items sorted by the total order "higher score first, equal scores by lower index", cut at k
and padded with (-1, -inf). `check_exact` asserts ids and score bits against it and names what went
wrong: a denied item returned, an eligible item displaced, a missing -1 tail.

The cases are built here so that the CPU suite can assert on fp64 scores that they are not vacuous:
every non-empty exclusion list holds items of its query's exact top max(1, k / 2) (but for the reversed
ramp, whose lists are the stream's last items as in the forward ramp and whose mask does the work),
and the masks deny about half the catalogue, so nearly every query's filtered list differs from its
unfiltered one.
"""
from __future__ import annotations

import torch

import retrieval_oracle as ro

NEG_INF = float("-inf")


def eligibility(M, N, allow=None, lists=None):
    """bool [M, N]: allow (bool [N] or None) minus each query's list (values outside [0, N) match nothing)."""
    elig = torch.ones(M, N, dtype=torch.bool) if allow is None else allow.clone().unsqueeze(0).repeat(M, 1)
    if lists is not None:
        assert len(lists) == M
        for m, l in enumerate(lists):
            v = torch.tensor([x for x in l if 0 <= x < N], dtype=torch.int64)
            elig[m, v] = False
    return elig


def expected_filtered(scores, elig, k):
    """(ids [M, k] int64, scores [M, k] of scores' dtype): the eligible items by the total order,
    (-1, -inf) past them. Scores are finite, so -inf marks a denied item."""
    M, N = scores.shape
    assert torch.isfinite(scores).all()
    s = torch.where(elig, scores, torch.full_like(scores, NEG_INF))
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    kk = min(k, N)
    ids = torch.full((M, k), -1, dtype=torch.int64)
    out = torch.full((M, k), NEG_INF, dtype=scores.dtype)
    ok = elig.gather(1, i[:, :kk])
    ids[:, :kk] = torch.where(ok, i[:, :kk], torch.full_like(i[:, :kk], -1))
    out[:, :kk] = v[:, :kk]
    return ids, out


def check_exact(ids, got, scores, elig, k):
    """ids [M, k] int64 / got [M, k] fp32 from the filtered call against fp32 `scores` [M, N] of every
    pair and the eligibility [M, N]."""
    ids, got = ids.cpu(), got.cpu()
    M, N = scores.shape
    assert ids.shape == (M, k) and got.shape == (M, k)
    assert ((ids >= -1) & (ids < N)).all(), "ids out of range"
    valid = ids >= 0
    assert elig.gather(1, ids.clamp(min=0))[valid].all(), "a denied item was returned"
    n_elig = elig.sum(1, keepdim=True).clamp(max=k)
    pos = torch.arange(k).unsqueeze(0)
    assert (valid == (pos < n_elig)).all(), "the -1 tail is missing or too long"
    assert (got[~valid] == NEG_INF).all(), "the tail's scores are not -inf"
    want_ids, want_sc = expected_filtered(scores, elig, k)
    assert torch.equal(ids, want_ids), "an eligible item was displaced, or the order is not the total order"
    assert torch.equal(got.view(torch.int32), want_sc.to(torch.float32).view(torch.int32)), "score bits differ"


def differs_fraction(scores, elig, k):
    """Share of queries whose filtered expected list differs from their unfiltered one."""
    a = expected_filtered(scores, elig, k)[0]
    b = expected_filtered(scores, torch.ones_like(elig), k)[0]
    return float((a != b).any(1).sum()) / scores.shape[0]


def csr(lists, lead=0):
    """(values int64 [lead + sum of lengths], offsets int64 [M + 1] starting at `lead`): the lists
    in the order given (unsorted), behind `lead` values that belong to no query."""
    vals = [7] * lead + [x for l in lists for x in l]
    offs = [lead]
    for l in lists:
        offs.append(offs[-1] + len(l))
    return torch.tensor(vals, dtype=torch.int64), torch.tensor(offs, dtype=torch.int64)


def top_half(Q, Cm, k, bias=None):
    """The exact (fp64) top max(1, k / 2) item indices of every query: list of lists."""
    s, _ = ro.exact_scores(Q, Cm, bias)
    return ro.expected_topk(s, max(1, k // 2))[0].tolist()


def _rand_ids(g, N, n):
    return torch.randint(0, N, (n,), generator=g).tolist()


def _mask(g, N, p):
    return torch.rand(N, generator=g) < p


# ---- the cases: dict(Q, Cm, k, allow bool [N] or None, lists or None) ----------------------------


def case_own_topk():
    """Each query's exact top 100 excluded, k = 100: what is left is ranks 100..199. (The GPU test
    excludes the first 100 ids of its own unfiltered run; on fp64 scores these are the same idea.)"""
    M, N, E, k = 40, 3000, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 101)
    s, _ = ro.exact_scores(Q, Cm)
    return dict(Q=Q, Cm=Cm, k=k, allow=None, lists=ro.expected_topk(s, k)[0].tolist())


def case_mask_half():
    M, N, E, k = 17, 1037, 64, 10
    Q, Cm = ro.make_inputs(M, N, E, 102)
    return dict(Q=Q, Cm=Cm, k=k, allow=_mask(torch.Generator().manual_seed(1102), N, 0.5), lists=None)


def case_mask_last_only():
    M, N, E, k = 9, 129, 64, 16
    Q, Cm = ro.make_inputs(M, N, E, 103)
    allow = torch.zeros(N, dtype=torch.bool)
    allow[N - 1] = True
    return dict(Q=Q, Cm=Cm, k=k, allow=allow, lists=None)


def case_mask_none():
    M, N, E, k = 9, 300, 64, 16
    Q, Cm = ro.make_inputs(M, N, E, 104)
    return dict(Q=Q, Cm=Cm, k=k, allow=torch.zeros(N, dtype=torch.bool), lists=None)


SPLIT2_BOUNDARY = 1536  # first item of the second split at N = 3000, splits = 2, E = 64 (128-item chunks)


def case_list_shapes():
    """Query m's list by m % 8: 0 empty; 1 one item (its best); 2, 7 many; 3 duplicates and values
    outside [0, N); 4 a run across the boundary of two splits; 5 all N items; 6 all but 37 (fewer
    than k left)."""
    M, N, E, k = 40, 3000, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 105)
    top = top_half(Q, Cm, k)
    g = torch.Generator().manual_seed(1105)
    lists = []
    for m in range(M):
        kind = m % 8
        if kind == 0:
            l = []
        elif kind == 1:
            l = top[m][:1]
        elif kind in (2, 7):
            l = top[m] + _rand_ids(g, N, 200)
        elif kind == 3:
            l = top[m][:10] * 2 + [-5, -1, N, N + 7, 2 ** 31 - 1] + top[m][10:20]
        elif kind == 4:
            l = list(range(SPLIT2_BOUNDARY - 40, SPLIT2_BOUNDARY + 40)) + top[m]
        elif kind == 5:
            l = list(range(N))
        else:
            keep = set(_rand_ids(g, N, 37))
            l = [n for n in range(N) if n not in keep] + top[m][:3]
        lists.append(l)
    return dict(Q=Q, Cm=Cm, k=k, allow=None, lists=lists)


TOGETHER = [(E, k) for E in (32, 96, 128) for k in (1, 10, 256)]


def case_together(E, k):
    M, N = 33, 2000
    Q, Cm = ro.make_inputs(M, N, E, 106 + E + k)
    g = torch.Generator().manual_seed(1106 + E + k)
    top = top_half(Q, Cm, k)
    lists = [top[m][::2] + _rand_ids(g, N, 100) if m % 5 else [] for m in range(M)]
    return dict(Q=Q, Cm=Cm, k=k, allow=_mask(g, N, 0.6), lists=lists)


TIE_DUP = list(range(635, 642)) + list(range(900, 906))  # the duplicate rows of the unfiltered tie test


def case_ties():
    """13 copies of one dominant row: copies 635 and 900 denied to everyone by the mask, query m
    denied one of the first five by its list, every other query also 900 (again) and the last copy:
    the answer is the lowest eligible copies, ascending, 10 or 9 of them."""
    M, N, E, k = 17, 1037, 64, 10
    g = torch.Generator().manual_seed(41)
    u = torch.randn(E, generator=g) * 0.5
    Q = u + 0.05 * torch.randn(M, E, generator=g)
    Cm = torch.randn(N, E, generator=g) * 0.5
    Cm[TIE_DUP] = 2.0 * u
    allow = torch.ones(N, dtype=torch.bool)
    allow[[635, 900]] = False
    lists = [[TIE_DUP[1 + m % 4]] + ([TIE_DUP[7], TIE_DUP[12]] if m % 2 else []) for m in range(M)]
    return dict(Q=Q, Cm=Cm, k=k, allow=allow, lists=lists)


def case_monotone(reverse):
    """score(m, n) = (m + 1) n exactly (the unfiltered test's ramp), or its reverse; every other item
    masked and each query's last 50 items excluded."""
    M, N, E, k = 40, 3000, 64, 100
    n = torch.arange(N)
    Cm = torch.zeros(N, E)
    Cm[:, 0], Cm[:, 1] = (n & 63).float(), (n >> 6).float()
    Q = torch.zeros(M, E)
    Q[:, 0], Q[:, 1] = torch.arange(1, M + 1).float(), 64.0 * torch.arange(1, M + 1)
    if reverse:
        Cm = Cm.flip(0)
    allow = (n & 1) == 1
    return dict(Q=Q, Cm=Cm, k=k, allow=allow, lists=[list(range(N - 50, N))] * M)


def case_edge_129():
    """M = 129: one query past the 128-query tile, and only it has a list (the mask is what changes
    the other queries' lists)."""
    M, N, E, k = 129, 300, 64, 10
    Q, Cm = ro.make_inputs(M, N, E, 107)
    lists = [[] for _ in range(M)]
    lists[128] = top_half(Q, Cm, k)[128] + [3, 299]
    return dict(Q=Q, Cm=Cm, k=k, allow=_mask(torch.Generator().manual_seed(1107), N, 0.5), lists=lists)


def case_split_invariance():
    M, N, E, k = 40, 3000, 64, 100
    Q, Cm = ro.make_inputs(M, N, E, 108)
    g = torch.Generator().manual_seed(1108)
    top = top_half(Q, Cm, k)
    lists = [top[m] + _rand_ids(g, N, 300) for m in range(M)]
    return dict(Q=Q, Cm=Cm, k=k, allow=_mask(g, N, 0.5), lists=lists)


CASES = {
    "own_topk": case_own_topk,
    "mask_half": case_mask_half,
    "mask_last_only": case_mask_last_only,
    "mask_none": case_mask_none,
    "list_shapes": case_list_shapes,
    **{f"together_E{E}_k{k}": (lambda E=E, k=k: case_together(E, k)) for E, k in TOGETHER},
    "ties": case_ties,
    "monotone": lambda: case_monotone(False),
    "monotone_reverse": lambda: case_monotone(True),
    "edge_129": case_edge_129,
    "split_invariance": case_split_invariance,
}
