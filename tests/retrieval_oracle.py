"""fp64 oracle of exact top-k retrieval (tt_topk_mips) and the rule its results are judged by.

The kernel rounds fp32 operands to bf16 and sums the E products of a pair in fp32 (bf16 products are
exact in fp32), so against the fp64 score of the SAME bf16-rounded rows its error is that of E - 1
fp32 additions: |s - s64| <= tol(m, n) = E * 2^-24 * sum_e |Q[m, e]| |C[n, e]| (the textbook bound
(n - 1) u sum|x_i|, u = 2^-24, rounded up to E). With a bias there is one more addition and the
bias in the sum: tol = (E + 1) * 2^-24 * (sum_e |q||c| + |bias[n]|).

Band rule: with tau the exact k-th best score of a query, every item whose exact score exceeds
tau + tol must be returned, no returned item may be below tau - tol, and items inside the band may
go either way. `band_fraction` is the share of queries that have any item OTHER than the k-th best
itself inside the band: the rule only bites where that share is small.
"""
from __future__ import annotations

import torch

U = 2.0 ** -24

# (M, N, E, k) of the GPU score / selection test; inputs are randn * 0.5 from the case's seed
CASES = [(40, 3000, 64, 100), (17, 1037, 32, 10), (33, 5000, 128, 256), (40, 3000, 96, 100), (1, 257, 64, 1)]
L2_CASE = (24, 2000, 64, 50)


def make_inputs(M, N, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, E, generator=g) * 0.5, torch.randn(N, E, generator=g) * 0.5


def case_inputs(i):
    M, N, E, k = CASES[i]
    return make_inputs(M, N, E, 1000 + i)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float64)


def exact_scores(Q, C, bias=None):
    """(scores fp64 [M, N], tol fp64 [M, N]) of the bf16-rounded operands."""
    q, c = bf16_round(Q.cpu()), bf16_round(C.cpu())
    E = q.shape[1]
    s = q @ c.T
    mag = q.abs() @ c.abs().T
    if bias is None:
        return s, E * U * mag
    b = bias.cpu().to(torch.float64)
    return s + b, (E + 1) * U * (mag + b.abs())


def l2_bias64(C):
    c = bf16_round(C.cpu())
    return -0.5 * (c * c).sum(1)


def expected_topk(scores, k):
    """(ids, scores) under the total order: higher score first, equal scores by lower index."""
    v, i = torch.sort(scores, dim=1, descending=True, stable=True)
    return i[:, :k], v[:, :k]


def kth_best(scores, k):
    N = scores.shape[1]
    if N < k:
        return torch.full((scores.shape[0],), float("-inf"), dtype=scores.dtype)
    return torch.sort(scores, dim=1, descending=True).values[:, k - 1]


def band_fraction(scores, tol, k):
    """Share of queries with an item other than the k-th best itself within tol of tau."""
    tau = kth_best(scores, k).unsqueeze(1)
    inside = ((scores - tau).abs() <= tol).sum(1)
    return float((inside > 1).sum()) / scores.shape[0]


def check_band(ids, got, scores, tol, k):
    """Assert the band rule, the score tolerance, distinct in-range ids and the sorted order for
    returned (ids [M, k] int64, got [M, k] fp32) against exact (scores, tol) [M, N]."""
    ids, got = ids.cpu(), got.cpu()
    M, N = scores.shape
    kk = min(k, N)
    assert ids.shape == (M, k) and got.shape == (M, k)
    if N < k:
        assert (ids[:, N:] == -1).all() and (got[:, N:] == float("-inf")).all()
    ids, got = ids[:, :kk], got[:, :kk].to(torch.float64)
    assert ((ids >= 0) & (ids < N)).all(), "ids out of range"
    assert (torch.sort(ids, dim=1).values.diff(dim=1) > 0).all(), "ids repeat"
    err = (got - scores.gather(1, ids)).abs()
    assert (err <= tol.gather(1, ids)).all(), f"score error {float((err / tol.gather(1, ids)).max()):.3f} of the bound"
    d = got.diff(dim=1)
    assert (d <= 0).all(), "scores not descending"
    assert ((d < 0) | (ids.diff(dim=1) > 0)).all(), "equal scores not by ascending index"
    tau = kth_best(scores, kk).unsqueeze(1)
    returned = torch.zeros(M, N, dtype=torch.bool)
    returned.scatter_(1, ids, True)
    must = scores > tau + tol
    assert (returned | ~must).all(), "an item above the band was not returned"
    assert not (returned & (scores < tau - tol)).any(), "an item below the band was returned"
