"""Cases and oracles of the target-rank tests (tests/test_gpu_ranks.py).

Exact oracle: for N <= 8192, ops.topk_mips_large(k = N) is each query's complete order of its eligible
items (ids in rank order, -1 past them), from the project's own selection kernels. A target's rank
must be its column, its score that column's bits; a target the list does not hold (out of range,
denied, excluded) has rank -1 and score -inf.

fp64 band (retrieval_oracle.exact_scores, no kernel involved): with s64 the exact scores of the
bf16-rounded rows and tol their error bounds, an eligible target's rank lies in [lo, hi],
lo = #{n: s64[n] > s64[t] + tol[t] + tol[n]}, hi = #{n != t: s64[n] >= s64[t] - tol[t] - tol[n]}.
"""
from __future__ import annotations

import torch

import retrieval_oracle as ro

R = 8  # targets per virtual query in csrc/rank.hip: the slab sizes worth testing sit around it

# (M, N, E) of the full-order test; the first has the jagged targets of 0..40 a query
SHAPES = [(130, 8000, 64), (17, 1037, 32), (33, 5000, 128), (40, 3000, 96), (1, 257, 64)]
# (M, N, E, T, seed) of the fp64 band test
BAND_CASES = [(40, 3000, 64, 8, 7001), (33, 5000, 128, 20, 7002), (17, 1037, 32, 3, 7003), (40, 3000, 96, 8, 7004)]


def csr(lists, lead=0, dtype=torch.int32):
    """(values [lead + sum of lengths], offsets int64 [M + 1] starting at `lead`)."""
    vals = [0] * lead + [x for l in lists for x in l]
    offs = [lead]
    for l in lists:
        offs.append(offs[-1] + len(l))
    return torch.tensor(vals, dtype=dtype), torch.tensor(offs, dtype=torch.int64)


def jagged_targets(M, N, seed, most=40):
    """0..most distinct targets a query; where there are queries enough: none, exactly R, R + 1,
    2 R + 2, and one with indices outside [0, N) among its targets."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for m in range(M):
        n = int(torch.randint(0, most + 1, (1,), generator=g))
        if M >= 5:
            n = {0: 0, 1: R, 2: R + 1, 3: 2 * R + 2}.get(m, n)
        out.append(torch.randperm(N, generator=g)[:min(n, N)].tolist())
    if M >= 5:
        out[4] = out[4][:3] + [N, -1, N + 77, -(1 << 31), (1 << 31) - 1] + out[4][3:]
    else:
        out[0] = [N, 0] + out[0] + [-1]
    return out


def expected_from_order(ids, scores, targets):
    """(ranks int64 [T], scores fp32 [T]) of the jagged `targets` from the complete order ids / scores
    [M, N] (CPU): the column that holds the target, else -1 / -inf."""
    M, N = ids.shape
    col = torch.full((M, N), -1, dtype=torch.int64)
    cols = torch.arange(N).repeat(M, 1)
    valid = ids >= 0
    col[torch.arange(M).unsqueeze(1).expand(M, N)[valid], ids[valid]] = cols[valid]
    ranks, sc = [], []
    for m, ts in enumerate(targets):
        for t in ts:
            c = int(col[m, t]) if 0 <= t < N else -1
            ranks.append(c)
            sc.append(float(scores[m, c]) if c >= 0 else float("-inf"))
    return torch.tensor(ranks, dtype=torch.int64), torch.tensor(sc, dtype=torch.float32)


def band(Q, C, targets, bias=None):
    """(lo, hi) int64 [T] of the fp64 band rule for the jagged in-range `targets`."""
    s, tol = ro.exact_scores(Q, C, bias)
    lo, hi = [], []
    for m, ts in enumerate(targets):
        for t in ts:
            above = s[m] > s[m, t] + tol[m, t] + tol[m]
            reach = s[m] >= s[m, t] - tol[m, t] - tol[m]
            reach[t] = False
            lo.append(int(above.sum()))
            hi.append(int(reach.sum()))
    return torch.tensor(lo), torch.tensor(hi)


def band_targets(M, N, T, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return [torch.randperm(N, generator=g)[:T].tolist() for _ in range(M)]
