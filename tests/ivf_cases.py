"""Inputs shared by the IVF tests (tests/test_cpu_ivf.py, tests/test_gpu_ivf.py).

The oracle of the list scan is the exact kernel itself: a query that is denied every item outside its
probed lists (and its seen items) through the exclusion list of ops.topk_mips must get the same ids
and the same score bits. `exclusion_for_probes` builds those lists on the CPU.

`mixture` is a separated Gaussian mixture on which recall 1.0 at nprobe = 1 follows by construction:
C centres 6 e_c, noise sigma = 0.05 per coordinate (|noise| about 0.05 sqrt(E) = 0.28 at E = 32), so
two clusters are about 6 sqrt(2) = 8.5 apart, far beyond the noise and the bf16 rounding (relative
2^-9 of values up to about 6: 0.012 per coordinate)."""
from __future__ import annotations

import torch


def eligibility_for_probes(assign, probes, nlist, dead_lists=()):
    """bool [M, N]: item n is in one of query m's probed lists. assign int64 [N] (the item's list),
    probes int [M, nprobe]; probe values outside [0, nlist), and the lists in `dead_lists`, count
    for nothing."""
    p = probes.to(torch.int64)
    ok = (p >= 0) & (p < nlist)
    for d in dead_lists:
        ok &= p != d
    p = torch.where(ok, p, torch.full_like(p, -1))
    return (assign.view(1, -1, 1) == p.unsqueeze(1)).any(-1)


def exclusion_from_eligibility(elig, seen=None):
    """(values int32, offsets int64 [M + 1]): per query the ascending items that are not eligible,
    united with its `seen` list (a list of lists of item rows)."""
    elig = elig.clone()
    if seen is not None:
        for m, l in enumerate(seen):
            v = torch.tensor([x for x in l if 0 <= x < elig.shape[1]], dtype=torch.int64)
            elig[m, v] = False
    denied = ~elig
    values = denied.nonzero()[:, 1].to(torch.int32)  # row-major: ascending within a query
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), denied.sum(1).cumsum(0)])
    return values, offsets


def distinct_probes(M, nlist, nprobe, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(M, nlist, generator=g).argsort(1)[:, :nprobe].to(torch.int32).contiguous()


MIX_C, MIX_E, MIX_PER, MIX_SIGMA, MIX_QPC = 16, 32, 200, 0.05, 4


def mixture(seed=7):
    """(items fp32 [3200, 32], item cluster int64 [3200], queries fp32 [64, 32], query cluster,
    init int64 [16]: one item row per cluster)."""
    g = torch.Generator().manual_seed(seed)
    N = MIX_C * MIX_PER
    cluster = torch.arange(N) % MIX_C
    cluster = cluster[torch.randperm(N, generator=g)]
    centres = 6.0 * torch.eye(MIX_C, MIX_E)
    items = centres[cluster] + MIX_SIGMA * torch.randn(N, MIX_E, generator=g)
    qcluster = torch.arange(MIX_C * MIX_QPC) % MIX_C
    queries = centres[qcluster] + MIX_SIGMA * torch.randn(qcluster.numel(), MIX_E, generator=g)
    init = torch.stack([(cluster == c).nonzero()[0, 0] for c in range(MIX_C)])
    return items, cluster, queries, qcluster, init
