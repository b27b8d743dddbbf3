"""IVF retrieval at real index sizes: the case table (test infrastructure, no GPU).

tt_ivf_scan declares 1 <= L <= 2^20 lists and 1 <= nprobe <= 64; the index is run with thousands of
lists. Each case below is the smallest index at which one run-time branch of csrc/ivf.hip exists (the
`branch` column). The table is shared by tests/test_gpu_ivf_scale.py (the kernels against the exact
filtered kernel) and tests/test_cpu_ivf_scale.py (which imports it, so that the assertions below run
without a GPU).

The module restates, as host arithmetic, what ivf.hip decides from the shape and the probes alone:
the lists one thread of ivf_offsets_kernel owns (`offsets_ranges`), the two exclusive scans
(`host_offsets`), the list scan's grid bound (`grid_bound`) and ivf_list_eligible_kernel's workgroups
and word loop (`mask_workgroups`, `mask_word_passes`). Every case is asserted on import to reach the
branch it is in the table for, so a later change to IVF_SCAN_THREADS, TK_QB or
IVF_MASK_LISTS_PER_WG cannot quietly make a case stop covering it (update the constants here with
ivf.hip, then re-pick the sizes).

Item and query rows come from retrieval_oracle.make_inputs; assignments and probes are drawn from
seeded generators and are functions of the case alone.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Tuple

import torch

import retrieval_oracle as ro

# csrc/ivf.hip and csrc/topk_scan.h constants the branches depend on
IVF_SCAN_THREADS = 1024       # ivf_offsets_kernel: one workgroup, thread t owns `per` lists
TK_QB = 128                   # pairs of one list per list-scan workgroup (a tile)
IVF_MASK_LISTS_PER_WG = 32    # ivf_list_eligible_kernel: one word of list_allow per workgroup
IVF_MAX_PROBE = 64
IVF_MAX_L = 1 << 20
MASK_WORDS_PER_PASS = 64      # ivf_list_eligible_kernel: a lane per word, `wd += 64`
LIST_ALIGN = 128              # ivf.LIST_ALIGN: IVFIndex.from_assignment's list alignment
CHUNK_ROWS_E64 = 128          # topk_scan.h: the rows of one staged chunk at E = 64 (64 at E = 128)

JUNK = (-1, None, 2 ** 31 - 1)  # probe values that are no probe; None stands for L itself


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def per_thread(L: int) -> int:
    """ivf_offsets_kernel's `per`."""
    return _cdiv(L, IVF_SCAN_THREADS)


def offsets_ranges(L: int):
    """(lo, hi) of every thread of ivf_offsets_kernel: lo = min(L, tid * per), hi = min(L, lo + per)."""
    per = per_thread(L)
    lo = torch.clamp(torch.arange(IVF_SCAN_THREADS) * per, max=L)
    return lo, torch.clamp(lo + per, max=L)


def grid_bound(M: int, nprobe: int, L: int) -> int:
    """The list scan's grid: full tiles, plus one partial tile per probed list."""
    PN = M * nprobe
    return _cdiv(PN, TK_QB) + min(L, PN)


def pair_counts(probes: torch.Tensor, L: int) -> torch.Tensor:
    """ivf_count_kernel: pairs per list; a value outside [0, L) is no probe."""
    p = probes.to(torch.int64).flatten()
    return torch.bincount(p[(p >= 0) & (p < L)], minlength=L)


def host_offsets(cnt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(list_off, tile_off) int64 [L + 1]: the exclusive scans of cnt and of ceil(cnt / TK_QB)."""
    zero = torch.zeros(1, dtype=torch.int64)
    return (torch.cat([zero, cnt.cumsum(0)]), torch.cat([zero, ((cnt + TK_QB - 1) // TK_QB).cumsum(0)]))


def mask_workgroups(L: int) -> int:
    return _cdiv(L, IVF_MASK_LISTS_PER_WG)


def mask_word_passes(begin: int, length: int) -> int:
    """Iterations of ivf_list_eligible_kernel's word loop for lane 0 over one list's rows."""
    if length <= 0:
        return 0
    return _cdiv(((begin + length - 1) >> 5) - (begin >> 5) + 1, MASK_WORDS_PER_PASS)


@dataclass(frozen=True)
class Case:
    id: str
    L: int
    N: int
    E: int
    M: int
    k: int
    nprobes: tuple
    branch: str          # what the case exists for
    per: int             # expected `per` of ivf_offsets_kernel (asserted below)
    focus: int           # the list the mask tests empty except for its last row

    @property
    def seed(self) -> int:
        return 7000 + self.L % 1000 + self.N

    def inputs(self):
        """(Q fp32 [M, E], items fp32 [N, E]) on the CPU."""
        return ro.make_inputs(self.M, self.N, self.E, self.seed)


BIG, BIG_ITEMS = 7, 5000               # many-lists: the list every query probes
EMPTY_LO, EMPTY_HI = 100, 1100         # many-lists: lists [100, 1100) hold no item
SINGLE_LO, SINGLE_HI = 1100, 1160      # many-lists: lists [1100, 1160) hold exactly one item
EMPTY_PROBED = 300                     # many-lists: only lists [100, 400) of the empty ones are ever probed
POOL = 800                             # many-lists: the lists the free probe columns draw from, none of them in [100, 1160)
LONE_ROW, LONE_COL = 11, 6             # many-lists: the pair that probes a list no other query probes
JUNK_ROWS = (3, 77, 150, 299)          # many-lists: rows that carry JUNK in JUNK_COLS (before the rotation)
JUNK_COLS = (3, 5, 7)

CASES = [
    Case("many-lists", 2500, 30_000, 64, 300, 50, (1, 8, 33, 64),
         "per = 3 with clipped trailing threads, a partial list_allow word, 1000 equal offsets in a row, "
         "a list of 5000 rows under three tiles, 33 and 64 merge lanes, a grid of thousands that is no multiple of 8",
         per=3, focus=BIG),
    Case("l-1024", 1024, 3000, 32, 40, 20, (4,), "the last size with per = 1: every thread owns one list",
         per=1, focus=1023),
    Case("l-1025", 1025, 3000, 32, 40, 20, (4,), "the first size with per = 2: thread 512 owns list 1024 alone, 511 threads idle",
         per=2, focus=1024),
    Case("l-max", IVF_MAX_L, 2000, 32, 40, 20, (4,), "L = 2^20, the declared limit: per = 1024, offsets up to list 2^20 - 1",
         per=1024, focus=IVF_MAX_L - 1),
]
BY_ID = {c.id: c for c in CASES}


# ---- assignments -------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def assignment(cid: str) -> torch.Tensor:
    """int64 [N]: every item's list."""
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(c.seed + 1)
    if cid == "many-lists":
        singles = SINGLE_HI - SINGLE_LO
        rest = torch.tensor([l for l in range(c.L) if l != BIG and not EMPTY_LO <= l < SINGLE_HI])
        perm = torch.randperm(c.N, generator=g)
        assign = torch.empty(c.N, dtype=torch.int64)
        assign[perm[:BIG_ITEMS]] = BIG
        assign[perm[BIG_ITEMS:BIG_ITEMS + singles]] = torch.arange(SINGLE_LO, SINGLE_HI)
        n_rest = c.N - BIG_ITEMS - singles
        assign[perm[BIG_ITEMS + singles:]] = rest[torch.randint(0, rest.numel(), (n_rest,), generator=g)]
        return assign
    if cid == "l-max":
        lists = torch.randperm(c.L - 1, generator=g)[:c.N - 1].sort().values
        return torch.cat([lists, torch.tensor([c.L - 1])])  # one item per list, list 2^20 - 1 among them
    assign = torch.randint(0, c.L, (c.N,), generator=g)
    assign[:3] = 1023
    assign[3:6] = c.L - 1
    return assign


def list_sizes(cid: str) -> torch.Tensor:
    return torch.bincount(assignment(cid), minlength=BY_ID[cid].L)


# ---- probes ------------------------------------------------------------------------------------


def _distinct_from(pool: torch.Tensor, M: int, n: int, taken: torch.Tensor, g) -> torch.Tensor:
    """int64 [M, n]: per row n distinct values of `pool` that are not in the row of `taken` [M, t]."""
    score = torch.rand(M, pool.numel(), generator=g)
    score[(pool.view(1, -1, 1) == taken.unsqueeze(1)).any(-1)] = 2.0
    return pool[score.argsort(1)[:, :n]]


def lone_list(cid: str = "many-lists") -> int:
    """A list with items that lies outside the pool of the free columns: probed by LONE_ROW alone."""
    sizes = list_sizes(cid)
    pool = set(_pool(cid).tolist())
    return next(l for l in range(SINGLE_HI, BY_ID[cid].L) if l not in pool and sizes[l] > 1)


@functools.lru_cache(maxsize=None)
def _pool(cid: str) -> torch.Tensor:
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(c.seed + 2)
    others = torch.tensor([l for l in range(c.L) if l != BIG and not EMPTY_LO <= l < SINGLE_HI])
    return others[torch.randperm(others.numel(), generator=g)[:POOL]].sort().values


@functools.lru_cache(maxsize=None)
def probes(cid: str, nprobe: int) -> torch.Tensor:
    """int32 [M, nprobe], distinct within a row (JUNK values aside, which are no probes)."""
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(c.seed + 100 + nprobe)
    M, L = c.M, c.L
    if cid == "many-lists":
        big = torch.full((M, 1), BIG, dtype=torch.int64)
        if nprobe == 1:
            return big.to(torch.int32)
        # columns: the big list, an empty list, a 1-item list, then free draws from the pool; each row is
        # then rotated by its index, so that every lane of the merge holds the big list for some query
        empty = torch.randint(EMPTY_LO, EMPTY_LO + EMPTY_PROBED, (M, 1), generator=g)
        single = torch.randint(SINGLE_LO, SINGLE_HI, (M, 1), generator=g)
        fixed = torch.cat([big, empty, single], 1)
        p = torch.cat([fixed, _distinct_from(_pool(cid), M, nprobe - 3, fixed, g)], 1)
        p[LONE_ROW, LONE_COL] = lone_list(cid)
        for r in JUNK_ROWS:
            p[r, list(JUNK_COLS)] = torch.tensor([v if v is not None else L for v in JUNK])
        shift = (torch.arange(nprobe).view(1, -1) - torch.arange(M).view(-1, 1)) % nprobe
        return p.gather(1, shift).to(torch.int32).contiguous()
    if cid == "l-max":
        occupied = assignment(cid)
        p = torch.cat([occupied[torch.rand(M, c.N, generator=g).argsort(1)[:, :nprobe - 1]],
                       torch.randint(0, L, (M, 1), generator=g)], 1)  # the last column: most likely an empty list
        p[::5, 1] = L - 1
        p[1::5, 0] = occupied[0]
        return p.to(torch.int32).contiguous()
    pool = torch.tensor([l for l in range(L) if l not in (1023, L - 1)])
    p = _distinct_from(pool, M, nprobe, torch.full((M, 1), -1), g)
    p[0::3, 1] = 1023
    p[1::3, 2] = L - 1
    return p.to(torch.int32).contiguous()


def permuted(p: torch.Tensor, seed: int) -> torch.Tensor:
    """The same probes with the columns of each row in another order."""
    g = torch.Generator().manual_seed(seed)
    return p.gather(1, torch.rand(p.shape, generator=g).argsort(1)).contiguous()


def reachable(cid: str, nprobe: int) -> torch.Tensor:
    """int64 [M]: the items of each query's probed lists."""
    c = BY_ID[cid]
    p = probes(cid, nprobe).to(torch.int64)
    ok = (p >= 0) & (p < c.L)
    return (list_sizes(cid)[p.clamp(0, c.L - 1)] * ok).sum(1)


# ---- masks -------------------------------------------------------------------------------------

LIVE_LISTS = 40


def live_lists(cid: str) -> torch.Tensor:
    """The LIVE_LISTS lists the third mask leaves eligible rows in: the focus list, list 1023 or a
    1-item list, and a seeded choice of the other lists that hold items."""
    c = BY_ID[cid]
    sizes = list_sizes(cid)
    must = [c.focus, SINGLE_LO if cid == "many-lists" else 1023]
    g = torch.Generator().manual_seed(c.seed + 3)
    others = torch.tensor([l for l in (sizes > 0).nonzero().flatten().tolist() if l not in must])
    pick = others[torch.randperm(others.numel(), generator=g)[:LIVE_LISTS - len(must)]]
    return torch.cat([torch.tensor(must), pick]).sort().values


@functools.lru_cache(maxsize=None)
def mask(cid: str, kind: str) -> torch.Tensor:
    """bool [N]. "half": a random half; "focus-last": every item but those of the focus list, of which
    only the one of highest index (the list's last row) stays; "live-40": a random half of the items
    of LIVE_LISTS lists (at least the first item of each), nothing else."""
    c = BY_ID[cid]
    assign = assignment(cid)
    g = torch.Generator().manual_seed(c.seed + 4)
    half = torch.rand(c.N, generator=g) < 0.5
    if kind == "half":
        return half
    if kind == "focus-last":
        m = assign != c.focus
        m[(assign == c.focus).nonzero().flatten()[-1]] = True
        return m
    assert kind == "live-40"
    live = live_lists(cid)
    inside = (assign.view(-1, 1) == live.view(1, -1)).any(1)
    m = inside & half
    for l in live.tolist():
        m[(assign == l).nonzero().flatten()[0]] = True
    return m


MASK_KINDS = ("half", "focus-last", "live-40")


# ---- a hand-made layout for tt_ivf_mask_lists -----------------------------------------------------

# (list_begin, list_len) over HAND_P packed rows: lists begin at rows that are no multiple of 32 and end
# inside a word; list 1 is longer than 2048 rows (lane 0 takes a second word pass); list 0 lies within
# one word (head and tail mask on the same word); list 3 is one row, the last bit of a word; list 5
# ends on the last row; list 6 reaches one row past P and list 7 begins past P (no eligible row);
# list 8 is empty; lists 9.. are 3 rows each at odd places, so that L = 37 needs a second workgroup
# and a partial list_allow word
HAND_P = 6001
HAND_LISTS = [(5, 20), (37, 2500), (2537, 59), (2623, 1), (2700, 1300), (4002, HAND_P - 4002), (5990, 12),
              (HAND_P + 3, 4), (100, 0)] + [(4000 - 7 * i, 3) for i in range(1, 29)]
HAND_N = 5000


def hand_layout():
    """(labels int32 [HAND_P], list_begin int64 [L], list_len int32 [L]): labels are a seeded draw from
    [-3, HAND_N + 3): a few are no item. The lists overlap, which tt_ivf_mask_lists does not mind."""
    g = torch.Generator().manual_seed(4242)
    labels = torch.randint(-3, HAND_N + 3, (HAND_P,), generator=g).to(torch.int32)
    begin = torch.tensor([b for b, _ in HAND_LISTS], dtype=torch.int64)
    length = torch.tensor([n for _, n in HAND_LISTS], dtype=torch.int32)
    return labels, begin, length


# ---- the eligibility oracle through an [M, L] table ---------------------------------------------------


def eligibility_by_list(assign, probes, nlist, dead_lists=()):
    """ivf_cases.eligibility_for_probes without its [M, N, nprobe] intermediate: bool [M, N], item n is
    in one of query m's probed lists, as probed[m, assign[n]] of a bool [M, nlist] table. Probe values
    outside [0, nlist), and the lists in `dead_lists`, count for nothing."""
    p = probes.to(torch.int64)
    ok = (p >= 0) & (p < nlist)
    for d in dead_lists:
        ok &= p != d
    probed = torch.zeros(p.shape[0], nlist + 1, dtype=torch.bool)
    probed.scatter_(1, torch.where(ok, p, torch.full_like(p, nlist)), True)
    return probed[:, :nlist].index_select(1, assign.to(torch.int64))


# ---- every case reaches its branch ------------------------------------------------------------------


def check_case(c: Case) -> None:
    """Host arithmetic only: the case reaches the branches it is in the table for."""
    L, sizes = c.L, list_sizes(c.id)
    assert 1 <= L <= IVF_MAX_L and c.E % 32 == 0 and 32 <= c.E <= 128 and 1 <= c.k <= 256, c.id
    assert per_thread(L) == c.per, (c.id, per_thread(L))
    assert int(sizes.sum()) == c.N and int(sizes[c.focus]) > 0, c.id
    for nprobe in c.nprobes:
        assert 1 <= nprobe <= IVF_MAX_PROBE, c.id
        p = probes(c.id, nprobe)
        assert p.shape == (c.M, nprobe) and p.dtype == torch.int32, c.id
        live = (p >= 0) & (p < L)
        srt = torch.where(live, p, -1 - torch.arange(nprobe, dtype=torch.int32)).sort(1).values
        assert (srt.diff(dim=1) != 0).all(), (c.id, nprobe, "probes repeat within a row")
        tiles = int(host_offsets(pair_counts(p, L))[1][-1])
        assert tiles <= grid_bound(c.M, nprobe, L), (c.id, nprobe)
        # a case with nprobe = 64 stays at E <= 64 (run time)
        assert nprobe < 64 or c.E <= 64, c.id


for _c in CASES:
    check_case(_c)


def _check_many_lists() -> None:
    c = BY_ID["many-lists"]
    L, sizes = c.L, list_sizes(c.id)
    lo, hi = offsets_ranges(L)
    # per = 3: full ranges, one clipped range (L % per != 0), and trailing threads with lo = hi = L
    assert c.per >= 2 and L % c.per and L % IVF_MASK_LISTS_PER_WG
    assert int((hi - lo == c.per).sum()) == L // c.per and int(((hi - lo > 0) & (hi - lo < c.per)).sum()) == 1
    assert int((lo == L).sum()) >= 100 and int(hi.max()) == L
    assert mask_workgroups(L) > 1
    # the assignment
    assert int(sizes[BIG]) == BIG_ITEMS > 4096 and (sizes[EMPTY_LO:EMPTY_HI] == 0).all() and EMPTY_HI - EMPTY_LO == 1000
    assert int((sizes == 1).sum()) >= 50 and (sizes[SINGLE_LO:SINGLE_HI] == 1).all()
    assert mask_word_passes(0, BIG_ITEMS) >= 2, "the big list needs a second pass of the mask word loop"
    assert c.E == 64 and BIG_ITEMS // CHUNK_ROWS_E64 >= 24, "dozens of chunks"
    assert c.nprobes == (1, 8, 33, 64)
    bounds = [grid_bound(c.M, n, L) for n in c.nprobes]
    assert any(b % 8 for b in bounds) and all(b > 300 for b in bounds), bounds
    assert max(bounds) > 2000 and grid_bound(c.M, 64, L) % 8
    for nprobe in c.nprobes:
        p = probes(c.id, nprobe)
        cnt = pair_counts(p, L)
        list_off, tile_off = host_offsets(cnt)
        # list 7: tiles of 128, 128 and 44 pairs
        assert int(cnt[BIG]) == c.M == 300 and int(tile_off[BIG + 1] - tile_off[BIG]) == 3 and c.M - 2 * TK_QB == 44
        assert ((p == BIG).sum(1) == 1).all()
        # most workgroups of the grid leave at once
        assert int(tile_off[-1]) * 5 < 4 * grid_bound(c.M, nprobe, L), (nprobe, int(tile_off[-1]))
        if nprobe == 1:
            continue
        pl = p.to(torch.int64)
        live = (pl >= 0) & (pl < L)
        sz = torch.where(live, sizes[pl.clamp(0, L - 1)], torch.full_like(pl, -1))
        assert ((sz == 0).sum(1) >= 1).all() and ((sz == 1).sum(1) >= 1).all(), nprobe
        assert int(cnt[lone_list()]) == 1 and int(sizes[lone_list()]) > 1, nprobe
        assert int((cnt == 0).sum()) >= 1000, (nprobe, "many lists are probed by none")
        # a run of hundreds of equal tile offsets (lists nobody probes) for the binary search to cross
        flat = (tile_off.diff() == 0).to(torch.int64)
        run = best = 0
        for v in flat.tolist():
            run = run + 1 if v else 0
            best = max(best, run)
        assert best >= EMPTY_HI - EMPTY_LO - EMPTY_PROBED >= 500, (nprobe, best)
        # junk between live columns, in each junk row
        for r in JUNK_ROWS:
            row = p[r].tolist()
            junk = [j for j, v in enumerate(row) if not 0 <= v < L]
            assert sorted(row[j] for j in junk) == [-1, L, 2 ** 31 - 1], (nprobe, r)
            lives = [j for j, v in enumerate(row) if 0 <= v < L]
            assert any(min(lives) < j < max(lives) for j in junk), (nprobe, r)
        # the merge: the big list sits in every lane for some query, lanes 32..63 included
        lanes = (p == BIG).to(torch.int64).argmax(1)
        assert set(lanes.tolist()) == set(range(nprobe)), nprobe
    # rows with fewer than k reachable items (the guard test's tail) exist at nprobe = 8, not at 1
    assert int((reachable(c.id, 1) < c.k).sum()) == 0
    # the masks
    assert int((list_sizes(c.id)[live_lists(c.id)] > 0).sum()) == LIVE_LISTS
    assert BIG in live_lists(c.id).tolist()


def _check_boundary() -> None:
    a, b = BY_ID["l-1024"], BY_ID["l-1025"]
    assert a.L == IVF_SCAN_THREADS and b.L == IVF_SCAN_THREADS + 1
    lo, hi = offsets_ranges(a.L)
    assert (hi - lo == 1).all()
    lo, hi = offsets_ranges(b.L)
    assert b.per == 2 and int((hi - lo == 2).sum()) == 512 and int((hi - lo == 1).sum()) == 1
    assert int(lo[512]) == 1024 and int(hi[512]) == 1025 and (lo[513:] == b.L).all()
    for c in (a, b):
        sizes = list_sizes(c.id)
        cnt = pair_counts(probes(c.id, 4), c.L)
        for l in (1023, c.L - 1):
            assert sizes[l] > 0 and cnt[l] > 0, (c.id, l)
        assert int((list_sizes(c.id)[live_lists(c.id)] > 0).sum()) == LIVE_LISTS
    assert b.L % IVF_MASK_LISTS_PER_WG == 1 and mask_workgroups(b.L) == 33


def _check_max() -> None:
    c = BY_ID["l-max"]
    assert c.L == IVF_MAX_L == 1 << 20 and c.per == IVF_SCAN_THREADS
    sizes = list_sizes(c.id)
    assert int((sizes == 1).sum()) == c.N and int(sizes[c.L - 1]) == 1
    occupied = sizes.nonzero().flatten()
    assert int(occupied[0]) < c.L // 64 and int((occupied > c.L // 2).sum()) > c.N // 4  # across the whole range
    cnt = pair_counts(probes(c.id, 4), c.L)
    assert int(cnt[c.L - 1]) >= 1
    probed = cnt.nonzero().flatten()
    owners = torch.unique(probed // c.per)
    assert owners.numel() > 50 and int(owners.max()) == IVF_SCAN_THREADS - 1  # many threads hold a pair, the last too


_check_many_lists()
_check_boundary()
_check_max()


def hand_checks() -> None:
    """The hand-made mask layout reaches the head / tail masks and the strided word loop."""
    assert any(b & 31 for b, n in HAND_LISTS if n > 0) and any((b + n) & 31 for b, n in HAND_LISTS if n > 0)
    assert mask_word_passes(*HAND_LISTS[1]) == 2 and HAND_LISTS[1][1] > 2048
    assert HAND_LISTS[0][0] >> 5 == (HAND_LISTS[0][0] + HAND_LISTS[0][1] - 1) >> 5  # one word: both masks apply
    assert HAND_LISTS[3][1] == 1 and HAND_LISTS[3][0] & 31 == 31
    assert sum(HAND_LISTS[5]) == HAND_P and sum(HAND_LISTS[6]) == HAND_P + 1 and HAND_LISTS[7][0] > HAND_P
    assert mask_workgroups(len(HAND_LISTS)) == 2 and len(HAND_LISTS) % IVF_MASK_LISTS_PER_WG


hand_checks()
