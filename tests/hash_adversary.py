"""Adversarial inputs for the grouping hash tables (test infrastructure; CPU only, numpy — no GPU
call in this module; tests/test_cpu_hash_adversary.py checks every routine and pins every
restatement below to the csrc/ text, tests/test_gpu_hash_adversary.py feeds the batches to the kernels).

The embedding update groups a step's lookups by unique (table, row) in open-addressed tables with
linear probing, one compare-and-swap per probe, wrapping at cap - 1:

  1. the dedup global table        dd_insert* (csrc/dedup.h), cap = dedup_cap(max_lookups) 128-B slots
  2. the ring insert role's LDS    insert_next_full_block (csrc/tower_tail.hip), INS_HS slots per workgroup
  3. the KJT-form global table     hash_insert / bwd_tile_hash_kernel (csrc/embedding.hip), bwd_cap()
  4. the KJT-form chunk LDS table  bwd_tile_hash_kernel, TILE_HS slots per chunk of <= TILE_CH lookups
  5. the deferred-insert resolver  dd_insert_defer_finish_at / dd_resolve_block: table 1 again

With uniform or Zipf ids the load factors (<= 1/16, <= 1/2) make a probe chain longer than two rare
and a chain through cap - 1 -> 0 practically absent. The routines here derive, from a restatement of
the kernels' hash, row ids that collide on purpose; the batches never exceed the lookups a workspace
was sized for, so probing terminates by design: long chains, never a full table."""
from __future__ import annotations

from dataclasses import dataclass, field
from math import gcd
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# ---- the restated hash, key packings and sizes (pinned by test_cpu_hash_adversary.py) --------------

MIX_MUL1 = 0xFF51AFD7ED558CCD  # csrc/dedup.h dd_mix64 (line 77) = csrc/embedding.hip mix64 (line 200)
MIX_MUL2 = 0xC4CEB9FE1A85EC53  # csrc/dedup.h dd_mix64 (line 79) = csrc/embedding.hip mix64 (line 202)
MIX_SHIFT = 33                 # the three x ^= x >> 33 of both mixers (dedup.h 76/78/80, embedding.hip 199/201/203)

DD_TABLE_SHIFT = 40   # csrc/dedup.h line 18: dedup key = table << 40 | row
DD_CNT_BITS = 18      # csrc/dedup.h line 19: slot word = key << 18 | count
DD_INL = 30           # csrc/dedup.h line 21: lookups stored inline; a row with more is hot
PK_ROW_BITS = 34      # csrc/embedding.hip line 190: KJT-form key = table << 34 | row
PK_CNT_BITS = 24      # csrc/embedding.hip line 189: slot word = key << 24 | count
HOT_MIN = 33          # csrc/embedding.hip line 210: KJT form, rows with >= 33 lookups are hot
HOT_SPLIT = 512       # csrc/embedding.hip line 214: a hot row above it is split into bag-id ranges
TILE_BAGS = 16        # csrc/embedding.hip line 222: bags per workgroup of bwd_tile_hash_kernel
TILE_CH = 1024        # csrc/embedding.hip line 223: lookups per chunk
TILE_HS = 2048        # csrc/embedding.hip line 224: LDS hash slots per chunk
INS_HS = 1024         # csrc/tower_tail.hip line 992: LDS hash slots of one ring insert workgroup
INS_GROUP = 256       # csrc/tower_tail.hip insert_next_full_block: INS_PT = 1 lookup per thread, 256 threads
DEDUP_CAP_MIN, DEDUP_CAP_FACTOR = 1024, 16  # csrc/dedup.hip dedup_cap (line 34): c = 1024; while (c < 16 * L)
BWD_CAP_MIN, BWD_CAP_FACTOR = 4096, 2       # csrc/embedding.hip bwd_cap (line 264): c = SCAN_TILE; while (c < 2 * L)
MAX_FAMILY = 96       # keys asked of one home slot: every slot has more candidates among 2^21 rows

_U64 = np.uint64


def mix64(x) -> np.ndarray:
    """The murmur3 finalizer of both tables, on uint64 arrays (wrap-around arithmetic)."""
    x = np.atleast_1d(np.asarray(x)).astype(_U64).copy()
    x ^= x >> _U64(MIX_SHIFT)
    x *= _U64(MIX_MUL1)
    x ^= x >> _U64(MIX_SHIFT)
    x *= _U64(MIX_MUL2)
    x ^= x >> _U64(MIX_SHIFT)
    return x


def dd_key(table: int, rows) -> np.ndarray:
    """csrc/dedup.hip dd_insert_cols_kernel (line 88): table << DD_TABLE_SHIFT | row."""
    return (_U64(table) << _U64(DD_TABLE_SHIFT)) | np.atleast_1d(np.asarray(rows)).astype(_U64)


def pk_key(table: int, rows) -> np.ndarray:
    """csrc/embedding.hip pk_key (line 192): table << PK_ROW_BITS | row."""
    return (_U64(table) << _U64(PK_ROW_BITS)) | np.atleast_1d(np.asarray(rows)).astype(_U64)


def dedup_cap(L: int) -> int:
    """csrc/dedup.hip dedup_cap (line 34): slots of the dedup table of a workspace for L lookups."""
    c = DEDUP_CAP_MIN
    while c < DEDUP_CAP_FACTOR * L:
        c <<= 1
    return c


def bwd_cap(L: int) -> int:
    """csrc/embedding.hip bwd_cap (line 264): slots of the KJT-form table of a workspace for L lookups."""
    c = BWD_CAP_MIN
    while c < BWD_CAP_FACTOR * L:
        c <<= 1
    return c


def home(keys, cap: int) -> np.ndarray:
    """Home slot of packed keys in a table of cap slots (cap a power of two: global or LDS)."""
    assert cap & (cap - 1) == 0
    return (mix64(keys) & _U64(cap - 1)).astype(np.int64)


# ---- families ----------------------------------------------------------------------------------------

_HASHES: dict = {}


def _row_hashes(table: int, N: int, pack: Callable) -> np.ndarray:
    """mix64 of the packed key of every row of [0, N) (kept: a family search is one mask over it)."""
    k = (pack.__name__, int(table), int(N))
    if k not in _HASHES:
        _HASHES[k] = mix64(pack(table, np.arange(N, dtype=np.int64)))
    return _HASHES[k]


def family(table: int, N: int, cap: int, home_slot: int, size: int, pack: Callable = dd_key,
           skip: int = 0) -> np.ndarray:
    """``size`` distinct rows of [1, N) whose packed key's home slot is ``home_slot`` (the first ones
    in ascending row order after ``skip`` candidates)."""
    assert size <= MAX_FAMILY, f"at most {MAX_FAMILY} keys per family, {size} asked"
    assert cap & (cap - 1) == 0
    cand = np.nonzero((_row_hashes(table, N, pack) & _U64(cap - 1)) == _U64(home_slot % cap))[0]
    cand = cand[cand >= 1]
    assert cand.size >= skip + size, (f"only {cand.size} rows of table {table} (N = {N}) have home slot "
                                      f"{home_slot} of {cap}: {skip} + {size} asked")
    return cand[skip:skip + size]


def lds_only_family(table: int, N: int, cap: int, hs: int, lds_home: int, size: int, pack: Callable = dd_key,
                    min_global: int = 2) -> np.ndarray:
    """``size`` distinct rows of [1, N) equal in the low log2(hs) hash bits (one LDS home slot) but
    taken in turn from every global home slot of that class (cap / hs of them for cap > hs), so the
    chain exists in the LDS table only."""
    assert hs <= cap and hs & (hs - 1) == 0
    cand = np.nonzero((_row_hashes(table, N, pack) & _U64(hs - 1)) == _U64(lds_home))[0]
    cand = cand[cand >= 1]
    g = home(pack(table, cand), cap)
    classes = [cand[g == s] for s in np.unique(g)]
    assert len(classes) >= min_global, f"LDS class {lds_home} spans {len(classes)} global slots, {min_global} asked"
    out, i = [], 0
    while len(out) < size:
        took = False
        for c in classes:
            if i < c.size and len(out) < size:
                out.append(int(c[i]))
                took = True
        assert took, f"LDS class {lds_home} of table {table} has fewer than {size} rows below {N}"
        i += 1
    return np.asarray(out, np.int64)


def occupied_slots(keys, cap: int) -> set:
    """The slots linear probing fills for a set of packed keys: the same set whatever the insertion
    order (so a concurrent insert must produce it); which key sits where is order-dependent."""
    keys = np.unique(np.asarray(keys, dtype=_U64))
    assert keys.size < cap, "a full table: probing would not terminate"
    occ = set()
    for h in home(keys, cap).tolist():
        while h in occ:
            h = (h + 1) & (cap - 1)
        occ.add(h)
    return occ


@dataclass
class TableCheck:
    wraps: bool          # a cluster runs through cap - 1 -> 0
    displaced: int       # keys not at their home slot
    longest: int         # longest probe distance
    displaced_keys: List[int] = field(default_factory=list)


def check_placement(slot_key: Dict[int, int], keys, cap: int) -> TableCheck:
    """What is predicted of a table after the inserts of ``keys`` (any order, any interleaving):
    the filled slots are occupied_slots(keys); every key is there exactly once; every key lies in its
    cluster at or cyclically after its home slot (every slot from its home to it is filled)."""
    keys = np.unique(np.asarray(keys, dtype=_U64))
    want = occupied_slots(keys, cap)
    got = set(slot_key)
    assert got == want, (f"filled slots differ from linear probing's: {len(got - want)} unexpected "
                         f"{sorted(got - want)[:8]}, {len(want - got)} missing {sorted(want - got)[:8]}")
    vals = sorted(int(k) for k in slot_key.values())
    assert vals == [int(k) for k in keys.tolist()], "a key is missing from the table or sits in two slots"
    longest, disp = 0, []
    for s, k in slot_key.items():
        h = int(home([k], cap)[0])
        d = (s - h) & (cap - 1)
        for j in range(d):
            assert ((h + j) & (cap - 1)) in got, f"key {k:#x} at slot {s}: slot {(h + j) & (cap - 1)} of its probe path is free"
        longest = max(longest, d)
        if d:
            disp.append(int(k))
    return TableCheck(wraps=(cap - 1) in got and 0 in got, displaced=len(disp), longest=longest, displaced_keys=disp)


# ---- twin --------------------------------------------------------------------------------------------


def twin(ids: Sequence[np.ndarray], N: Sequence[int], drop_zero: bool = True):
    """Relabel the distinct rows of a batch, per table, onto rows 1..U in order of first appearance.
    ``ids[t]``: every id of table t in lookup order (several steps' columns concatenated share one
    relabeling); row = id floor-mod N[t]; ``drop_zero``: id 0 is a dropped lookup and stays 0.
    The lookup -> group partition of the twin is the adversarial batch's. Returns (twin ids, maps):
    maps[t][j] is the adversarial row whose twin is row j + 1."""
    out, maps = [], []
    for c, n in zip(ids, N):
        c = np.asarray(c)
        keep = c != 0 if drop_zero else np.ones(c.shape, bool)
        rows = np.mod(c[keep].astype(np.int64), n)
        u, first, inv = np.unique(rows, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")
        rank = np.empty(u.size, np.int64)
        rank[order] = np.arange(1, u.size + 1)
        assert u.size < n, "the twin needs rows 1..U below N"
        t = np.zeros(c.shape, np.int64)
        t[keep] = rank[inv.reshape(-1)]
        out.append(t.astype(c.dtype))
        maps.append(u[order].astype(np.int64))
    return out, maps


def partition(ids: np.ndarray, n: int, drop_zero: bool = True):
    """The groups of one table's lookups as (first position, size) pairs sorted by first position."""
    c = np.asarray(ids).astype(np.int64)
    pos = np.nonzero(c != 0)[0] if drop_zero else np.arange(c.size)
    rows = np.mod(c[pos], n)
    _, first, cnt = np.unique(rows, return_index=True, return_counts=True)
    o = np.argsort(first)
    return pos[first[o]], cnt[o]


# ---- patterns ----------------------------------------------------------------------------------------


@dataclass
class Pattern:
    name: str
    table: int
    rows: np.ndarray            # distinct rows of the family
    counts: np.ndarray          # lookups per row
    window: Optional[Tuple[int, int]] = None  # lookup positions [lo, hi) of its table it must stay in

    def lookups(self, rng) -> np.ndarray:
        """The pattern's lookups in an order that interleaves its keys."""
        x = np.repeat(self.rows, self.counts)
        return x[rng.permutation(x.size)]


DD_P3_COUNTS = (1, 2, DD_INL, DD_INL + 1, DD_INL + 2, 40)   # around the inline limit / hot threshold
PK_P3_COUNTS = (1, 2, HOT_MIN - 1, HOT_MIN, 600)            # around HOT_MIN, one row past HOT_SPLIT


def p1_one_home(table: int, N: int, cap: int, pack: Callable, home_slot: int, size: int = 48, skip: int = 0,
                window: Optional[Tuple[int, int]] = None) -> Pattern:
    assert size >= 48
    return Pattern("P1", table, family(table, N, cap, home_slot, size, pack, skip), np.ones(size, np.int64), window)


def p2_wrap(table: int, N: int, cap: int, pack: Callable, each: int = 8) -> Pattern:
    """Families homed at cap - 2 and cap - 1: 2 * each keys fill cap - 2, cap - 1, 0, 1, ..."""
    assert each >= 8
    rows = np.concatenate([family(table, N, cap, cap - 2, each, pack), family(table, N, cap, cap - 1, each, pack)])
    return Pattern("P2", table, rows, np.ones(rows.size, np.int64))


def p3_mixed_counts(table: int, N: int, cap: int, pack: Callable, home_slot: int, counts: Sequence[int]) -> Pattern:
    """One family whose keys have the given lookup counts: whichever insert wins the home slot, all
    the others (at least two hot ones) are displaced."""
    return Pattern("P3", table, family(table, N, cap, home_slot, len(counts), pack), np.asarray(counts, np.int64))


def p4_lds_only(table: int, N: int, cap: int, hs: int, pack: Callable, lds_home: int, window: Tuple[int, int],
                size: int = 128) -> Pattern:
    """A chain of ``size`` keys in one LDS table (all its lookups inside ``window``: one chunk / one
    insert workgroup), never more distinct keys than half the LDS slots."""
    assert 128 <= size <= hs // 2 and window[1] - window[0] <= hs // 2
    return Pattern("P4", table, lds_only_family(table, N, cap, hs, lds_home, size, pack), np.ones(size, np.int64), window)


def _stride(w: int) -> int:
    s = 67  # past one wave of 64: neighbours of a family are inserted by different waves / workgroups
    while gcd(s, w) != 1:
        s += 2
    return s


def _place(flat: np.ndarray, taken: np.ndarray, ids: np.ndarray, lo: int, hi: int,
           avoid: Optional[np.ndarray] = None) -> None:
    """ids at strided free positions of flat[lo:hi] (outside ``avoid``)."""
    w = hi - lo
    s = _stride(w)
    cand = lo + (np.arange(w, dtype=np.int64) * s) % w
    cand = cand[~taken[cand] & (True if avoid is None else ~avoid[cand])]
    assert cand.size >= ids.size, f"{ids.size} lookups do not fit the {cand.size} free positions of [{lo}, {hi})"
    flat[cand[:ids.size]] = ids
    taken[cand[:ids.size]] = True


def build_flat(n: int, patterns: Sequence[Pattern], N: int, rng, zeros: int = 4, shift_ids: bool = True,
               tail_distinct: bool = False) -> np.ndarray:
    """One table's n lookups (int64 ids): the patterns' lookups at strided positions (windowed ones
    first), ``zeros`` ids 0, a tail of ordinary random ids. ``shift_ids`` (column form: id floor-mod
    N is the row, id 0 dropped): ids moved by -N, 0, +N or +2N and the tail drawn from [-N, 3N).
    ``tail_distinct``: the tail holds distinct rows that are no pattern's row."""
    flat = np.zeros(n, np.int64)
    taken = np.zeros(n, bool)
    used = np.concatenate([p.rows for p in patterns]) if patterns else np.zeros(0, np.int64)
    windows = np.zeros(n, bool)  # a pattern without a window stays outside the others' windows
    for p in patterns:
        if p.window is not None:
            windows[p.window[0]:p.window[1]] = True
    for p in sorted(patterns, key=lambda p: p.window is None):
        ids = p.lookups(rng)
        if shift_ids:
            ids = ids + rng.integers(-1, 3, ids.size) * N
        if p.window is not None:
            _place(flat, taken, ids, p.window[0], p.window[1])
        else:
            _place(flat, taken, ids, 0, n, windows if int((~windows & ~taken).sum()) >= ids.size else None)
    free = np.nonzero(~taken)[0]
    assert free.size >= zeros, "no room for the dropped ids"
    free = free[rng.permutation(free.size)]
    tail_pos = free[zeros:]
    if tail_distinct:
        pool = np.setdiff1d(rng.choice(np.arange(1, N), size=min(N - 1, tail_pos.size + used.size + 64), replace=False), used)
        tail = pool[:tail_pos.size]
        assert tail.size == tail_pos.size
    else:
        tail = rng.integers(1, N, tail_pos.size)
    if shift_ids:
        tail = tail + rng.integers(-1, 3, tail.size) * N
        tail = np.where(tail == 0, N, tail)
    flat[tail_pos] = tail
    return flat


def cols_batch(B: int, N: Sequence[int], patterns: Sequence[Pattern], seed: int, zeros: int = 4) -> List[np.ndarray]:
    """Single-hot id columns [B] per table (feature t -> table t, lookup i = t * B + b)."""
    assert sum(int(p.counts.sum()) for p in patterns) + zeros * len(N) <= B * len(N)
    rng = np.random.default_rng(seed)
    return [build_flat(B, [p for p in patterns if p.table == t], n, rng, zeros) for t, n in enumerate(N)]


def kjt_batch(B: int, N: Sequence[int], patterns: Sequence[Pattern], totals: Sequence[int], seed: int, max_len: int = 20,
              full_tiles: Sequence[Tuple[int, int]] = (), full_len: int = 20, zeros: int = 2,
              tail_distinct: bool = False):
    """A key-major multi-hot KJT of len(N) features x B bags of 0..max_len ids, exactly totals[f]
    lookups of feature f (their sum <= the workspace's max_lookups). ``full_tiles``: (feature, tile)
    pairs whose TILE_BAGS bags all hold ``full_len`` ids — kjt_tile_window() of such a tile is the
    window of the patterns that must share one chunk. Ids are rows (no mod, id 0 is row 0). Returns
    (values int64, lengths int32 [F * B])."""
    assert B % TILE_BAGS == 0
    lengths = kjt_lengths(B, totals, seed, max_len, full_tiles, full_len)
    rng = np.random.default_rng(seed + 1)
    vals = [build_flat(int(totals[f]), [p for p in patterns if p.table == f], N[f], rng, zeros, shift_ids=False,
                       tail_distinct=tail_distinct) for f in range(len(N))]
    return np.concatenate(vals), lengths


def kjt_lengths(B: int, totals: Sequence[int], seed: int, max_len: int = 20,
                full_tiles: Sequence[Tuple[int, int]] = (), full_len: int = 20) -> np.ndarray:
    """Bag lengths 0..max_len summing to exactly totals[f] per feature (a full tile's bags fixed at
    full_len, two bags per feature empty)."""
    rng = np.random.default_rng(seed)
    F = len(totals)
    lengths = rng.integers(0, max_len + 1, F * B).astype(np.int64)
    fixed = np.zeros(F * B, bool)
    for f, tile in full_tiles:
        s = f * B + tile * TILE_BAGS
        lengths[s:s + TILE_BAGS] = full_len
        fixed[s:s + TILE_BAGS] = True
    for f in range(F):
        seg = np.arange(f * B, (f + 1) * B)
        empty = seg[~fixed[seg]][:2]
        lengths[empty] = 0
        fixed[empty] = True
        free = seg[~fixed[seg]]
        s = int(lengths[seg].sum())
        assert s - int(lengths[free].sum()) <= totals[f] <= s - int(lengths[free].sum()) + max_len * free.size
        while s != totals[f]:
            i = int(free[rng.integers(free.size)])
            if s < totals[f] and lengths[i] < max_len:
                lengths[i] += 1
                s += 1
            elif s > totals[f] and lengths[i] > 0:
                lengths[i] -= 1
                s -= 1
    return lengths.astype(np.int32)


def kjt_tile_window(lengths: np.ndarray, B: int, f: int, tile: int) -> Tuple[int, int]:
    """Positions [lo, hi), within feature f's lookups, of the lookups of its tile (TILE_BAGS bags)."""
    off = np.concatenate([[0], np.cumsum(lengths[f * B:(f + 1) * B].astype(np.int64))])
    return int(off[tile * TILE_BAGS]), int(off[(tile + 1) * TILE_BAGS])


def kjt_chunks(lengths: np.ndarray) -> List[Tuple[int, int]]:
    """(start, length) of every chunk bwd_tile_hash_kernel walks: per tile of TILE_BAGS bags of the
    F * B bags, its lookups in chunks of TILE_CH (csrc/embedding.hip, the j0 loop)."""
    off = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
    out = []
    for b0 in range(0, lengths.size, TILE_BAGS):
        s0, e0 = int(off[b0]), int(off[min(lengths.size, b0 + TILE_BAGS)])
        for j0 in range(s0, e0, TILE_CH):
            out.append((j0, min(TILE_CH, e0 - j0)))
    return out


def packed_keys(ids: Sequence[np.ndarray], N: Sequence[int], pack: Callable, drop_zero: bool = True) -> List[np.ndarray]:
    """Per table, the packed key of every lookup (0xffff...: dropped)."""
    out = []
    for t, (c, n) in enumerate(zip(ids, N)):
        c = np.asarray(c).astype(np.int64)
        k = pack(t, np.mod(c, n))
        if drop_zero:
            k = np.where(c != 0, k, _U64(0xFFFFFFFFFFFFFFFF))
        out.append(k)
    return out


# ---- the batches of the tests (the CPU test checks exactly what the GPU test runs) --------------------

N_ROWS = 1 << 21  # rows per table: every home slot of the tables below has > MAX_FAMILY candidate rows


def dedup_patterns(N: Sequence[int], cap: int, pack: Callable = dd_key,
                   p3_counts: Sequence[int] = DD_P3_COUNTS) -> List[Pattern]:
    """P1 and P2 on table 0, P3 on table 1 (stand-alone inserts: columns and segments)."""
    return [p1_one_home(0, N[0], cap, pack, 100), p2_wrap(0, N[0], cap, pack),
            p3_mixed_counts(1, N[1], cap, pack, cap // 2 + 9, p3_counts)]


def fused_patterns(N: Sequence[int], cap: int) -> List[Pattern]:
    """The fused steps (B = 512: lookups 0..511 table 0, 512..1023 table 1; one ring insert workgroup
    per INS_GROUP consecutive lookups): P4 inside the first workgroup and P2 on table 0, P1 and P3
    over both workgroups of table 1."""
    return [p4_lds_only(0, N[0], cap, INS_HS, dd_key, 7, (0, INS_GROUP)), p2_wrap(0, N[0], cap, dd_key),
            p1_one_home(1, N[1], cap, dd_key, 100), p3_mixed_counts(1, N[1], cap, dd_key, cap // 2 + 9, DD_P3_COUNTS)]


KJT_B, KJT_TOTAL, KJT_P4_TILE = 128, 2048, 3
KJT_TOTALS = (TILE_CH + 320, KJT_TOTAL - TILE_CH - 320)


def kjt_adversarial(N: Sequence[int], cap: int, seed: int):
    """2 x KJT_B bags of 0..20 ids, KJT_TOTAL lookups. Feature 0: one tile of 16 bags of 64 ids = ONE
    chunk of TILE_CH lookups (every thread of its workgroup holds up to 4 chunk entries) that
    carries P4 and a P1 family of home slot 100 (the batched global insert retries them in rounds);
    another P1 family of the same home slot and P2 spread over the other tiles. Feature 1: P3.
    Returns (values, lengths, patterns)."""
    full = [(0, KJT_P4_TILE)]
    lengths = kjt_lengths(KJT_B, KJT_TOTALS, seed, full_tiles=full, full_len=TILE_CH // TILE_BAGS)
    win = kjt_tile_window(lengths, KJT_B, 0, KJT_P4_TILE)
    pats = [p4_lds_only(0, N[0], cap, TILE_HS, pk_key, 11, win),
            p1_one_home(0, N[0], cap, pk_key, 100, skip=48, window=win),
            p1_one_home(0, N[0], cap, pk_key, 100), p2_wrap(0, N[0], cap, pk_key),
            p3_mixed_counts(1, N[1], cap, pk_key, cap // 2 + 9, PK_P3_COUNTS)]
    values, lengths2 = kjt_batch(KJT_B, N, pats, KJT_TOTALS, seed, full_tiles=full, full_len=TILE_CH // TILE_BAGS)
    assert np.array_equal(lengths, lengths2)
    return values, lengths, pats


def kjt_full_load(N: Sequence[int], cap: int, seed: int):
    """P5: exactly cap / 2 lookups, all distinct (the table at its designed maximum load), the P1 and
    P2 families among them. Returns (values, lengths, patterns)."""
    pats = [p1_one_home(0, N[0], cap, pk_key, 100), p2_wrap(0, N[0], cap, pk_key),
            p1_one_home(1, N[1], cap, pk_key, cap // 2 + 9)]
    values, lengths = kjt_batch(KJT_B, N, pats, (cap // 4, cap // 4), seed, zeros=1, tail_distinct=True)
    return values, lengths, pats


def kjt_split(values: np.ndarray, lengths: np.ndarray, B: int, F: int) -> List[np.ndarray]:
    """Per feature, its ids of a key-major KJT."""
    off = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
    return [values[off[f * B]:off[(f + 1) * B]] for f in range(F)]
